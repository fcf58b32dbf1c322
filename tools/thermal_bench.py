#!/usr/bin/env python3
"""What does the buoyancy kick cost?  scalar_buoyancy() against the scalar step, run_thermal() against run_scalar() and run_steps().

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, 20 steps) with a scalar begun
at zero, these calls are timed, interleaved round by round (round 0 warms up,
medians of the rest):

  (a) k times scalar_buoyancy(s, phi_ref)   the kick on the current lattice; s alternates its sign,
                                            so the lattice stays where it was
  (b) the yardstick: scalar_advance(k)      k scalar steps of the same handle in the same process

The device time is the launch class per launch (D2Q9: `scalar_buoyancy` against
`scalar_step` of profile_summary()) or the wall time of the blocking calls per kick /
per step (D3Q19, which has no profile classes; a kick's wall time holds its own
synchronisation and the ghost-plane refresh behind it, k steps of one advance share
one).  Rates are on the bytes a kernel must move per cell: the kick 85 B in 2-D (20
scalar read, 1 obstacle, 8 flow planes read and written) and 173 B in 3-D (28, 1,
18 x 8); the step 77 B and 133 B (tools/scalar_bench.py).  The yardstick is kernel
(b), not a number from elsewhere: the kick should reach at least 0.75 of (b)'s TB/s
-- both are LDS-free streams over the same two lattices.  The tool reports the ratio
and whether it is met; it always exits 0 when the measurement itself succeeded.

Then the coupled run per step: run_thermal(steps, accel, stride) at stride 1 (the
exact coupling) and at the fused depth of the flow kernel, against run_scalar() at
the same strides and run_steps() alone on the same handle (medians over the rounds).

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/thermal_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--k 10] [--coupled 60] [--limit 600]
"""
from __future__ import annotations

import json
import statistics
import sys
import time

import diag_bench

KICK_BYTES = {2: 85.0, 3: 173.0}
STEP_BYTES = {2: 77.0, 3: 133.0}
IMPULSE, PHI_REF = 1e-6, 0.5


def worker(a) -> int:
    e, run, cells, grid, _ = diag_bench.engine(a)
    print(f"thermal_bench: {grid}, {a.steps} steps, {a.rounds} rounds, {a.k} kicks / scalar steps per timed call",
          flush=True)
    e.scalar_begin(None, omega_s=1.3)
    depth = e.steps_per_launch() if a.dim == 2 else 3            # D3Q19: three-step passes
    s = [0.0] * (a.dim - 1) + [IMPULSE]

    def kicks():
        for i in range(a.k):
            e.scalar_buoyancy([c if i % 2 == 0 else -c for c in s], PHI_REF)

    calls = (("buoyancy", kicks), ("yardstick", lambda: e.scalar_advance(a.k)))
    classes = {"buoyancy": ("scalar_buoyancy",), "yardstick": ("scalar_step",)}

    def line(r, name, dt, ms):
        return f"  round {r} {name:10s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}")

    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: classes[name]), line)
    if a.dim == 2:
        kick_ms = diag_bench.median_device(got["buoyancy"], "scalar_buoyancy") / a.k
        step_ms = diag_bench.median_device(got["yardstick"], "scalar_step") / a.k
    else:
        kick_ms = diag_bench.median_wall(got["buoyancy"]) * 1e3 / a.k
        step_ms = diag_bench.median_wall(got["yardstick"]) * 1e3 / a.k
    tbs = lambda bytes_per_cell, ms: bytes_per_cell * cells / (ms * 1e-3) / 1e12      # noqa: E731
    kick_tbs, step_tbs = tbs(KICK_BYTES[a.dim], kick_ms), tbs(STEP_BYTES[a.dim], step_ms)

    # the coupled run against the passive one and the flow alone
    def per_step(call):
        t = []
        for r in range(a.rounds + 1):
            t0 = time.perf_counter()
            call()
            if r:
                t.append((time.perf_counter() - t0) / a.coupled * 1e3)
        return statistics.median(t)

    strides = sorted({1, depth})
    flow_ms = per_step(lambda: run(a.coupled))
    passive = {n: per_step(lambda n=n: e.run_scalar(a.coupled, n)) for n in strides}
    thermal = {n: per_step(lambda n=n: e.run_thermal(a.coupled, [c * 1e-3 for c in s], PHI_REF, n)) for n in strides}
    rec = {"tool": "thermal_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds, "k": a.k,
           "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking calls",
           "kick_ms": round(kick_ms, 4), "kick_bytes_per_cell": KICK_BYTES[a.dim], "kick_tbs": round(kick_tbs, 3),
           "yardstick": "scalar_step (scalar_advance())", "yardstick_ms": round(step_ms, 4),
           "yardstick_bytes_per_cell": STEP_BYTES[a.dim], "yardstick_tbs": round(step_tbs, 3),
           "ratio": round(kick_tbs / step_tbs, 3), "meets_0.75": kick_tbs >= 0.75 * step_tbs,
           "kick_wall_ms": round(diag_bench.median_wall(got["buoyancy"]) * 1e3 / a.k, 4),
           "coupled_steps": a.coupled, "fused_depth": depth, "run_steps_ms_per_step": round(flow_ms, 4),
           "run_scalar_ms_per_step": {str(n): round(v, 4) for n, v in passive.items()},
           "run_thermal_ms_per_step": {str(n): round(v, 4) for n, v in thermal.items()}}
    e.close()
    print(f"buoyancy kick {kick_ms:.4f} ms = {kick_tbs:.3f} TB/s on {KICK_BYTES[a.dim]:.0f} B per cell; yardstick "
          f"scalar step {step_ms:.4f} ms = {step_tbs:.3f} TB/s on {STEP_BYTES[a.dim]:.0f} B per cell; ratio "
          f"{rec['ratio']} ({'meets' if rec['meets_0.75'] else 'short of'} 0.75)")
    print(f"per step over {a.coupled}: run_steps {flow_ms:.4f} ms; " +
          "; ".join(f"stride {n}: run_scalar {passive[n]:.4f} ms, run_thermal {thermal[n]:.4f} ms" for n in strides))
    print(json.dumps(rec), flush=True)
    return 0


def _more(ap):
    ap.add_argument("--k", type=int, default=10, help="kicks / scalar steps per timed call")
    ap.add_argument("--coupled", type=int, default=60, help="steps of each timed coupled run")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, _more))
