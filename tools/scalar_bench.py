#!/usr/bin/env python3
"""What does carrying a passive scalar cost?  scalar_advance() against macroscopic_fields, run_scalar() against run_steps().

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, 20 steps) with a scalar begun
at zero and a short fixed list, these calls are timed, interleaved round by round
(round 0 warms up, medians of the rest):

  (a) scalar_advance(k)     k scalar steps over the frozen lattice, nothing to the host
  (b) the yardstick         the macroscopic-fields kernel of the same handle in the same
                            process: fields() (D2Q9: the `macroscopic_fields` launch class of
                            profile_summary()) or field_stats() (D3Q19, which has no profile
                            classes: the blocking call's wall time, a launch and the copy of
                            its block partials)
  (c) scalar_stats()        one stats launch and the fold of its partials

The device time of (a) is the `scalar_step` launch class per launch (D2Q9) or the
wall time of scalar_advance(k) / k (D3Q19).  Rates are on the bytes a kernel must
move per cell: the step kernel 77 B in 2-D (36 flow, 1 obstacle, 20 read, 20
written) and 133 B in 3-D (76, 1, 28, 28); the fields kernel 37 B read and 4 B per
field written (D2Q9, all four fields: 53 B), the stats launch 77 B (D3Q19).  The
yardstick is kernel (b), not a number from elsewhere: the step kernel should reach
at least 0.75 of (b)'s TB/s -- both are LDS-free streams over the same lattice; the
quarter covers the five (seven) extra store streams and the E and W planes one off
the alignment.  The tool reports the ratio and whether it is met; it always exits 0
when the measurement itself succeeded.

Then the coupled run: run_scalar(steps, stride) per step at stride 1 (the exact
coupling) and at the fused depth of the flow kernel, against run_steps(steps) alone
on the same handle (medians over the rounds).

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/scalar_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--k 10] [--coupled 60] [--limit 600]
"""
from __future__ import annotations

import json
import statistics
import sys
import time

import diag_bench

STEP_BYTES = {2: 77.0, 3: 133.0}


def worker(a) -> int:
    import numpy as np

    e, run, cells, grid, _ = diag_bench.engine(a)
    print(f"scalar_bench: {grid}, {a.steps} steps, {a.rounds} rounds, {a.k} scalar steps per advance", flush=True)
    e.scalar_begin(None, omega_s=1.3)
    n = e.params.nx
    mid = [np.array([n // 2, n // 2 + 1], np.int32)] * a.dim
    e.scalar_fix(*mid, np.array([1.0, 2.0], np.float32))
    if a.dim == 2:
        yard_call, yard_cls, yard_bytes = e.fields, "macroscopic_fields", 37.0 + 4.0 * 4
        depth = e.steps_per_launch()
    else:
        yard_call, yard_cls, yard_bytes = e.field_stats, None, 77.0
        depth = 3                                        # three-step passes
    calls = (("advance", lambda: e.scalar_advance(a.k)), ("yardstick", yard_call), ("stats", e.scalar_stats))
    classes = {"advance": ("scalar_step", "scalar_fixed"), "yardstick": (yard_cls,), "stats": ("scalar_stats",)}

    def line(r, name, dt, ms):
        return f"  round {r} {name:10s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}")

    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: classes[name]), line)
    if a.dim == 2:
        step_ms = diag_bench.median_device(got["advance"], "scalar_step") / a.k
        fixed_ms = diag_bench.median_device(got["advance"], "scalar_fixed") / a.k
        yard_ms = diag_bench.median_device(got["yardstick"], yard_cls)
        stats_ms = diag_bench.median_device(got["stats"], "scalar_stats")
    else:
        step_ms = diag_bench.median_wall(got["advance"]) * 1e3 / a.k
        fixed_ms = None
        yard_ms = diag_bench.median_wall(got["yardstick"]) * 1e3
        stats_ms = diag_bench.median_wall(got["stats"]) * 1e3
    tbs = lambda bytes_per_cell, ms: bytes_per_cell * cells / (ms * 1e-3) / 1e12      # noqa: E731
    step_tbs, yard_tbs = tbs(STEP_BYTES[a.dim], step_ms), tbs(yard_bytes, yard_ms)

    # the coupled run against the flow alone
    def per_step(call):
        t = []
        for r in range(a.rounds + 1):
            t0 = time.perf_counter()
            call()
            if r:
                t.append((time.perf_counter() - t0) / a.coupled * 1e3)
        return statistics.median(t)

    flow_ms = per_step(lambda: run(a.coupled))
    coupled = {s: per_step(lambda s=s: e.run_scalar(a.coupled, s)) for s in sorted({1, depth})}
    rec = {"tool": "scalar_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds, "k": a.k,
           "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking call",
           "step_ms": round(step_ms, 4), "step_bytes_per_cell": STEP_BYTES[a.dim], "step_tbs": round(step_tbs, 3),
           "fixed_ms": None if fixed_ms is None else round(fixed_ms, 4),
           "yardstick": "macroscopic_fields (fields())" if a.dim == 2 else "macroscopic_fields3d stats (field_stats())",
           "yardstick_ms": round(yard_ms, 4), "yardstick_bytes_per_cell": yard_bytes, "yardstick_tbs": round(yard_tbs, 3),
           "ratio": round(step_tbs / yard_tbs, 3), "meets_0.75": step_tbs >= 0.75 * yard_tbs,
           "stats_ms": round(stats_ms, 4),
           "advance_wall_ms_per_step": round(diag_bench.median_wall(got["advance"]) * 1e3 / a.k, 4),
           "coupled_steps": a.coupled, "fused_depth": depth, "run_steps_ms_per_step": round(flow_ms, 4),
           "run_scalar_ms_per_step": {str(s): round(v, 4) for s, v in coupled.items()}}
    e.close()
    print(f"scalar step {step_ms:.4f} ms = {step_tbs:.3f} TB/s on {STEP_BYTES[a.dim]:.0f} B per cell; yardstick "
          f"{rec['yardstick']} {yard_ms:.4f} ms = {yard_tbs:.3f} TB/s on {yard_bytes:.0f} B per cell; ratio "
          f"{rec['ratio']} ({'meets' if rec['meets_0.75'] else 'short of'} 0.75); stats {stats_ms:.4f} ms")
    print(f"per step over {a.coupled}: run_steps {flow_ms:.4f} ms; run_scalar " +
          ", ".join(f"stride {s} {v:.4f} ms" for s, v in coupled.items()))
    print(json.dumps(rec), flush=True)
    return 0


def _more(ap):
    ap.add_argument("--k", type=int, default=10, help="scalar steps per timed advance")
    ap.add_argument("--coupled", type=int, default=60, help="steps of each timed coupled run")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, _more))
