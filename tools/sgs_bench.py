#!/usr/bin/env python3
"""What does the sub-grid model cost?  sgs_apply() against a whole-domain forcing zone, and run_les against run_steps.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, 20 steps) these calls are
timed, interleaved round by round (round 0 warms up, medians of the rest), each k
times per timed call:

  constant, constant+stats   Smagorinsky with one Cs for the domain (a kernel argument)
  plane, plane+stats         the same model with Cs from a coefficient plane
  omega                      the prescribed rate (no square root of the tensor's use, one divide more)
  nut                        eddy_viscosity(): the read-only form, staged and copied to the host
  empty                      no model set: the call returns before it launches
  yardstick                  forcing_apply() of one uniform whole-domain zone on the same handle

The device time is the launch class per launch (D2Q9: `sgs` and `forcing` of
profile_summary()) or the wall time of the blocking calls (D3Q19, which has no
profile classes; it holds the call's own synchronisation and the ghost-plane refresh
behind it).  Rates are on the bytes a kernel must move per cell: the filter 73 B in
2-D (36 read, 36 written, 1 obstacle byte) and 153 B in 3-D, 4 B more with a plane;
the forcing zone 69 B and 149 B (tools/forcing_bench.py).

One bar, reported and never enforced (the tool exits 0 when the measurement itself
succeeded): the constant form without the statistics should reach 0.75 of the
yardstick's rate.  Then the loops: run_les(steps) per step at stride 1 and at the
fused depth beside run_steps(steps), medians of the same number of rounds.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/sgs_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--k 10] [--loop 60] [--limit 600]
"""
from __future__ import annotations

import json
import statistics
import sys
import time

import numpy as np

import diag_bench

FILTER_BYTES = {2: 73.0, 3: 153.0}
PLANE_BYTES = {2: 77.0, 3: 157.0}
ZONE_BYTES = {2: 69.0, 3: 149.0}
CS, RATE, BAR = 0.17, 1.2, 0.75


def worker(a) -> int:
    e, run, cells, grid, _ = diag_bench.engine(a)
    n = a.n or (8192 if a.dim == 2 else 256)
    print(f"sgs_bench: {grid}, {a.steps} steps, {a.rounds} rounds, {a.k} applications per timed call", flush=True)
    dims = a.dim
    whole, origin = (n,) * dims, (0,) * dims
    e.forcing_zone(0, origin, whole, 0.01, [0.01] + [0.0] * (dims - 1), [1e-6] + [0.0] * (dims - 1))
    cs_plane = np.full(whole, CS, np.float32)
    current = [None]

    def model(kind):
        if kind == current[0]:
            return
        current[0] = kind
        if kind in ("constant", "nut"):
            e.sgs_model("smagorinsky", CS)
        elif kind == "plane":
            e.sgs_model("smagorinsky", cs_plane)
        elif kind == "omega":
            e.sgs_model("omega", RATE)
        else:
            e.sgs_model("off")

    def applies(stats):
        def call():
            for _ in range(a.k):
                e.sgs_apply(1.0, stats=stats)
        return call

    def nuts():
        for _ in range(a.k):
            e.eddy_viscosity()

    def zones():
        for _ in range(a.k):
            e.forcing_apply(1.0)

    calls = (("constant", applies(False)), ("constant+stats", applies(True)), ("plane", applies(False)),
             ("plane+stats", applies(True)), ("omega", applies(False)), ("nut", nuts), ("empty", applies(False)),
             ("yardstick", zones))
    cls = lambda name: ("forcing",) if name == "yardstick" else ("sgs nut",) if name == "nut" else ("sgs",)   # noqa: E731

    def line(r, name, dt, ms):
        return f"  round {r} {name:16s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}")

    def measure():
        for name, call in calls:
            model(name.split("+")[0])                    # the model is set outside the timed call
            yield (name, *diag_bench.timed(e, call, cls(name)))

    got = diag_bench.rounds(a.rounds, measure, line)

    def per_call(name):
        """ms per application: device time where the engine has profile classes, else wall time."""
        if a.dim == 2 and name != "empty":
            return diag_bench.median_device(got[name], cls(name)[0]) / a.k
        return diag_bench.median_wall(got[name]) * 1e3 / a.k

    ms = {name: per_call(name) for name, _ in calls}
    tbs = lambda bytes_per_cell, t: bytes_per_cell * cells / (t * 1e-3) / 1e12      # noqa: E731
    rate = {"constant": tbs(FILTER_BYTES[dims], ms["constant"]), "constant+stats": tbs(FILTER_BYTES[dims], ms["constant+stats"]),
            "plane": tbs(PLANE_BYTES[dims], ms["plane"]), "plane+stats": tbs(PLANE_BYTES[dims], ms["plane+stats"]),
            "omega": tbs(FILTER_BYTES[dims], ms["omega"]), "yardstick": tbs(ZONE_BYTES[dims], ms["yardstick"])}
    ratio = rate["constant"] / rate["yardstick"]

    # the loops: seconds per step of run_steps, run_les at stride 1 and at the fused depth
    depth = e.steps_per_launch() if hasattr(e, "steps_per_launch") else 3
    e.forcing_clear()
    model("constant")
    loops = {"run_steps": lambda: run(a.loop), "run_les stride 1": lambda: e.run_les(a.loop, 1),
             f"run_les stride {depth}": lambda: e.run_les(a.loop, depth)}
    per_step = {k: [] for k in loops}
    for r in range(a.rounds + 1):
        for name, call in loops.items():
            t0 = time.perf_counter()
            call()
            dt = time.perf_counter() - t0
            if r:
                per_step[name].append(dt / a.loop * 1e3)
    loop_ms = {k: statistics.median(v) for k, v in per_step.items()}

    rec = {"tool": "sgs_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds, "k": a.k,
           "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking calls",
           "ms": {k: round(v, 5) for k, v in ms.items()}, "tbs": {k: round(v, 3) for k, v in rate.items()},
           "wall_ms": {name: round(diag_bench.median_wall(got[name]) * 1e3 / a.k, 5) for name, _ in calls},
           "bytes_per_cell": {"filter": FILTER_BYTES[dims], "plane": PLANE_BYTES[dims], "yardstick": ZONE_BYTES[dims]},
           "ratio_to_yardstick": round(ratio, 3), "bar": BAR, "meets_bar": ratio >= BAR,
           "loop_steps": a.loop, "fused_depth": depth, "ms_per_step": {k: round(v, 5) for k, v in loop_ms.items()}}
    e.close()
    print("; ".join(f"{k} {ms[k]:.4f} ms" + (f" = {rate[k]:.3f} TB/s" if k in rate else "") for k, _ in calls))
    print(f"constant {rate['constant']:.3f} TB/s against the yardstick's {rate['yardstick']:.3f} TB/s: ratio {ratio:.3f}, "
          f"{'meets' if rec['meets_bar'] else 'short of'} the bar {BAR}")
    print("; ".join(f"{k} {v:.4f} ms/step" for k, v in loop_ms.items()))
    print(json.dumps(rec), flush=True)
    return 0


def _more(ap):
    ap.add_argument("--k", type=int, default=10, help="applications per timed call")
    ap.add_argument("--loop", type=int, default=60, help="steps per timed loop")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, _more))
