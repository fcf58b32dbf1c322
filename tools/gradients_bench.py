#!/usr/bin/env python3
"""What do vorticity, strain and Q cost on the device?  gradient_stats() / gradients() vs fields() + numpy on ONE handle.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, a few steps) these calls
are timed, interleaved round by round (round 0 warms up, medians of the rest):

  (a) gradient_stats()            edge kernel, copies, one stats launch; four numbers to the host
  (b) gradients()                 the same pass storing every field, then the fields to the host
  (c) field_stats()               the yardstick: the per-cell stats pass over the same populations
  (d) fields(ux, uy[, uz])        what the library offered before: the velocities to the host ...
  (e) ... + numpy                 ... and lio.velocity_gradients[3d] there

Host wall time is taken around each call.  The device time of (a), (b) and (c) is
their launch class of profile_summary() (D2Q9: "velocity_gradients stats",
"velocity_gradients", "macroscopic_fields stats"; the D3Q19 engine has no profile
classes, so there the blocking call's wall time stands in: launch, copies and
synchronise included).  (a) is also printed as achieved bytes/s on the compulsory
37 B (D3Q19: 77 B) per cell -- nine (nineteen) populations and the obstacle byte,
each once -- next to the float4 device-copy rate tools/fields_bench.py records
(6.29 TB/s; not re-measured here), and as a ratio to (c).  The cost of
gradient_history(100, every=10) over run_steps(100) is reported.

Exit status 1 unless (a) is faster on the host clock than (d) alone: (a) moves
four numbers to the host, so anything else is a bug.  The ratio to (c) is reported,
not gated.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/gradients_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--limit 600]
"""
from __future__ import annotations

import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lbm-graphcore_amd")]

BYTES = {2: 37.0, 3: 77.0}      # compulsory bytes per cell of a stats pass
RECORDED_COPY_TBS = 6.29        # float4 device copy, MI355X (tools/fields_bench.py); recorded, not measured here
CLASSES = {"gradient_stats": "velocity_gradients stats", "gradients": "velocity_gradients",
           "field_stats": "macroscopic_fields stats"}


def worker(a) -> int:
    from lbm_amd import io as lio
    from lbm_amd import native

    if a.dim == 2:
        from bench import synthetic_obstacles
        n = a.n or 8192
        cells, grid = n * n, f"{n}x{n}"
        p = lio.Params(n, n, a.steps, 10, 0.1, 0.005, 1.85)
        obst = synthetic_obstacles(n, n)
        e = native.Engine(p, obst, flags=native.FLAG_PROFILE)
        vel = ("ux", "uy")
        run = lambda k: e.run_steps(k, accelerate_first=False)   # noqa: E731
        host = lambda f: lio.velocity_gradients(f["ux"], f["uy"], obst)   # noqa: E731
        history = lambda: e.gradient_history(100, 10)   # noqa: E731
    else:
        n = a.n or 256
        cells, grid = n ** 3, f"{n}^3"
        p = lio.Params3D(n, n, n, a.steps, 0.1, 0.001, 1.85)
        obst = lio.channel_obstacles3d(n, n, n)
        e = native.Engine3D(p, obst, devices=[0])
        vel = ("ux", "uy", "uz")
        run = e.run_steps
        host = lambda f: lio.velocity_gradients3d(f["ux"], f["uy"], f["uz"], obst)   # noqa: E731
        history = lambda: e.gradient_history(100, 10)   # noqa: E731
    e.init_equilibrium()
    run(a.steps)
    print(f"gradients_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)

    def device_ms(name):
        if a.dim != 2 or name not in CLASSES:
            return None
        k = [k for k in e.profile_summary() if k["name"] == CLASSES[name]]
        return k[0]["total_ms"] if k else 0.0

    def timed(name, call):
        if a.dim == 2:
            e.profile_reset()
        t0 = time.perf_counter()
        out = call()
        dt = time.perf_counter() - t0
        del out
        return dt, device_ms(name)

    calls = (("gradient_stats", e.gradient_stats), ("gradients", e.gradients), ("field_stats", e.field_stats),
             ("fields", lambda: e.fields(vel)), ("fields_numpy", lambda: host(e.fields(vel))))
    wall = {k: [] for k, _ in calls}
    dev = {k: [] for k in CLASSES}
    for r in range(a.rounds + 1):
        for name, call in calls:
            dt, ms = timed(name, call)
            if r > 0:
                wall[name].append(dt)
                if name in dev:
                    dev[name].append(dt * 1e3 if ms is None else ms)
            print(f"  round {r} {name:16s} wall {dt * 1e3:10.3f} ms" +
                  ("" if ms is None else f"   {CLASSES[name]} {ms:8.3f} ms"), flush=True)
    cost = {"run_steps_100": [], "gradient_history_100_every_10": []}
    for r in range(4):
        t0 = time.perf_counter()
        run(100)
        t1 = time.perf_counter()
        history()
        t2 = time.perf_counter()
        if r:
            cost["run_steps_100"].append(t1 - t0)
            cost["gradient_history_100_every_10"].append(t2 - t1)
    e.close()
    med_wall = {k: statistics.median(v) for k, v in wall.items()}
    med_dev = {k: statistics.median(v) for k, v in dev.items()}
    tbs = BYTES[a.dim] * cells / (med_dev["gradient_stats"] * 1e-3) / 1e12
    rec = {
        "tool": "gradients_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med_wall.items()},
        "device_ms": {k: round(v, 4) for k, v in med_dev.items()},
        "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking call",
        "bytes_per_cell": BYTES[a.dim],
        "gradient_stats_tbs": round(tbs, 3),
        "gradient_stats_over_field_stats": round(med_dev["gradient_stats"] / med_dev["field_stats"], 3),
        "device_copy_tbs_recorded": RECORDED_COPY_TBS,
        "run_ms": {k: round(statistics.median(v) * 1e3, 3) for k, v in cost.items()},
        "stats_faster_than_fields": med_wall["gradient_stats"] < med_wall["fields"],
    }
    w, d = rec["wall_ms"], rec["device_ms"]
    print(f"median wall ms: (a) gradient_stats() {w['gradient_stats']}  (b) gradients() {w['gradients']}  "
          f"(c) field_stats() {w['field_stats']}  (d) fields() {w['fields']}  (e) fields() + numpy {w['fields_numpy']}")
    print(f"device ms ({rec['device_time_source']}): (a) {d['gradient_stats']} = {rec['gradient_stats_tbs']} TB/s on "
          f"{BYTES[a.dim]:.0f} B per cell, {rec['gradient_stats_over_field_stats']} x (c) {d['field_stats']}; "
          f"(b) {d['gradients']} (recorded float4 device copy: {RECORDED_COPY_TBS} TB/s)")
    print(f"run_steps(100) {rec['run_ms']['run_steps_100']} ms; gradient_history(100, every=10) "
          f"{rec['run_ms']['gradient_history_100_every_10']} ms")
    print(json.dumps(rec), flush=True)
    return 0 if rec["stats_faster_than_fields"] else 1


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--dim", type=int, default=2, choices=(2, 3))
    ap.add_argument("--n", type=int, default=0, help="edge length (default 8192 for --dim 2, 256 for --dim 3)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=600, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rounds < 1:
        ap.error("--rounds must be >= 1")
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(__file__).resolve()), "--worker", "--dim",
           str(a.dim), "--n", str(a.n), "--steps", str(a.steps), "--rounds", str(a.rounds)]
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
