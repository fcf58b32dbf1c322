#!/usr/bin/env python3
"""What does the non-equilibrium strain rate cost on the device?  strain_stats() / strain_rate() vs fields() and gradients() on ONE handle.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, a few steps) these calls
are timed, interleaved round by round (round 0 warms up -- it also builds the
near-wall map -- medians of the rest):

  (a) strain_stats()       one stats launch over the populations and the class map; five numbers to the host
  (b) strain_rate()        the same pass storing every field (4 / 7), then the fields to the host
  (c) field_stats()        the yardstick: the per-cell stats pass over the same populations
  (d) gradient_stats()     the finite-difference statistics (edge kernel, copies, one stats launch)
  (e) fields()             every macroscopic field (4 / 5) to the host
  (f) gradients()          every finite-difference field (4 / 7) to the host

Host wall time is taken around each call.  The device time of (a) - (d) is their
launch class of profile_summary() (D2Q9: "neq_strain stats", "neq_strain",
"macroscopic_fields stats", "velocity_gradients stats"; the D3Q19 engine has no
profile classes, so there the blocking call's wall time stands in: launch, copies
and synchronise included).  (a) and (b) are also printed as achieved bytes/s on
their compulsory bytes: 36 B (D3Q19: 76 B) of populations read per cell, 1 B of
map, and 4 B per stored field for (b).  One pass, memory-bound: nothing is gated
but (a) being faster on the host clock than (e), which moves whole fields.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/stress_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--limit 600]
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

READ_BYTES = {2: 37.0, 3: 77.0}      # populations and one map byte per cell
CLASSES = {"strain_stats": "neq_strain stats", "strain_rate": "neq_strain", "field_stats": "macroscopic_fields stats",
           "gradient_stats": "velocity_gradients stats"}


def worker(a) -> int:
    from lbm_amd import io as lio
    from lbm_amd import native

    if a.dim == 2:
        from bench import synthetic_obstacles
        n = a.n or 8192
        cells, grid = n * n, f"{n}x{n}"
        p = lio.Params(n, n, a.steps, 10, 0.1, 0.005, 1.85)
        e = native.Engine(p, synthetic_obstacles(n, n), flags=native.FLAG_PROFILE)
        run = lambda k: e.run_steps(k, accelerate_first=False)   # noqa: E731
        nfields = len(native.STRESS_FIELDS)
    else:
        n = a.n or 256
        cells, grid = n ** 3, f"{n}^3"
        p = lio.Params3D(n, n, n, a.steps, 0.1, 0.001, 1.85)
        e = native.Engine3D(p, lio.channel_obstacles3d(n, n, n), devices=[0])
        run = e.run_steps
        nfields = len(native.STRESS_FIELDS3D)
    e.init_equilibrium()
    run(a.steps)
    print(f"stress_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)

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

    calls = (("strain_stats", e.strain_stats), ("strain_rate", e.strain_rate), ("field_stats", e.field_stats),
             ("gradient_stats", e.gradient_stats), ("fields", e.fields), ("gradients", e.gradients))
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
    cost = {"run_steps_100": [], "strain_history_100_every_10": []}
    for r in range(4):
        t0 = time.perf_counter()
        run(100)
        t1 = time.perf_counter()
        e.strain_history(100, 10)
        t2 = time.perf_counter()
        if r:
            cost["run_steps_100"].append(t1 - t0)
            cost["strain_history_100_every_10"].append(t2 - t1)
    stats = e.strain_stats()
    e.close()
    med_wall = {k: statistics.median(v) for k, v in wall.items()}
    med_dev = {k: statistics.median(v) for k, v in dev.items()}
    store_bytes = READ_BYTES[a.dim] + 4.0 * nfields
    rec = {
        "tool": "stress_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med_wall.items()},
        "device_ms": {k: round(v, 4) for k, v in med_dev.items()},
        "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking call",
        "stats_bytes_per_cell": READ_BYTES[a.dim], "store_bytes_per_cell": store_bytes,
        "strain_stats_tbs": round(READ_BYTES[a.dim] * cells / (med_dev["strain_stats"] * 1e-3) / 1e12, 3),
        "strain_rate_tbs": round(store_bytes * cells / (med_dev["strain_rate"] * 1e-3) / 1e12, 3),
        "strain_stats_over_field_stats": round(med_dev["strain_stats"] / med_dev["field_stats"], 3),
        "strain_stats_over_gradient_stats": round(med_dev["strain_stats"] / med_dev["gradient_stats"], 3),
        "run_ms": {k: round(statistics.median(v) * 1e3, 3) for k, v in cost.items()},
        "wall_cells": stats[2],
        "stats_faster_than_fields": med_wall["strain_stats"] < med_wall["fields"],
    }
    w, d = rec["wall_ms"], rec["device_ms"]
    print("median wall ms: " + "  ".join(f"{k}() {w[k]}" for k, _ in calls))
    print(f"device ms ({rec['device_time_source']}): strain_stats {d['strain_stats']} = {rec['strain_stats_tbs']} TB/s on "
          f"{READ_BYTES[a.dim]:.0f} B per cell, {rec['strain_stats_over_field_stats']} x field_stats {d['field_stats']}, "
          f"{rec['strain_stats_over_gradient_stats']} x gradient_stats {d['gradient_stats']}; strain_rate "
          f"{d['strain_rate']} = {rec['strain_rate_tbs']} TB/s on {store_bytes:.0f} B per cell")
    print(f"run_steps(100) {rec['run_ms']['run_steps_100']} ms; strain_history(100, every=10) "
          f"{rec['run_ms']['strain_history_100_every_10']} ms")
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
