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

import json
import sys

import diag_bench

READ_BYTES = {2: 37.0, 3: 77.0}      # populations and one map byte per cell
CLASSES = {"strain_stats": "neq_strain stats", "strain_rate": "neq_strain", "field_stats": "macroscopic_fields stats",
           "gradient_stats": "velocity_gradients stats"}


def worker(a) -> int:
    from lbm_amd import native

    e, run, cells, grid, _ = diag_bench.engine(a)
    nfields = len(native.STRESS_FIELDS if a.dim == 2 else native.STRESS_FIELDS3D)
    print(f"stress_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)

    calls = (("strain_stats", e.strain_stats), ("strain_rate", e.strain_rate), ("field_stats", e.field_stats),
             ("gradient_stats", e.gradient_stats), ("fields", e.fields), ("gradients", e.gradients))

    def line(r, name, dt, ms):
        return (f"  round {r} {name:16s} wall {dt * 1e3:10.3f} ms" +
                ("" if ms is None or name not in CLASSES else f"   {CLASSES[name]} {ms.get(CLASSES[name], 0.0):8.3f} ms"))

    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: (CLASSES.get(name),)), line)
    plain, hist = diag_bench.history_cost(run, lambda: e.strain_history(100, 10), 3)
    stats = e.strain_stats()
    e.close()
    med_wall = {k: diag_bench.median_wall(v) for k, v in got.items()}
    med_dev = {k: diag_bench.median_device(got[k], c) for k, c in CLASSES.items()}
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
        "run_ms": {"run_steps_100": round(plain * 1e3, 3), "strain_history_100_every_10": round(hist * 1e3, 3)},
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


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__))
