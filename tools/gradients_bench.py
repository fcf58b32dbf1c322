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

import json
import sys

import diag_bench

BYTES = {2: 37.0, 3: 77.0}      # compulsory bytes per cell of a stats pass
RECORDED_COPY_TBS = 6.29        # float4 device copy, MI355X (tools/fields_bench.py); recorded, not measured here
CLASSES = {"gradient_stats": "velocity_gradients stats", "gradients": "velocity_gradients",
           "field_stats": "macroscopic_fields stats"}


def worker(a) -> int:
    from lbm_amd import io as lio

    e, run, cells, grid, obst = diag_bench.engine(a)
    if a.dim == 2:
        vel = ("ux", "uy")
        host = lambda f: lio.velocity_gradients(f["ux"], f["uy"], obst)   # noqa: E731
    else:
        vel = ("ux", "uy", "uz")
        host = lambda f: lio.velocity_gradients3d(f["ux"], f["uy"], f["uz"], obst)   # noqa: E731
    print(f"gradients_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)

    calls = (("gradient_stats", e.gradient_stats), ("gradients", e.gradients), ("field_stats", e.field_stats),
             ("fields", lambda: e.fields(vel)), ("fields_numpy", lambda: host(e.fields(vel))))

    def line(r, name, dt, ms):
        return (f"  round {r} {name:16s} wall {dt * 1e3:10.3f} ms" +
                ("" if ms is None or name not in CLASSES else f"   {CLASSES[name]} {ms.get(CLASSES[name], 0.0):8.3f} ms"))

    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: (CLASSES.get(name),)), line)
    plain, hist = diag_bench.history_cost(run, lambda: e.gradient_history(100, 10), 3)
    e.close()
    med_wall = {k: diag_bench.median_wall(v) for k, v in got.items()}
    med_dev = {k: diag_bench.median_device(got[k], c) for k, c in CLASSES.items()}
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
        "run_ms": {"run_steps_100": round(plain * 1e3, 3), "gradient_history_100_every_10": round(hist * 1e3, 3)},
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


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__))
