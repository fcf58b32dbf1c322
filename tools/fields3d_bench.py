#!/usr/bin/env python3
"""What does inspecting a D3Q19 run cost?  lbm3d_store vs lbm3d_store_fields on ONE handle.

On one Engine3D (default 256^3 channel, equilibrium initialised on the
device, a few steps) four calls are timed, interleaved round by round:

  (a) store(cells=True)        the 19 populations: AoS staging + 76 B per cell to the host
  (b) fields()                 u_x, u_y, u_z, |u|, pressure computed on the device: 20 B per cell
  (c) fields(("pressure",))    one field: 4 B per cell
  (d) fields_box(z-slice)      all five fields of the middle z plane: 20 B per cell of the plane

Host wall time is taken around each call (it includes the result arrays the
binding allocates, as a caller's would).  Medians over the rounds are
printed, then field_stats() (timed once per round) and one JSON line.  Exit
status 1 when (b) is not faster than (a): (b) moves 20 B per cell against 76
and stages about a quarter of the memory, so that is a bug.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/fields3d_bench.py [--n 256] [--steps 6] [--rounds 5] [--limit 600]
"""
from __future__ import annotations

import json
import sys

import diag_bench


def worker(a) -> int:
    from lbm_amd import io as lio
    from lbm_amd import native

    n = a.n
    cells = n ** 3
    p = lio.Params3D(n, n, n, a.steps, 0.1, 0.001, 1.85)
    e = native.Engine3D(p, lio.channel_obstacles3d(n, n, n), devices=[0])
    e.init_equilibrium()
    e.run_steps(a.steps)
    print(f"fields3d_bench: {n}^3, {a.steps} steps, {a.rounds} rounds", flush=True)

    calls = (("store_cells", lambda: e.store(cells=True)), ("fields_all", lambda: e.fields()),
             ("fields_pressure", lambda: e.fields(("pressure",))),
             ("box_z_slice", lambda: e.fields_box(0, 0, n // 2, n, n, 1)), ("field_stats", lambda: e.field_stats()))
    # round 0 warms up (first touch of the staging sizes, clocks)
    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: ()),
                            lambda r, name, dt, ms: f"  round {r} {name:16s} wall {dt * 1e3:10.2f} ms")
    mass, umax = e.field_stats()
    e.close()
    med = {k: diag_bench.median_wall(v) for k, v in got.items()}
    rec = {
        "tool": "fields3d_bench", "grid": f"{n}^3", "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med.items()},
        "host_gbs": {"store_cells": round(76.0 * cells / med["store_cells"] / 1e9, 2),
                     "fields_all": round(20.0 * cells / med["fields_all"] / 1e9, 2),
                     "fields_pressure": round(4.0 * cells / med["fields_pressure"] / 1e9, 2)},
        "mass": mass, "max_speed": umax,
        "fields_faster_than_store": med["fields_all"] < med["store_cells"],
    }
    w = rec["wall_ms"]
    print(f"median wall ms: (a) store(cells) {w['store_cells']}  (b) fields() {w['fields_all']}  "
          f"(c) fields(pressure) {w['fields_pressure']}  (d) z-slice box {w['box_z_slice']}  "
          f"field_stats {w['field_stats']}")
    print(json.dumps(rec), flush=True)
    return 0 if rec["fields_faster_than_store"] else 1


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, dim=False, n=256, steps=6))
