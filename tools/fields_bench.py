#!/usr/bin/env python3
"""What does inspecting a run cost?  lbm_store vs lbm_store_fields on ONE handle.

On one engine (default 8192^2, equilibrium initialised on the device, 20
steps, LBM_FLAG_PROFILE) three calls are timed, interleaved round by round:

  (a) store(cells=True)       the nine populations: AoS staging + 36 B per cell to the host
  (b) fields()                u_x, u_y, |u|, pressure computed on the device: 16 B per cell
  (c) fields(("pressure",))   one field: 4 B per cell

Host wall time is taken around each call (it includes the result arrays the
binding allocates, as a caller's would); the device time of the
`macroscopic_fields` launch class comes from profile_summary().  Medians over
the rounds are printed, the kernel's device time also as achieved bytes/s on
53 B per cell (37 read + 16 written), next to the float4-copy rate of the
device (6.29 TB/s, MI355X), and one JSON line.  Exit status 1 when (b) is not
faster than (a): (b) moves less than half the bytes and stages less than half
the memory, so that is a bug.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/fields_bench.py [--n 8192] [--steps 20] [--rounds 5] [--limit 300]
"""
from __future__ import annotations

import json
import sys

import diag_bench

COPY_RATE_TBS = 6.29   # float4 device copy, MI355X (8.0 TB/s HBM3E spec)
CLASS = "macroscopic_fields"


def worker(a) -> int:
    from lbm_amd import io as lio
    from lbm_amd import native
    from bench import synthetic_obstacles

    nx, ny = a.n, a.ny or a.n
    cells = nx * ny
    p = lio.Params(nx, ny, a.steps, 10, 0.1, 0.005, 1.85)
    e = native.Engine(p, synthetic_obstacles(nx, ny), flags=native.FLAG_PROFILE)
    e.init_equilibrium()
    e.run_steps(a.steps, accelerate_first=True)
    print(f"fields_bench: {nx}x{ny}, {a.steps} steps, kernel {e.kernel_in_use()}, {a.rounds} rounds", flush=True)

    calls = (("store_cells", lambda: e.store(cells=True, n_av=0)), ("fields_all", lambda: e.fields()),
             ("fields_pressure", lambda: e.fields(("pressure",))))
    # round 0 warms up (first-touch of the staging sizes, clocks)
    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: (CLASS,)), lambda r, name, dt, ms: (
        f"  round {r} {name:16s} wall {dt * 1e3:10.2f} ms   macroscopic_fields {ms.get(CLASS, 0.0):8.3f} ms"))
    mass, umax = e.field_stats()
    e.close()
    med_wall = {k: diag_bench.median_wall(v) for k, v in got.items()}
    med_dev = {k: diag_bench.median_device(v, CLASS) for k, v in got.items()}
    rec = {
        "tool": "fields_bench", "grid": f"{nx}x{ny}", "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med_wall.items()},
        "macroscopic_fields_ms": {k: round(med_dev[k], 4) for k in ("fields_all", "fields_pressure")},
        "fields_all_tbs_53B": round(53.0 * cells / (med_dev["fields_all"] * 1e-3) / 1e12, 3)
        if med_dev["fields_all"] > 0 else None,
        "fields_pressure_tbs_41B": round(41.0 * cells / (med_dev["fields_pressure"] * 1e-3) / 1e12, 3)
        if med_dev["fields_pressure"] > 0 else None,
        "float4_copy_tbs": COPY_RATE_TBS,
        "mass": mass, "max_speed": umax,
        "fields_faster_than_store": med_wall["fields_all"] < med_wall["store_cells"],
    }
    print(f"median wall ms: (a) store(cells) {rec['wall_ms']['store_cells']}  (b) fields() "
          f"{rec['wall_ms']['fields_all']}  (c) fields(pressure) {rec['wall_ms']['fields_pressure']}")
    print(f"macroscopic_fields device ms: (b) {rec['macroscopic_fields_ms']['fields_all']} = "
          f"{rec['fields_all_tbs_53B']} TB/s on 53 B per cell; (c) {rec['macroscopic_fields_ms']['fields_pressure']} = "
          f"{rec['fields_pressure_tbs_41B']} TB/s on 41 B per cell (float4 copy: {COPY_RATE_TBS} TB/s)")
    print(json.dumps(rec), flush=True)
    return 0 if rec["fields_faster_than_store"] else 1


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, lambda ap: ap.add_argument("--ny", type=int, default=0),
                             dim=False, n=8192, limit=300))
