#!/usr/bin/env python3
"""What does a force sample cost?  The wall-force calls next to the alternatives.

On one D2Q9 handle (default 8192^2, LBM_FLAG_PROFILE, equilibrium + 20 steps)
and one D3Q19 handle (default 256^3), each with two obstacle sets --

  sparse   channel walls plus a few box bodies (what a drag / lift run looks like)
  random   10 % random obstacles (every obstacle cell a wall cell, ~10^5-10^6 bodies)

-- these calls are timed, interleaved round by round after a warm-up round:

  wall_force()         total force: a gather over the wall list
  body_forces()        per-body sums on the device (bodies of lio.label_bodies)
  wall_force_field()   the planar per-cell map
  field_stats()        the existing whole-lattice reduction (reads every population)
  store() + numpy      what a caller had to do before: all populations to the host,
                       lio.wall_force there (one round only: it takes seconds)

and, 2-D only, the cost force_history(steps, every=10) adds per step over plain
run_steps(steps).  Host wall time is taken around each call; for 2-D the device
time of the launch classes comes from profile_summary().  Medians are printed
and one JSON line per case.  Exit status 1 when wall_force() on the sparse set
is not faster than field_stats(): the wall list would not be doing its job.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/force_bench.py [--n 8192] [--n3 256] [--steps 20] [--rounds 5] [--limit 900] [--only 2d|3d]
"""
from __future__ import annotations

import json
import statistics
import sys
import time

import numpy as np

import diag_bench


def obstacles2d(nx, ny, kind):
    o = np.zeros((ny, nx), np.uint8)
    if kind == "random":
        o[np.random.default_rng(1).random((ny, nx)) < 0.1] = 1
        return o
    o[0] = o[-1] = 1
    s = max(nx // 32, 2)
    for cx, cy in ((nx // 4, ny // 2), (nx // 2, ny // 3), (3 * nx // 4, 2 * ny // 3)):
        o[cy - s:cy + s, cx - s:cx + s] = 1
    return o


def obstacles3d(n, kind):
    from lbm_amd import io as lio
    o = lio.channel_obstacles3d(n, n, n).copy()
    if kind == "random":
        o[np.random.default_rng(1).random((n, n, n)) < 0.1] = 1
        return o
    s = max(n // 16, 1)
    for c in (n // 4, 5 * n // 8):
        o[c - s:c + s, n // 2 - s:n // 2 + s, c - s:c + s] = 1
    return o


def timed_rounds(calls, rounds, once, device_ms=None, reset=None):
    wall = {k: [] for k in calls}
    dev = {k: [] for k in calls}
    for r in range(rounds + 1):   # round 0 warms up (wall list build, staging sizes, clocks)
        for name, call in calls.items():
            if name in once and r != 1:
                continue
            if reset:
                reset()
            t0 = time.perf_counter()
            out = call()
            dt = time.perf_counter() - t0
            del out
            d = device_ms(name) if device_ms else None
            if r > 0:
                wall[name].append(dt)
                dev[name].append(d)
            print(f"    round {r} {name:20s} wall {dt * 1e3:10.3f} ms" + (f"   device {d:8.4f} ms" if d is not None else ""),
                  flush=True)
    med = {k: round(statistics.median(v) * 1e3, 4) for k, v in wall.items() if v}
    medd = {k: round(statistics.median(v), 4) for k, v in dev.items() if v and v[0] is not None}
    return med, medd


def case2d(a, kind):
    from lbm_amd import io as lio
    from lbm_amd import native
    nx = ny = a.n
    obst = obstacles2d(nx, ny, kind)
    t0 = time.perf_counter()
    labels, nbodies = lio.label_bodies(obst)
    t_label = time.perf_counter() - t0
    links = lio.wall_links(obst)
    nwall = int((links != 0).sum())
    del links
    p = lio.Params(nx, ny, a.steps, 10, 0.1, 0.005, 1.85)
    e = native.Engine(p, obst, flags=native.FLAG_PROFILE)
    e.init_equilibrium()
    e.run_steps(a.steps, accelerate_first=True)
    t0 = time.perf_counter()
    e.wall_force()
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    e.set_bodies(labels, nbodies)
    t_bodies = time.perf_counter() - t0
    print(f"  2-D {kind}: {nx}x{ny}, kernel {e.kernel_in_use()}, {nwall} wall cells, {nbodies} bodies "
          f"(label_bodies {t_label:.2f} s, first wall_force with the list build {t_build:.2f} s, set_bodies {t_bodies:.2f} s)",
          flush=True)
    cls = {"wall_force": "wall_force", "body_forces": "wall_force bodies", "wall_force_field": "wall_force map",
           "field_stats": "macroscopic_fields stats"}

    def device_ms(name):
        k = [k for k in e.profile_summary() if k["name"] == cls.get(name)]
        return k[0]["total_ms"] if k else None

    def store_numpy():
        cells, _ = e.store(n_av=0)
        return lio.wall_force(obst, cells)

    calls = {"wall_force": e.wall_force, "body_forces": e.body_forces, "wall_force_field": e.wall_force_field,
             "field_stats": e.field_stats, "store_numpy": store_numpy}
    wall, dev = timed_rounds(calls, a.rounds, {"store_numpy"}, device_ms, e.profile_reset)
    # force_history(every=10) against plain run_steps, the same number of steps, interleaved
    steps = a.hsteps
    plain, hist = diag_bench.history_cost(e.run_steps, lambda: e.force_history(steps, 10), a.rounds, steps)
    per_step_us = (hist - plain) / steps * 1e6
    e.close()
    rec = {"tool": "force_bench", "case": f"2d {kind}", "grid": f"{nx}x{ny}", "wall_cells": nwall, "bodies": nbodies,
           "wall_ms": wall, "device_ms": dev, "list_build_s": round(t_build, 3), "set_bodies_s": round(t_bodies, 3),
           "run_steps_ms": round(plain * 1e3, 3),
           "force_history_every10_ms": round(hist * 1e3, 3), "history_steps": steps,
           "force_history_added_us_per_step": round(per_step_us, 3)}
    print(json.dumps(rec), flush=True)
    return rec


def case3d(a, kind):
    from lbm_amd import io as lio
    from lbm_amd import native
    n = a.n3
    obst = obstacles3d(n, kind)
    t0 = time.perf_counter()
    labels, nbodies = lio.label_bodies(obst)
    t_label = time.perf_counter() - t0
    nwall = int((lio.wall_links3d(obst) != 0).sum())
    p = lio.Params3D(n, n, n, 0, 0.1, 0.002, 1.7)
    e = native.Engine3D(p, obst, devices=[0])
    e.init_equilibrium()
    e.run_steps(a.steps)
    t0 = time.perf_counter()
    e.wall_force()
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    e.set_bodies(labels, nbodies)
    t_bodies = time.perf_counter() - t0
    print(f"  3-D {kind}: {n}^3, {nwall} wall cells, {nbodies} bodies (label_bodies {t_label:.2f} s, first wall_force "
          f"with the list build {t_build:.2f} s, set_bodies {t_bodies:.2f} s)", flush=True)

    def store_numpy():
        cells, _ = e.store()
        return lio.wall_force3d(obst, cells)

    calls = {"wall_force": e.wall_force, "body_forces": e.body_forces, "wall_force_field": e.wall_force_field,
             "field_stats": e.field_stats, "store_numpy": store_numpy}
    wall, _ = timed_rounds(calls, a.rounds, {"store_numpy"})
    e.close()
    rec = {"tool": "force_bench", "case": f"3d {kind}", "grid": f"{n}^3", "wall_cells": nwall, "bodies": nbodies,
           "wall_ms": wall, "list_build_s": round(t_build, 3), "set_bodies_s": round(t_bodies, 3)}
    print(json.dumps(rec), flush=True)
    return rec


def worker(a) -> int:
    ok = True
    for dims, case in (("2d", case2d), ("3d", case3d)):
        if a.only and a.only != dims:
            continue
        for kind in ("sparse", "random"):
            if a.kind and a.kind != kind:
                continue
            rec = case(a, kind)
            w = rec["wall_ms"]
            print(f"  {rec['case']}: median wall ms " + "  ".join(f"{k} {v}" for k, v in w.items()), flush=True)
            if kind == "sparse" and not w["wall_force"] < w["field_stats"]:
                print("  wall_force() on the sparse set is NOT faster than field_stats()", flush=True)
                ok = False
    return 0 if ok else 1


def more_arguments(ap) -> None:
    ap.add_argument("--n3", type=int, default=256)
    ap.add_argument("--hsteps", type=int, default=100, help="steps of the force_history comparison")
    ap.add_argument("--only", choices=("2d", "3d"), default="")
    ap.add_argument("--kind", choices=("sparse", "random"), default="")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, more_arguments, dim=False, n=8192, limit=900))
