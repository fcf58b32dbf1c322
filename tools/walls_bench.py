#!/usr/bin/env python3
"""What do the scalar wall models cost?  scalar_advance() with and without walls on one handle.

On one engine (default 8192^2, or --dim 3: 256^3; equilibrium initialised on the device, 20 steps) with a
scalar begun at 1 and a wall set of well under 1 % of the cells -- the two channel walls as one
fixed-value body plus --bodies small bodies (discs of radius 20 in 2-D, cubes of 3^3 in 3-D; fixed value,
fixed flux and adiabatic in turn) -- these calls are timed, interleaved round by round (round 0 warms up,
medians of the rest):

  (a) scalar_advance(K) with the walls set        per step: the step launches and the wall pass
  (b) scalar_advance(K) after scalar_walls(None)  per step: the same handle without walls
  (c) scalar_stats()                              the yardstick: one full pass over the cells
  (d) scalar_body_flux()                          one sample of the per-body sums
  (e) scalar_wall_flux(), scalar_wall_flux_field()

The hard condition, which decides the exit status: the per-step time the walls add, (a) - (b), is below
one scalar_stats() -- the pass is O(wall cells), not O(cells).  Both are taken from the launch classes of
profile_summary() in 2-D (`scalar_walls` per launch against `scalar_stats`) and from the wall time of the
blocking calls in both dimensions; every form measured must hold.

Second comparison: one scalar_body_flux() against the host route, scalar(populations=True) plus
lio.scalar_wall_flux[3d] (once: it takes seconds).

The measurement runs in a child process under `timeout`, so a hang ends it; the JSON record also goes to
--out (default profiles/walls/):

  python tools/walls_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--advance 20] [--bodies 400] [--out DIR]
"""
from __future__ import annotations

import json
import sys
import time
from pathlib import Path

import diag_bench


def wall_set(a, np, lio):
    """(obst, labels, kinds, values): the channel walls (body 0, fixed value) and a.bodies small bodies."""
    rng = np.random.default_rng(7)
    if a.dim == 2:
        n = a.n or 8192
        obst = np.zeros((n, n), np.uint8)
        labels = np.full((n, n), -1, np.int32)
        obst[0], obst[-1], labels[0], labels[-1] = 1, 1, 0, 0
        r = max(1, min(20, n // 64))
        side = int(np.ceil(np.sqrt(a.bodies)))
        pitch = (n - 4 * r) // max(side, 1)
        yy, xx = np.mgrid[-r:r + 1, -r:r + 1]
        disc = (yy * yy + xx * xx <= r * r)
        for b in range(a.bodies):
            cy, cx = 3 * r + (b // side) * pitch, 3 * r + (b % side) * pitch + int(rng.integers(0, max(pitch - 2 * r - 2, 1)))
            obst[cy - r:cy + r + 1, cx - r:cx + r + 1][disc] = 1
            labels[cy - r:cy + r + 1, cx - r:cx + r + 1][disc] = 1 + b
    else:
        n = a.n or 256
        obst = lio.channel_obstacles3d(n, n, n).astype(np.uint8)
        labels = np.where(obst != 0, 0, -1).astype(np.int32)
        side = int(np.ceil(a.bodies ** (1.0 / 3.0)))
        pitch = (n - 8) // max(side, 1)
        for b in range(a.bodies):
            c = [4 + ((b // side ** i) % side) * pitch + pitch // 2 for i in range(3)]
            sl = tuple(slice(v - 1, v + 2) for v in c)
            if obst[sl].any():
                continue
            obst[sl], labels[sl] = 1, 1 + b
    nb = 1 + a.bodies
    kinds = np.concatenate([[1], (np.arange(a.bodies) % 3 + 1) % 3]).astype(np.int32)
    values = np.where(kinds == 2, 0.001, 2.0).astype(np.float32)
    assert kinds.size == nb
    return obst, labels, kinds, values


def worker(a) -> int:
    import numpy as np
    from lbm_amd import io as lio
    from lbm_amd import native

    obst, labels, kinds, values = wall_set(a, np, lio)
    links = (lio.scalar_wall_links if a.dim == 2 else lio.scalar_wall_links3d)(obst)
    wall_cells, cells = int((links != 0).sum()), int(obst.size)
    del links
    if a.dim == 2:
        n = obst.shape[0]
        grid = f"{n}x{n}"
        e = native.Engine(lio.Params(n, n, a.steps, 10, 0.1, 0.005, 1.85), obst, flags=native.FLAG_PROFILE)
        e.init_equilibrium()
        e.run_steps(a.steps, accelerate_first=False)
    else:
        n = obst.shape[0]
        grid = f"{n}^3"
        e = native.Engine3D(lio.Params3D(n, n, n, a.steps, 0.1, 0.001, 1.85), obst, devices=[0])
        e.init_equilibrium()
        e.run_steps(a.steps)
    print(f"walls_bench: {grid}, {wall_cells} wall cells = {100.0 * wall_cells / cells:.3f} % of the cells, "
          f"{kinds.size} bodies, {a.rounds} rounds of scalar_advance({a.advance})", flush=True)
    e.scalar_begin(np.ones(obst.shape, np.float32), omega_s=1.3)
    t0 = time.perf_counter()
    e.scalar_walls(labels, kinds, values)
    build_s = time.perf_counter() - t0
    e.scalar_advance(2)

    def with_walls():
        e.scalar_advance(a.advance)

    def without_walls():
        e.scalar_advance(a.advance)

    classes = {"advance walls": ("scalar_step", "scalar_walls"), "advance plain": ("scalar_step", "scalar_walls"),
               "scalar_stats": ("scalar_stats",), "body_flux": ("scalar_wall_flux bodies",),
               "wall_flux": ("scalar_wall_flux",), "flux_field": ("scalar_wall_flux map",)}
    kept = {name: [] for name in classes}
    for r in range(a.rounds + 1):
        for name, call in (("advance walls", with_walls), ("scalar_stats", e.scalar_stats),
                           ("body_flux", e.scalar_body_flux), ("wall_flux", e.scalar_wall_flux),
                           ("flux_field", e.scalar_wall_flux_field)):
            dt, ms = diag_bench.timed(e, call, classes[name])
            print(f"  round {r} {name:14s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}"), flush=True)
            if r:
                kept[name].append((dt, ms))
        e.scalar_walls(None, 0)                                   # the same handle without walls
        dt, ms = diag_bench.timed(e, without_walls, classes["advance plain"])
        print(f"  round {r} {'advance plain':14s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}"),
              flush=True)
        if r:
            kept["advance plain"].append((dt, ms))
        e.scalar_walls(labels, kinds, values)
        e.scalar_advance(1)                                       # the flux has its meaning after an advance

    wall_ms = lambda name: diag_bench.median_wall(kept[name]) * 1e3      # noqa: E731
    step_walls, step_plain = wall_ms("advance walls") / a.advance, wall_ms("advance plain") / a.advance
    added = step_walls - step_plain
    stats = wall_ms("scalar_stats")
    rec = {"tool": "walls_bench", "grid": grid, "wall_cells": wall_cells, "wall_cell_share": wall_cells / cells,
           "bodies": int(kinds.size), "rounds": a.rounds, "advance": a.advance, "set_walls_s": round(build_s, 3),
           "step_with_walls_ms": round(step_walls, 4), "step_without_walls_ms": round(step_plain, 4),
           "added_ms_per_step": round(added, 4), "added_over_step": round(added / step_plain, 4),
           "scalar_stats_wall_ms": round(stats, 4), "body_flux_wall_ms": round(wall_ms("body_flux"), 4),
           "wall_flux_wall_ms": round(wall_ms("wall_flux"), 4), "flux_field_wall_ms": round(wall_ms("flux_field"), 4)}
    ok = added < stats
    rec["added_below_one_scalar_stats"] = ok
    if a.dim == 2:
        dev = lambda name, cls: diag_bench.median_device(kept[name], cls)   # noqa: E731
        rec["device_ms"] = {"scalar_step_per_launch": round(dev("advance plain", "scalar_step") / a.advance, 4),
                            "scalar_walls_per_launch": round(dev("advance walls", "scalar_walls") / a.advance, 5),
                            "scalar_stats": round(dev("scalar_stats", "scalar_stats"), 4),
                            "scalar_wall_flux bodies": round(dev("body_flux", "scalar_wall_flux bodies"), 5),
                            "scalar_wall_flux": round(dev("wall_flux", "scalar_wall_flux"), 5),
                            "scalar_wall_flux map": round(dev("flux_field", "scalar_wall_flux map"), 5)}
        rec["device_pass_below_one_scalar_stats"] = \
            rec["device_ms"]["scalar_walls_per_launch"] < rec["device_ms"]["scalar_stats"]
        ok = ok and rec["device_pass_below_one_scalar_stats"]
        print(f"device: {rec['device_ms']}", flush=True)
    print(f"per step: with walls {step_walls:.4f} ms, without {step_plain:.4f} ms, added {added:.4f} ms = "
          f"{rec['added_over_step']} of a step; one scalar_stats() {stats:.4f} ms: "
          f"{'below' if rec['added_below_one_scalar_stats'] else 'NOT below'} it", flush=True)

    # the second comparison: one sample on the device against the host route (once)
    t0 = time.perf_counter()
    qb, _ = e.scalar_body_flux()
    t1 = time.perf_counter()
    g = e.scalar(populations=True)[1]
    t2 = time.perf_counter()
    host = (lio.scalar_wall_flux if a.dim == 2 else lio.scalar_wall_flux3d)(g, obst, labels, kinds, values)[1][0]
    t3 = time.perf_counter()
    rec.update({"host_route_store_s": round(t2 - t1, 3), "host_route_numpy_s": round(t3 - t2, 3),
                "body_flux_over_host_route": (t1 - t0) / (t3 - t1),
                "largest_body_sum_difference": float(np.abs(qb - host).max())})
    print(f"scalar_body_flux() {1e3 * (t1 - t0):.3f} ms against the host route {t3 - t1:.2f} s (store {t2 - t1:.2f} s, "
          f"numpy {t3 - t2:.2f} s); largest difference of a body sum {rec['largest_body_sum_difference']:.3e}", flush=True)
    e.close()
    print(json.dumps(rec), flush=True)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"walls_bench_{a.dim}d_{grid.replace('^', 'p')}.json").write_text(json.dumps(rec, indent=1) + "\n")
    return 0 if ok else 1


def _more(ap):
    ap.add_argument("--advance", type=int, default=20, help="scalar steps of each timed scalar_advance")
    ap.add_argument("--bodies", type=int, default=400, help="small bodies beside the channel walls")
    ap.add_argument("--out", default=str(diag_bench.ROOT / "profiles" / "walls"), help="where the record goes")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, _more))
