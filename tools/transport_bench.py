#!/usr/bin/env python3
"""What do the scalar transport sums cost?  scalar_binned() against binned() of the same handle.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3: 256^3
channel; equilibrium initialised on the device, 20 steps) with a scalar begun at zero and
two fixed cells, these calls are timed at the bins (nx, ny[, nz]), (16, 16[, 16]) and
(nx, 1[, nz]), interleaved round by round (round 0 warms up, medians of the rest):

  (a) scalar_binned(*bins)                 every field: the form that reads the flow lattice
  (b) the yardstick: binned(*bins)         the flow's binned sums: the same geometry, fold and fp64
                                           sums, in the same process
  (c) scalar_binned(*bins, which=faces)    the no-flow form, the planes of the faces only
  (d) scalar_stats()                       a pure read of the same scalar planes (once, not per bins)

The device time is the first pass's launch class (D2Q9: `scalar_binned` against `binned_sums`
of profile_summary(); the folds are listed beside them) or the wall time of the blocking call
(D3Q19, which has no profile classes).  Rates are on the bytes a pass must move per cell: (a)
57 B in 2-D (36 flow, 1 obstacle, 20 scalar) and 105 B in 3-D (76, 1, 28); (b) 37 B and 77 B; (c)
16 B and 24 B (the two planes of every face, no rest plane, no map); (d) 21 B and 29 B.  Wanted: (a) reaches at least
0.75 of (b)'s TB/s at the bins (nx, ny) and (16, 16); (nx, 1) is reported without a ratio wanted
(the yardstick is scan-bound there).  The tool reports the ratios and whether they are met.

The hard condition, which decides the exit status (2-D): scalar_profile(1) takes at most a tenth
of the host wall time of scalar() plus fields(("ux", "uy")) plus the numpy reduction of phi, phi^2,
ux phi and uy phi per row, in the same process.

Last, transport_history(coupled, every=6, nx, 1[, nz], accel, stride=6) against run_thermal(coupled,
stride=6) alone, per step.

The measurement runs in a child process under `timeout`, so a hang ends it; the JSON record also
goes to --out (default profiles/transport/):

  python tools/transport_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--coupled 60] [--out DIR] [--limit 600]
"""
from __future__ import annotations

import json
import statistics
import sys
import time
from pathlib import Path

import diag_bench

FULL_BYTES = {2: 57.0, 3: 105.0}
YARD_BYTES = {2: 37.0, 3: 77.0}
FACE_BYTES = {2: 16.0, 3: 24.0}
STATS_BYTES = {2: 21.0, 3: 29.0}


def worker(a) -> int:
    import numpy as np

    e, run, cells, grid, obst = diag_bench.engine(a)
    shape = e._shape()
    extent = shape[::-1]                                             # x first
    print(f"transport_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)
    e.scalar_begin(None, omega_s=1.3)
    mid = [n // 2 for n in extent]
    lo = [np.array([c], np.int32) for c in mid[:-1]] + [np.array([1], np.int32)]
    hi = [np.array([c], np.int32) for c in mid[:-1]] + [np.array([extent[-1] - 2], np.int32)]
    e.scalar_fix(*[np.concatenate(p) for p in zip(lo, hi)], np.array([0.5, -0.5], np.float32))
    e.scalar_advance(2)
    faces = ("fx", "fy", "fz")[:a.dim]
    profile = tuple(1 if c == 1 else n for c, n in enumerate(extent))
    bins_list = [("full", extent), ("16", (16,) * a.dim), ("rows", profile)]
    calls, classes = [], {}
    for label, bins in bins_list:
        calls += [(f"transport {label}", lambda b=bins: e.scalar_binned(*b)),
                  (f"yardstick {label}", lambda b=bins: e.binned(*b)),
                  (f"faces {label}", lambda b=bins: e.scalar_binned(*b, which=faces))]
        classes[f"transport {label}"] = classes[f"faces {label}"] = ("scalar_binned", "scalar_binned fold")
        classes[f"yardstick {label}"] = ("binned_sums", "binned_sums fold")
    calls.append(("scalar_stats", e.scalar_stats))
    classes["scalar_stats"] = ("scalar_stats",)

    def line(r, name, dt, ms):
        return f"  round {r} {name:16s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}")

    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: classes[name]), line)

    def device_ms(name):
        """(first pass or whole blocking call, fold or None) in ms."""
        if a.dim == 2:
            return diag_bench.median_device(got[name], classes[name][0]), \
                (diag_bench.median_device(got[name], classes[name][1]) if len(classes[name]) > 1 else None)
        return diag_bench.median_wall(got[name]) * 1e3, None

    tbs = lambda bytes_per_cell, ms: bytes_per_cell * cells / (ms * 1e-3) / 1e12      # noqa: E731
    rec = {"tool": "transport_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
           "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking calls",
           "bytes_per_cell": {"transport": FULL_BYTES[a.dim], "yardstick": YARD_BYTES[a.dim],
                              "faces": FACE_BYTES[a.dim], "scalar_stats": STATS_BYTES[a.dim]},
           "bins": {}}
    stats_ms, _ = device_ms("scalar_stats")
    rec["scalar_stats_ms"] = round(stats_ms, 4)
    rec["scalar_stats_tbs"] = round(tbs(STATS_BYTES[a.dim], stats_ms), 3)
    for label, bins in bins_list:
        t_ms, t_fold = device_ms(f"transport {label}")
        y_ms, y_fold = device_ms(f"yardstick {label}")
        f_ms, f_fold = device_ms(f"faces {label}")
        t_tbs, y_tbs, f_tbs = tbs(FULL_BYTES[a.dim], t_ms), tbs(YARD_BYTES[a.dim], y_ms), tbs(FACE_BYTES[a.dim], f_ms)
        r = {"bins": list(bins), "transport_ms": round(t_ms, 4), "transport_tbs": round(t_tbs, 3),
             "yardstick_ms": round(y_ms, 4), "yardstick_tbs": round(y_tbs, 3), "ratio": round(t_tbs / y_tbs, 3),
             "faces_ms": round(f_ms, 4), "faces_tbs": round(f_tbs, 3),
             "faces_over_scalar_stats": round(f_tbs / rec["scalar_stats_tbs"], 3) if rec["scalar_stats_tbs"] else None,
             "fold_ms": {"transport": t_fold, "yardstick": y_fold, "faces": f_fold},
             "wall_ms": {k: round(diag_bench.median_wall(got[f"{k} {label}"]) * 1e3, 3)
                         for k in ("transport", "yardstick", "faces")}}
        if label != "rows":
            r["meets_0.75"] = t_tbs >= 0.75 * y_tbs
        rec["bins"][label] = r
        print(f"bins {tuple(bins)}: transport {t_ms:.4f} ms = {t_tbs:.3f} TB/s on {FULL_BYTES[a.dim]:.0f} B; yardstick "
              f"binned {y_ms:.4f} ms = {y_tbs:.3f} TB/s on {YARD_BYTES[a.dim]:.0f} B; ratio {r['ratio']}"
              + ("" if label == "rows" else f" ({'meets' if r['meets_0.75'] else 'short of'} 0.75)")
              + f"; faces only {f_ms:.4f} ms = {f_tbs:.3f} TB/s on {FACE_BYTES[a.dim]:.0f} B"
              f" (scalar_stats {stats_ms:.4f} ms = {rec['scalar_stats_tbs']} TB/s)", flush=True)

    # the hard condition: the profile on the device against the host route
    ok = True
    names = ("ux", "uy", "uz")[:a.dim]

    def host_route():
        phi = e.scalar().astype(np.float64)
        f = e.fields(names)
        fluid = obst.reshape(shape) == 0
        axes = tuple(i for i in range(a.dim) if i != a.dim - 2)       # every axis but y
        out = [np.where(fluid, phi, 0.0).sum(axis=axes), np.where(fluid, phi * phi, 0.0).sum(axis=axes)]
        out += [np.where(fluid, f[n] * phi, 0.0).sum(axis=axes) for n in names]
        return out

    dev_t, host_t = [], []
    for r in range(a.rounds + 1):
        t0 = time.perf_counter()
        e.scalar_profile(1)
        t1 = time.perf_counter()
        host_route()
        t2 = time.perf_counter()
        if r:
            dev_t.append(t1 - t0)
            host_t.append(t2 - t1)
    dev_ms, host_ms = statistics.median(dev_t) * 1e3, statistics.median(host_t) * 1e3
    rec["scalar_profile_wall_ms"], rec["host_route_wall_ms"] = round(dev_ms, 3), round(host_ms, 3)
    rec["profile_over_host"] = round(dev_ms / host_ms, 4)
    if a.dim == 2:
        ok = dev_ms <= 0.1 * host_ms
        rec["meets_a_tenth_of_the_host_route"] = ok
    print(f"scalar_profile(1) {dev_ms:.3f} ms against the host route (scalar() + fields() + numpy) {host_ms:.3f} ms: "
          f"{rec['profile_over_host']}" + (f" ({'meets' if ok else 'MISSES'} a tenth)" if a.dim == 2 else ""), flush=True)

    # the monitored coupled run against the coupled run alone
    accel = [0.0] * (a.dim - 1) + [1e-9]

    def per_step(call):
        t = []
        for r in range(a.rounds + 1):
            t0 = time.perf_counter()
            call()
            if r:
                t.append((time.perf_counter() - t0) / a.coupled * 1e3)
        return statistics.median(t)

    alone = per_step(lambda: e.run_thermal(a.coupled, accel, 0.0, 6))
    watched = per_step(lambda: e.transport_history(a.coupled, 6, *profile, accel=accel, stride=6))
    faces_only = per_step(lambda: e.transport_history(a.coupled, 6, *profile, which=faces[1:2], accel=accel, stride=6))
    rec.update({"coupled_steps": a.coupled, "run_thermal_ms_per_step": round(alone, 4),
                "transport_history_ms_per_step": round(watched, 4),
                "transport_history_fy_only_ms_per_step": round(faces_only, 4)})
    print(f"per step over {a.coupled} at stride 6: run_thermal {alone:.4f} ms; transport_history every 6, bins "
          f"{profile}: {watched:.4f} ms (fy only: {faces_only:.4f} ms)")
    e.close()
    print(json.dumps(rec), flush=True)
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    (out / f"transport_bench_{a.dim}d_{grid.replace('^', 'p')}.json").write_text(json.dumps(rec, indent=1) + "\n")
    return 0 if ok else 1


def _more(ap):
    ap.add_argument("--coupled", type=int, default=60, help="steps of each timed coupled run")
    ap.add_argument("--out", default=str(diag_bench.ROOT / "profiles" / "transport"), help="where the record goes")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, _more))
