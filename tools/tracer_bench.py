#!/usr/bin/env python3
"""What does moving or sampling a point set cost?  tracers_advance() / tracer_sample() vs fields() + numpy.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, 20 steps) and for uniformly
random point sets of n = 1e5, 1e6 and 1e7 points, these calls are timed,
interleaved round by round (round 0 warms up, medians of the rest):

  (a) tracers_advance(1, "heun")   one advance_tracers launch, nothing to the host
  (b) tracer_sample()              one sample_tracers launch, 8 B per point and field to the host
  (c) fields(ux, uy[, uz])         what the library offered before: the velocity fields to the host ...
  (d) ... + lio.tracer_advance     ... and the same Heun advance in numpy there

Host wall time is taken around each call.  The device time of (a) and (b) is the
`advance_tracers` / `sample_tracers` launch class of profile_summary() (D2Q9; the
D3Q19 engine has no profile classes, so there the blocking call's wall time stands
in: launch and synchronise included).  From the medians the tool also reports the
device time per point and the point count at which a Heun advance costs as much
as one fields() call (linear interpolation between the measured counts; "beyond
the measured counts" when even the largest is cheaper).

Exit status 1 unless a 1e6-point Heun advance takes less host wall time than the
fields() call alone on that handle: the cost a particle loop paid before any
particle arithmetic.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/tracer_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--points 100000,1000000,10000000]
                               [--limit 600]
"""
from __future__ import annotations

import json
import statistics
import sys

import diag_bench

# bytes a point reads per interpolation (4 / 8 cells of Q populations and a map byte) and per call
CELL_BYTES = {2: 4 * 37.0, 3: 8 * 77.0}
POS_BYTES = {2: 16.0, 3: 24.0}
CLASSES = {"advance_heun": "advance_tracers", "sample": "sample_tracers"}


def worker(a) -> int:
    import numpy as np

    from lbm_amd import io as lio

    e, run, _, grid, _ = diag_bench.engine(a)
    extent = (e.params.nx,) * a.dim
    vel = ("ux", "uy") if a.dim == 2 else ("ux", "uy", "uz")
    advance_np = lio.tracer_advance if a.dim == 2 else lio.tracer_advance3d
    counts = [int(c) for c in a.points.split(",")]
    print(f"tracer_bench: {grid}, {a.steps} steps, {a.rounds} rounds, points {counts}", flush=True)

    rng = np.random.default_rng(1)
    rec = {"tool": "tracer_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
           "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking call",
           "bytes_per_point": {"advance_heun": 2 * CELL_BYTES[a.dim] + 2 * POS_BYTES[a.dim],
                               "sample": CELL_BYTES[a.dim] + POS_BYTES[a.dim] + 8.0 * (a.dim + 1)},
           "points": {}}
    for npts in counts:
        pos = [rng.random(npts) * ext for ext in extent]
        e.tracers_begin(*pos)

        def fields_numpy():
            f = e.fields(vel)
            return advance_np(*[f[k] for k in vel], *pos, 1.0, "heun")

        calls = (("advance_heun", lambda: e.tracers_advance(1, "heun")), ("sample", e.tracer_sample),
                 ("fields", lambda: e.fields(vel)), ("fields_numpy_heun", fields_numpy))

        def line(r, name, dt, ms):
            return (f"  n {npts:9d} round {r} {name:18s} wall {dt * 1e3:10.3f} ms" +
                    ("" if ms is None or name not in CLASSES else f"   device {ms.get(CLASSES[name], 0.0):9.4f} ms"))

        got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: (CLASSES.get(name),)), line)
        e.tracers_end()
        w = {k: diag_bench.median_wall(v) * 1e3 for k, v in got.items()}
        d = {k: diag_bench.median_device(got[k], c) for k, c in CLASSES.items()}
        rec["points"][str(npts)] = {
            "wall_ms": {k: round(v, 3) for k, v in w.items()},
            "device_ms": {k: round(v, 4) for k, v in d.items()},
            "device_ns_per_point": {k: round(v * 1e6 / npts, 3) for k, v in d.items()},
            "device_gbs": {k: round(rec["bytes_per_point"][k] * npts / (v * 1e-3) / 1e9, 1) for k, v in d.items()},
        }
        print(f"n {npts}: median wall ms (a) advance heun {w['advance_heun']:.3f}  (b) sample {w['sample']:.3f}  "
              f"(c) fields() {w['fields']:.3f}  (d) fields() + numpy heun {w['fields_numpy_heun']:.3f};  device ms "
              f"(a) {d['advance_heun']:.4f}  (b) {d['sample']:.4f}", flush=True)
    e.close()
    # the point count at which a Heun advance costs one fields() call (host wall clock)
    pts = sorted(int(k) for k in rec["points"])
    adv = [rec["points"][str(k)]["wall_ms"]["advance_heun"] for k in pts]
    fld = statistics.median(rec["points"][str(k)]["wall_ms"]["fields"] for k in pts)
    even = None
    if adv[0] >= fld:
        even = f"below {pts[0]}"
    for (n0, t0), (n1, t1) in zip(zip(pts, adv), zip(pts[1:], adv[1:])):
        if even is None and t0 < fld <= t1:
            even = int(n0 + (fld - t0) * (n1 - n0) / (t1 - t0))
    rec["fields_wall_ms"] = round(fld, 3)
    rec["break_even_points"] = even if even is not None else f"beyond the measured counts (> {pts[-1]})"
    key = "1000000" if "1000000" in rec["points"] else str(pts[len(pts) // 2])
    m = rec["points"][key]["wall_ms"]
    rec["gate_points"] = int(key)
    rec["advance_faster_than_fields"] = m["advance_heun"] < m["fields"]
    print(f"fields() {fld:.3f} ms; a Heun advance costs as much at: {rec['break_even_points']} points")
    print(json.dumps(rec), flush=True)
    return 0 if rec["advance_faster_than_fields"] else 1


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__,
                             lambda ap: ap.add_argument("--points", default="100000,1000000,10000000")))
