#!/usr/bin/env python3
"""What do the binned sums cost on the device?  binned() of four bin shapes vs field_stats() and fields() on ONE handle.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, a few steps) these calls
are timed, interleaved round by round (round 0 warms up -- it also fetches the
fluid counts of each bin shape, which are kept -- medians of the rest):

  (a) binned(nx, 1[, nz])     the profile across the channel
  (b) binned(1, ny[, nz])     the sums over every cross-section
  (c) binned(16, 16[, 16])    a reduced-resolution picture
  (d) binned(nx, ny[, nz])    domain totals
  (e) coarse_fields(16)       the block means of the velocities (four / five of the fields of (c))
  (f) field_stats()           the yardstick: the per-cell stats pass over the same populations
  (g) fields()                every macroscopic field (4 / 5) to the host

Host wall time is taken around each call.  The device time of (a) - (f) is the
sum of their launch classes of profile_summary() (D2Q9: "binned_sums" and
"binned_sums fold", shown apart; "macroscopic_fields stats"; the D3Q19 engine
has no profile classes, so only wall times are reported there).  The ratios to
field_stats() are reported, not gated: the one condition is that
coarse_fields(16) is faster on the host clock than fields(), which moves 256
times the bytes.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/binned_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--limit 600]
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

READ_BYTES = {2: 37.0, 3: 77.0}      # populations and the obstacle byte per cell
PASS, FOLD, STATS = "binned_sums", "binned_sums fold", "macroscopic_fields stats"


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
        shapes = {"profile": (n, 1), "sections": (1, n), "coarse16": (16, 16), "total": (n, n)}
    else:
        n = a.n or 256
        cells, grid = n ** 3, f"{n}^3"
        p = lio.Params3D(n, n, n, a.steps, 0.1, 0.001, 1.85)
        e = native.Engine3D(p, lio.channel_obstacles3d(n, n, n), devices=[0])
        run = e.run_steps
        shapes = {"profile": (n, 1, n), "sections": (1, n, n), "coarse16": (16, 16, 16), "total": (n, n, n)}
    e.init_equilibrium()
    run(a.steps)
    print(f"binned_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)

    def device_ms():
        if a.dim != 2:
            return {}
        return {k["name"]: k["total_ms"] for k in e.profile_summary() if k["name"] in (PASS, FOLD, STATS)}

    def timed(call):
        if a.dim == 2:
            e.profile_reset()
        t0 = time.perf_counter()
        out = call()
        dt = time.perf_counter() - t0
        del out
        return dt, device_ms()

    calls = [(f"binned {k}", (lambda b: lambda: e.binned(*b))(b)) for k, b in shapes.items()]
    calls += [("coarse_fields(16)", lambda: e.coarse_fields(16)), ("field_stats", e.field_stats), ("fields", e.fields)]
    wall = {k: [] for k, _ in calls}
    dev = {k: {} for k, _ in calls}
    for r in range(a.rounds + 1):
        for name, call in calls:
            dt, ms = timed(call)
            if r > 0:
                wall[name].append(dt)
                for cls, v in ms.items():
                    dev[name].setdefault(cls, []).append(v)
            print(f"  round {r} {name:20s} wall {dt * 1e3:10.3f} ms   " +
                  "  ".join(f"{c} {v:.3f} ms" for c, v in ms.items()), flush=True)
    cost = {"run_steps_100": [], "binned_history_100_every_10_profile": []}
    for r in range(3):
        t0 = time.perf_counter()
        run(100)
        t1 = time.perf_counter()
        e.binned_history(100, 10, *shapes["profile"])
        t2 = time.perf_counter()
        if r:
            cost["run_steps_100"].append(t1 - t0)
            cost["binned_history_100_every_10_profile"].append(t2 - t1)
    e.close()
    med_wall = {k: statistics.median(v) for k, v in wall.items()}
    med_dev = {k: {c: statistics.median(v) for c, v in d.items()} for k, d in dev.items()}
    rec = {
        "tool": "binned_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med_wall.items()},
        "device_ms": {k: {c: round(v, 4) for c, v in d.items()} for k, d in med_dev.items() if d},
        "read_bytes_per_cell": READ_BYTES[a.dim],
        "run_ms": {k: round(statistics.median(v) * 1e3, 3) for k, v in cost.items()},
        "coarse_faster_than_fields": med_wall["coarse_fields(16)"] < med_wall["fields"],
    }
    if a.dim == 2:
        stats = med_dev["field_stats"][STATS]
        rec["pass_over_field_stats"] = {k: round(d[PASS] / stats, 3) for k, d in med_dev.items() if PASS in d}
        rec["pass_tbs"] = {k: round(READ_BYTES[2] * cells / (d[PASS] * 1e-3) / 1e12, 3)
                           for k, d in med_dev.items() if PASS in d}
    print("median wall ms: " + "  ".join(f"{k} {v}" for k, v in rec["wall_ms"].items()))
    for k, d in rec["device_ms"].items():
        print(f"device ms  {k:20s} " + "  ".join(f"{c} {v}" for c, v in d.items()) +
              (f"   pass = {rec['pass_over_field_stats'][k]} x field_stats, {rec['pass_tbs'][k]} TB/s"
               if k in rec.get("pass_over_field_stats", {}) else ""))
    print(f"run_steps(100) {rec['run_ms']['run_steps_100']} ms; binned_history(100, every=10, profile) "
          f"{rec['run_ms']['binned_history_100_every_10_profile']} ms")
    print(json.dumps(rec), flush=True)
    return 0 if rec["coarse_faster_than_fields"] else 1


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
