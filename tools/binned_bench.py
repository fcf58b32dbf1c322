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

import json
import statistics
import sys

import diag_bench

READ_BYTES = {2: 37.0, 3: 77.0}      # populations and the obstacle byte per cell
PASS, FOLD, STATS = "binned_sums", "binned_sums fold", "macroscopic_fields stats"


def worker(a) -> int:
    e, run, cells, grid, _ = diag_bench.engine(a)
    n = e.params.nx
    if a.dim == 2:
        shapes = {"profile": (n, 1), "sections": (1, n), "coarse16": (16, 16), "total": (n, n)}
    else:
        shapes = {"profile": (n, 1, n), "sections": (1, n, n), "coarse16": (16, 16, 16), "total": (n, n, n)}
    print(f"binned_bench: {grid}, {a.steps} steps, {a.rounds} rounds", flush=True)

    calls = [(f"binned {k}", (lambda b: lambda: e.binned(*b))(b)) for k, b in shapes.items()]
    calls += [("coarse_fields(16)", lambda: e.coarse_fields(16)), ("field_stats", e.field_stats), ("fields", e.fields)]

    def line(r, name, dt, ms):
        return (f"  round {r} {name:20s} wall {dt * 1e3:10.3f} ms   " +
                "  ".join(f"{c} {v:.3f} ms" for c, v in (ms or {}).items()))

    got = diag_bench.rounds(a.rounds, diag_bench.each(e, calls, lambda name: (PASS, FOLD, STATS)), line)
    plain, hist = diag_bench.history_cost(run, lambda: e.binned_history(100, 10, *shapes["profile"]), 2)
    e.close()
    med_wall = {k: diag_bench.median_wall(v) for k, v in got.items()}
    med_dev = {k: {c: statistics.median(ms[c] for _, ms in v) for c in (v[0][1] or {})} for k, v in got.items()}
    rec = {
        "tool": "binned_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med_wall.items()},
        "device_ms": {k: {c: round(v, 4) for c, v in d.items()} for k, d in med_dev.items() if d},
        "read_bytes_per_cell": READ_BYTES[a.dim],
        "run_ms": {"run_steps_100": round(plain * 1e3, 3), "binned_history_100_every_10_profile": round(hist * 1e3, 3)},
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


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__))
