#!/usr/bin/env python3
"""What does a sample of the time averages cost?  avg_sample() vs fields() + numpy on ONE handle.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, a few steps) these calls
are timed, interleaved round by round (round 0 warms up, medians of the rest):

  (a) avg_sample(), MEAN           one accumulate_moments launch, nothing to the host
  (b) avg_sample(), MEAN|SECOND    the same with the products
  (c) fields(ux, uy[, uz], p)      what the library offered before: the fields to the host ...
  (d) ... + numpy                  ... and lio.moment_sums-style fp64 accumulation of all moments there

Host wall time is taken around each call.  The device time of (a) and (b) is the
`accumulate_moments` launch class of profile_summary() (D2Q9; the D3Q19 engine has
no profile classes, so there the blocking call's wall time stands in: launch and
synchronise included).  It is also printed as achieved bytes/s on the kernel's
bytes per cell and sample (D2Q9 85 / 149 B, D3Q19 141 / 253 B), next to a device
copy timed live in this process (torch, 1 GiB, read + write; where torch sees no
device, the float4-copy rate fields_bench.py records, 6.29 TB/s), and the cost of
run_averaged(100, every=10) over run_steps(100) is reported.

Exit status 1 unless (b) is faster on the host clock than (c) alone: (b) moves no
byte to the host, so anything else is a bug.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/avg_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--limit 600]
"""
from __future__ import annotations

import json
import statistics
import sys

import diag_bench

BYTES = {2: (85.0, 149.0), 3: (141.0, 253.0)}   # per cell and sample: MEAN, MEAN|SECOND
RECORDED_COPY_TBS = 6.29   # float4 device copy, MI355X (tools/fields_bench.py)
CLASS = "accumulate_moments"


def copy_rate_tbs():
    """Device-to-device copy of 1 GiB (read + write counted), median of 5 after a warm-up; None without torch."""
    try:
        import torch
        if not torch.cuda.is_available():
            print("avg_bench: torch sees no device, no live copy rate", flush=True)
            return None
        n = 1 << 28
        src, dst = torch.zeros(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.float32, device="cuda")
        ms = []
        for r in range(6):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            dst.copy_(src)
            b.record()
            torch.cuda.synchronize()
            if r:
                ms.append(a.elapsed_time(b))
        del src, dst
        torch.cuda.empty_cache()
        return 2.0 * 4.0 * n / (statistics.median(ms) * 1e-3) / 1e12
    except Exception as exc:   # the copy rate is context only
        print(f"avg_bench: no live copy rate ({exc})", flush=True)
        return None


def worker(a) -> int:
    import numpy as np

    e, run, cells, grid, _ = diag_bench.engine(a)
    first = ("ux", "uy", "pressure") if a.dim == 2 else ("ux", "uy", "uz", "pressure")
    nv = len(first) - 1
    pairs = [(i, j) for i in range(nv) for j in range(i, nv)] + [(nv, nv)]
    copy_tbs = copy_rate_tbs()
    copy_source = "measured live" if copy_tbs is not None else "recorded, not measured in this run"
    copy_tbs = RECORDED_COPY_TBS if copy_tbs is None else copy_tbs
    print(f"avg_bench: {grid}, {a.steps} steps, {a.rounds} rounds, device copy {copy_tbs:.2f} TB/s ({copy_source})",
          flush=True)

    host_sums = [np.zeros(e._shape(), np.float64) for _ in range(len(first) + len(pairs))]

    def fields_numpy():
        f = e.fields(first)
        s = [f[k].astype(np.float64) for k in first]
        for k in range(len(first)):
            host_sums[k] += s[k]
        for k, (i, j) in enumerate(pairs):
            host_sums[len(first) + k] += s[i] * s[j]

    names = ("sample_mean", "sample_mean_second", "fields", "fields_numpy")

    def measure():
        for name, second in (("sample_mean", False), ("sample_mean_second", True)):
            e.avg_begin(second=second)   # allocation and zeroing stay outside the timed call
            e.avg_sample()               # first touch of the fresh accumulators
            yield (name, *diag_bench.timed(e, e.avg_sample, (CLASS,)))
        yield ("fields", *diag_bench.timed(e, lambda: e.fields(first)))
        yield ("fields_numpy", *diag_bench.timed(e, fields_numpy))

    def line(r, name, dt, ms):
        return (f"  round {r} {name:20s} wall {dt * 1e3:10.3f} ms" +
                ("" if ms is None or name not in names[:2] else f"   accumulate_moments {ms.get(CLASS, 0.0):8.3f} ms"))

    got = diag_bench.rounds(a.rounds, measure, line)
    # the sampled run against the plain one (the accumulators of MEAN|SECOND are still allocated)
    plain, hist = diag_bench.history_cost(run, lambda: e.run_averaged(100, 10), 3)
    e.avg_end()
    e.close()
    med_wall = {k: diag_bench.median_wall(got[k]) for k in names}
    med_dev = {k: diag_bench.median_device(got[k], CLASS) for k in names[:2]}
    tbs = {k: BYTES[a.dim][i] * cells / (med_dev[k] * 1e-3) / 1e12 for i, k in enumerate(names[:2])}
    rec = {
        "tool": "avg_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds,
        "wall_ms": {k: round(v * 1e3, 3) for k, v in med_wall.items()},
        "accumulate_moments_ms": {k: round(v, 4) for k, v in med_dev.items()},
        "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking call",
        "bytes_per_cell": dict(zip(names[:2], BYTES[a.dim])),
        "accumulate_moments_tbs": {k: round(v, 3) for k, v in tbs.items()},
        "device_copy_tbs": round(copy_tbs, 3), "device_copy_source": copy_source,
        "run_ms": {"run_steps_100": round(plain * 1e3, 3), "run_averaged_100_every_10": round(hist * 1e3, 3)},
        "sample_faster_than_fields": med_wall["sample_mean_second"] < med_wall["fields"],
    }
    w = rec["wall_ms"]
    print(f"median wall ms: (a) sample MEAN {w['sample_mean']}  (b) sample MEAN|SECOND {w['sample_mean_second']}  "
          f"(c) fields() {w['fields']}  (d) fields() + numpy {w['fields_numpy']}")
    print(f"accumulate_moments ms ({rec['device_time_source']}): (a) {rec['accumulate_moments_ms']['sample_mean']} = "
          f"{rec['accumulate_moments_tbs']['sample_mean']} TB/s on {BYTES[a.dim][0]:.0f} B per cell; (b) "
          f"{rec['accumulate_moments_ms']['sample_mean_second']} = {rec['accumulate_moments_tbs']['sample_mean_second']}"
          f" TB/s on {BYTES[a.dim][1]:.0f} B per cell (device copy, {copy_source}: {rec['device_copy_tbs']} TB/s)")
    print(f"run_steps(100) {rec['run_ms']['run_steps_100']} ms; run_averaged(100, every=10) "
          f"{rec['run_ms']['run_averaged_100_every_10']} ms")
    print(json.dumps(rec), flush=True)
    return 0 if rec["sample_faster_than_fields"] else 1


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__))
