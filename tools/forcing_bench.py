#!/usr/bin/env python3
"""What does a forcing zone cost?  forcing_apply() against the buoyancy kick, and a strip against the whole domain.

On one engine (default 8192^2 with the sparse synthetic obstacle set, or --dim 3:
256^3 channel; equilibrium initialised on the device, 20 steps) these calls are
timed, interleaved round by round (round 0 warms up, medians of the rest), each k
times per timed call:

  uniform, uniform+impulse   a whole-domain zone with constant coefficients (kernel arguments)
  fields, fields+impulse     the same zone with five (seven) coefficient planes
  strip                      the uniform zone on a tenth of the domain's rows (planes): the cost is O(zone)
  cell                       a one-cell zone: one launch and its synchronisation
  empty                      no zone set: the call returns before it launches
  yardstick                  scalar_buoyancy() of a scalar begun at zero on the same handle

The device time is the launch class per launch (D2Q9: `forcing` and `scalar_buoyancy`
of profile_summary()) or the wall time of the blocking calls (D3Q19, which has no
profile classes; it holds the call's own synchronisation and the ghost-plane refresh
behind it).  Rates are on the bytes a kernel must move per cell: the uniform form
69 B in 2-D (36 read, 32 written, 1 obstacle byte) and 149 B in 3-D, the fields form
20 B and 28 B more; the buoyancy kick 85 B and 173 B (tools/thermal_bench.py).

Two bars, reported and never enforced (the tool exits 0 when the measurement itself
succeeded): the uniform form without the impulse should reach the yardstick's rate
less the max - min spread the yardstick shows over the rounds; the strip should cost
no more than a tenth of the whole-domain time plus the time of `empty`.

The measurement runs in a child process under `timeout`, so a hang ends it:

  python tools/forcing_bench.py [--dim 2|3] [--n N] [--steps 20] [--rounds 5] [--k 10] [--limit 600]
"""
from __future__ import annotations

import json
import sys

import numpy as np

import diag_bench

UNIFORM_BYTES = {2: 69.0, 3: 149.0}
FIELDS_BYTES = {2: 89.0, 3: 177.0}
KICK_BYTES = {2: 85.0, 3: 173.0}
LAM, TARGET, FORCE = 0.01, 0.01, 1e-6


def worker(a) -> int:
    e, run, cells, grid, _ = diag_bench.engine(a)
    n = a.n or (8192 if a.dim == 2 else 256)
    print(f"forcing_bench: {grid}, {a.steps} steps, {a.rounds} rounds, {a.k} applications per timed call", flush=True)
    e.scalar_begin(None, omega_s=1.3)
    dims = a.dim
    whole, origin = (n,) * dims, (0,) * dims
    strip = (n,) * (dims - 1) + (n // 10,)
    target, force = [TARGET] + [0.0] * (dims - 1), [FORCE] + [0.0] * (dims - 1)
    lam_field = np.full(whole, LAM, np.float32)

    current = [None]

    def zone(kind):
        if kind == current[0]:
            return
        current[0] = kind
        e.forcing_clear()
        if kind == "uniform":
            e.forcing_zone(0, origin, whole, LAM, target, force)
        elif kind == "fields":
            e.forcing_zone(0, origin, whole, lam_field, target, force)
        elif kind == "strip":
            e.forcing_zone(0, origin, strip, LAM, target, force)
        elif kind == "cell":
            e.forcing_zone(0, origin, (1,) * dims, LAM, target, force)

    def applies(impulse):
        def call():
            for _ in range(a.k):
                e.forcing_apply(1.0, impulse=impulse)
        return call

    def kicks():
        s = [0.0] * (dims - 1) + [1e-6]
        for i in range(a.k):
            e.scalar_buoyancy([c if i % 2 == 0 else -c for c in s], 0.5)

    calls = (("uniform", applies(False)), ("uniform+impulse", applies(True)), ("fields", applies(False)),
             ("fields+impulse", applies(True)), ("strip", applies(False)), ("cell", applies(False)),
             ("empty", applies(False)), ("yardstick", kicks))
    cls = lambda name: ("scalar_buoyancy",) if name == "yardstick" else ("forcing",)       # noqa: E731

    def line(r, name, dt, ms):
        return f"  round {r} {name:16s} wall {dt * 1e3:10.3f} ms" + ("" if ms is None else f"   device {ms}")

    def measure():
        for name, call in calls:
            zone(name.split("+")[0])                     # the zone is set outside the timed call
            yield (name, *diag_bench.timed(e, call, cls(name)))

    got = diag_bench.rounds(a.rounds, measure, line)

    def per_call(name):
        """ms per application: device time where the engine has profile classes, else wall time."""
        c = cls(name)[0]
        if a.dim == 2 and name != "empty":
            return diag_bench.median_device(got[name], c) / a.k
        return diag_bench.median_wall(got[name]) * 1e3 / a.k

    ms = {name: per_call(name) for name, _ in calls}
    tbs = lambda bytes_per_cell, t, share=1.0: bytes_per_cell * cells * share / (t * 1e-3) / 1e12      # noqa: E731
    yard = [(dt * 1e3 if m is None else m.get("scalar_buoyancy", 0.0)) / a.k for dt, m in got["yardstick"]]
    yard_tbs = sorted(tbs(KICK_BYTES[dims], t) for t in yard)
    spread = yard_tbs[-1] - yard_tbs[0]
    rate = {"uniform": tbs(UNIFORM_BYTES[dims], ms["uniform"]), "uniform+impulse": tbs(UNIFORM_BYTES[dims], ms["uniform+impulse"]),
            "fields": tbs(FIELDS_BYTES[dims], ms["fields"]), "fields+impulse": tbs(FIELDS_BYTES[dims], ms["fields+impulse"]),
            "strip": tbs(UNIFORM_BYTES[dims], ms["strip"], (n // 10) / n), "yardstick": tbs(KICK_BYTES[dims], ms["yardstick"])}
    strip_bar = 0.1 * ms["uniform"] + ms["empty"]
    rec = {"tool": "forcing_bench", "grid": grid, "steps": a.steps, "rounds": a.rounds, "k": a.k,
           "device_time_source": "profile_summary" if a.dim == 2 else "wall time of the blocking calls",
           "ms": {k: round(v, 5) for k, v in ms.items()}, "tbs": {k: round(v, 3) for k, v in rate.items()},
           "wall_ms": {name: round(diag_bench.median_wall(got[name]) * 1e3 / a.k, 5) for name, _ in calls},
           "bytes_per_cell": {"uniform": UNIFORM_BYTES[dims], "fields": FIELDS_BYTES[dims], "yardstick": KICK_BYTES[dims]},
           "yardstick_spread_tbs": round(spread, 3),
           "uniform_meets_yardstick": rate["uniform"] >= rate["yardstick"] - spread,
           "strip_bar_ms": round(strip_bar, 5), "strip_meets_bar": ms["strip"] <= strip_bar}
    e.close()
    print("; ".join(f"{k} {ms[k]:.4f} ms" + (f" = {rate[k]:.3f} TB/s" if k in rate else "") for k, _ in calls))
    print(f"uniform {rate['uniform']:.3f} TB/s against the yardstick's {rate['yardstick']:.3f} TB/s (spread {spread:.3f}): "
          f"{'meets' if rec['uniform_meets_yardstick'] else 'short of'} it; strip {ms['strip']:.4f} ms against "
          f"{strip_bar:.4f} ms: {'meets' if rec['strip_meets_bar'] else 'short of'} it")
    print(json.dumps(rec), flush=True)
    return 0


def _more(ap):
    ap.add_argument("--k", type=int, default=10, help="applications per timed call")


if __name__ == "__main__":
    sys.exit(diag_bench.main(worker, __file__, _more))
