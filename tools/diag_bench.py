"""Shared mechanics of the diagnostic benches beside this file (avg, binned, fields, fields3d,
force, gradients, stress, tracer): the --dim engine set-up, the timed call, the interleaved
rounds, the run_steps-against-history cost loop and the main() that re-runs the bench as a
--worker child under `timeout`.  What a bench measures, prints and gates stays in its own file."""
from __future__ import annotations

import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "lbm-graphcore_amd")]


def engine(a):
    """The engine of --dim / --n, equilibrium initialised on the device and a.steps steps run.
    --dim 2: n x n (default 8192) with the sparse synthetic obstacle set and FLAG_PROFILE;
    --dim 3: the n^3 (default 256) channel on devices=[0].
    Returns (engine, run(k), cells, grid label, obstacles)."""
    from lbm_amd import io as lio
    from lbm_amd import native

    if a.dim == 2:
        from bench import synthetic_obstacles
        n = a.n or 8192
        cells, grid = n * n, f"{n}x{n}"
        obst = synthetic_obstacles(n, n)
        e = native.Engine(lio.Params(n, n, a.steps, 10, 0.1, 0.005, 1.85), obst, flags=native.FLAG_PROFILE)
        run = lambda k: e.run_steps(k, accelerate_first=False)   # noqa: E731
    else:
        n = a.n or 256
        cells, grid = n ** 3, f"{n}^3"
        obst = lio.channel_obstacles3d(n, n, n)
        e = native.Engine3D(lio.Params3D(n, n, n, a.steps, 0.1, 0.001, 1.85), obst, devices=[0])
        run = e.run_steps
    e.init_equilibrium()
    run(a.steps)
    return e, run, cells, grid, obst


def timed(e, call, classes=()):
    """(wall seconds of call(), {class: device ms} of those of `classes` that profile_summary() lists).
    The D3Q19 engine has no profile classes: None in place of the dict."""
    profiled = hasattr(e, "profile_reset")
    if profiled:
        e.profile_reset()
    t0 = time.perf_counter()
    out = call()
    dt = time.perf_counter() - t0
    del out
    if not profiled:
        return dt, None
    return dt, {k["name"]: k["total_ms"] for k in e.profile_summary() if k["name"] in classes}


def rounds(n, measure, line):
    """n + 1 interleaved rounds; round 0 warms up and is discarded.  measure() yields (name, wall s,
    device ms) per call of one round -- timed()'s pair behind the name; line(r, name, dt, ms) is the
    text printed for it.  Returns {name: [(dt, ms), ...]} of rounds 1..n."""
    kept = {}
    for r in range(n + 1):
        for name, dt, ms in measure():
            if r > 0:
                kept.setdefault(name, []).append((dt, ms))
            print(line(r, name, dt, ms), flush=True)
    return kept


def each(e, calls, classes_of):
    """A measure() for rounds(): timed() of every (name, call), with the profile classes classes_of(name)."""
    def measure():
        for name, call in calls:
            yield (name, *timed(e, call, classes_of(name)))
    return measure


def median_wall(samples):
    return statistics.median(dt for dt, _ in samples)


def median_device(samples, cls):
    """Median device ms of profile class `cls` (0 where a call launched none); without profile
    classes the blocking call's wall time stands in."""
    return statistics.median(dt * 1e3 if ms is None else ms.get(cls, 0.0) for dt, ms in samples)


def history_cost(run, history, n, steps=100):
    """(median seconds of run(steps), of history()) over n interleaved rounds behind a warm-up one."""
    plain, hist = [], []
    for r in range(n + 1):
        t0 = time.perf_counter()
        run(steps)
        t1 = time.perf_counter()
        history()
        t2 = time.perf_counter()
        if r:
            plain.append(t1 - t0)
            hist.append(t2 - t1)
    return statistics.median(plain), statistics.median(hist)


def main(worker, file, more=None, *, dim=True, n=0, steps=20, limit=600) -> int:
    """Parse the common arguments (and those more(parser) adds) and run worker(args) in a child
    process under `timeout -k 10 <limit>`, every parsed argument forwarded, so a hang ends it."""
    ap = argparse.ArgumentParser()
    if dim:
        ap.add_argument("--dim", type=int, default=2, choices=(2, 3))
        ap.add_argument("--n", type=int, default=n, help="edge length (default 8192 for --dim 2, 256 for --dim 3)")
    else:
        ap.add_argument("--n", type=int, default=n)
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--rounds", type=int, default=5)
    if more:
        more(ap)
    ap.add_argument("--limit", type=int, default=limit, help="seconds the measuring child may take")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rounds < 1:
        ap.error("--rounds must be >= 1")
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, str(Path(file).resolve()), "--worker"]
    for k, v in vars(a).items():
        if k not in ("limit", "worker") and v != "":        # "": an optional choice left open
            cmd += [f"--{k}", str(v)]
    return subprocess.run(cmd).returncode
