"""Lagrangian tracers and point probes on the device, D2Q9 (lbm_tracer_*;
include/lbm_tracers_hip.h, csrc/lbm_tracers.hip, csrc/lbm_tracers.hpp).

Bar: after every advance the positions are BITWISE (uint64 patterns)
lio.tracer_advance of the same handle's fields() at the moment of the call, the
blocked flags lio.tracer_blocked, and tracer_sample lio.tracer_interp of those
fields -- the numpy restatement of the header's definition, pinned by exact
arithmetic in tests/test_tracers_host.py -- for both schemes, every step kernel,
both lattice layouts, both sides of the ping-pong pair, and decomposed handles,
whose positions equal the single-domain handle's.  No tolerance anywhere.
"""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG
from lbm_amd import io as lio
from tracer_util import N, SENTINEL64, _b64, _same, seeds

pytestmark = pytest.mark.gpu

ALL = ("ux", "uy", "pressure")
CHUNKS = (3, 1, 4, 2, 5)      # odd and even: both lattices of the pair get read
GRIDS = [(37, 19), (64, 32)]
SCHEMES = ["euler", "heun"]


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _problem(nx, ny, seed, iters=8):
    """About 10 % random obstacles on a 5 % perturbed equilibrium."""
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    obst[0, 0] = obst[ny - 1, nx - 1] = 1            # the corner cells the edge seeds touch
    obst[ny // 2, nx // 2] = 0
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    return p, obst, cells


def _border_seeds(x, y, nx, ny, k0=100):
    """Overwrites some random seeds with points on and next to the borders of the (1, 2) and (2, 2)
    decompositions (x = nx / 2, y = ny / 2), close enough for a step's displacement to cross."""
    k = k0
    for off in (0.0, -1.0, -0.5, -1e-3, -1e-9, 1e-9, 1e-3, 0.5, -0.02, 0.02, -0.1, 0.1):
        x[k], k = nx // 2 + off, k + 1
        y[k], k = ny // 2 + off, k + 1
        x[k], y[k], k = nx // 2 + off, ny // 2 - off, k + 1
    return x, y


def _seeds(p, seed=5):
    x, y = seeds(np.random.default_rng(seed), (p.nx, p.ny))
    return _border_seeds(x, y, p.nx, p.ny)


def _advance_and_check(e, obst, x, y, n, scheme, first, what=""):
    """One chunk of n steps, then one advance: the handle against the restatement of its fields()."""
    if n:
        e.run_steps(n, accelerate_first=first)
    f = e.fields(ALL)
    x, y = lio.tracer_advance(f["ux"], f["uy"], x, y, float(n), scheme)
    e.tracers_advance(n, scheme)
    t = e.tracers()
    assert tuple(t) == ("x", "y", "blocked") and t["x"].dtype == np.float64 and t["blocked"].dtype == np.uint8
    for c, want in (("x", x), ("y", y)):
        bad = _b64(t[c]) != _b64(want)
        assert not bad.any(), (what, n, c, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(t["blocked"], lio.tracer_blocked(obst, x, y)), (what, n)
    s = e.tracer_sample()
    assert tuple(s) == ALL
    for name in ALL:
        bad = _b64(s[name]) != _b64(lio.tracer_interp(f[name], x, y))
        assert not bad.any(), (what, n, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return x, y


def _sequence(e, p, obst, cells0, scheme, what="", chunks=CHUNKS):
    e.load_cells(cells0)
    x, y = _seeds(p)
    e.tracers_begin(x, y)
    assert e.tracer_count == N
    for i, n in enumerate(chunks):
        x, y = _advance_and_check(e, obst, x, y, n, scheme, i == 0, what)
    assert (x >= 0).all() and (x < p.nx).all() and (y >= 0).all() and (y < p.ny).all()
    return x, y


# ------------------------------------------------------ 1. cell centres ----

@pytest.mark.parametrize("nx,ny", GRIDS)
def test_sample_at_cell_centres_is_fields(gpu_lib, nx, ny):
    p, obst, cells0 = _problem(nx, ny, 10 * nx + ny)
    yy, xx = np.mgrid[0:ny, 0:nx]
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.tracers_begin(xx.ravel().astype(np.float64), yy.ravel().astype(np.float64))
        for steps in (0, 3, 4):
            if steps:
                e.run_steps(steps, accelerate_first=steps == 3)
            f, s = e.fields(ALL), e.tracer_sample()
            for name in ALL:
                assert _same(s[name], f[name].astype(np.float64).ravel()), (name, steps)
            t = e.tracers()
            assert np.array_equal(t["blocked"], obst.ravel()) and _same(t["x"], xx.ravel()) and _same(t["y"], yy.ravel())
    ob = obst.ravel() != 0
    assert ob.any() and not _b64(s["ux"])[ob].any() and not _b64(s["uy"])[ob].any()
    third = np.float32(p.density) * np.float32(np.float32(1) / np.float32(3))
    assert (_b64(s["pressure"])[ob] == _b64(np.float64(third))).all()


# ------------------------------------------------- 2. advance sequences ----

@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_advance_sequences_bitwise(gpu_lib, nx, ny, scheme):
    p, obst, cells0 = _problem(nx, ny, 100 * nx + ny)
    x0, y0 = _seeds(p)
    with gpu_lib.Engine(p, obst) as e:
        x, y = _sequence(e, p, obst, cells0, scheme, (nx, ny, scheme))
    assert (np.abs(x - x0) > 1e-3).sum() > N // 2          # the points moved


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_advance_every_kernel_bitwise(gpu_lib, mode, scheme):
    n = gpu_lib
    kw, want = {
        "auto": (dict(), ("resident", "step2")),
        "stream": (dict(kernel=n.KERNEL_STREAM), ("stream",)),
        "stream_tolerance": (dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE), ("stream",)),
        "step2": (dict(kernel=n.KERNEL_STEP2), ("step2",)),
        "scalar": (dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP), ("scalar",)),
        "pipeline": (dict(kernel=n.KERNEL_PIPELINE), ("pipeline",)),
    }[mode]
    p, obst, cells0 = _problem(132, 70, 7)
    with n.Engine(p, obst, **kw) as e:
        _sequence(e, p, obst, cells0, scheme, (mode, scheme))
        assert e.kernel_in_use() in want
        if mode == "stream_tolerance":
            assert e.numerics() == "tolerance"


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_advance_planar_layout_bitwise(gpu_lib, debug_knobs, monkeypatch, kernel, scheme):
    """The planar lattice layout (LBM_LAYOUT=planar, a debug knob)."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    p, obst, cells0 = _problem(37, 19, 13)
    with n.Engine(p, obst, **kw) as e:
        _sequence(e, p, obst, cells0, scheme, ("planar", kernel, scheme))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------------ 3. decomposed ----

@pytest.fixture(scope="module")
def single_64x32(gpu_lib):
    """(p, obst, cells0, {scheme: (x, y)}) of the single-domain handle after the sequence: the
    reference of the decomposed cases, computed once and left unchanged."""
    p, obst, cells0 = _problem(64, 32, 31)
    out = {}
    for scheme in SCHEMES:
        with gpu_lib.Engine(p, obst, parts=1) as e:
            out[scheme] = _sequence(e, p, obst, cells0, scheme, "single")
            assert len(e.local_rects()) == 1
    # a Heun midpoint of the first advance lies in another sub-domain than its point, in x and in y
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(CHUNKS[0], accelerate_first=True)
        f = e.fields(("ux", "uy"))
    x, y = _seeds(p)
    dt = float(CHUNKS[0])
    mx = lio.tracer_wrap(x + dt * lio.tracer_interp(f["ux"], x, y), p.nx)
    my = lio.tracer_wrap(y + dt * lio.tracer_interp(f["uy"], x, y), p.ny)
    assert ((x < 32) != (mx < 32)).any() and ((y < 16) != (my < 16)).any()
    for a in (cells0, obst) + out["euler"] + out["heun"]:
        a.setflags(write=False)
    return p, obst, cells0, out


def _decomposed_kw(native, how):
    if how == "local4":
        return dict(parts=4, grid=(2, 2), devices=[0])
    if how == "local2":
        return dict(parts=2, grid=(1, 2), devices=[0])
    return dict(parts=1, grid=(1, 1), devices=[0], flags=native.FLAG_FORCE_EXCHANGE,
                transport=native.TRANSPORT_RCCL, rank=0, world=1, unique_id=native.rccl_unique_id())


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("how", ["local4", "local2", "rccl1"])
def test_positions_do_not_depend_on_the_decomposition(gpu_lib, single_64x32, how, scheme):
    p, obst, cells0, ref = single_64x32
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        rects = e.local_rects()
        assert len(rects) == {"local4": 4, "local2": 2, "rccl1": 1}[how]
        if how != "rccl1":
            assert any(r[0] == 32 for r in rects)          # the border the seeds sit on
        x, y = _sequence(e, p, obst, cells0, scheme, (how, scheme))
    assert _same(x, ref[scheme][0]) and _same(y, ref[scheme][1])


# -------------------------------------------- 4. no engine state touched ----

def test_tracers_touch_no_engine_state(gpu_lib):
    p, obst, cells0 = _problem(64, 32, 21, iters=13)
    x, y = _seeds(p)
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.tracers_begin(x, y)
        e.run_steps(7, accelerate_first=True)
        av7 = e.store(cells=False, n_av=7)[1].copy()
        e.tracers_advance(7, "heun")
        e.tracer_sample()
        e.tracers()
        e.run_steps(6)
        cells_a, av6 = e.store(n_av=6)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        cells, av = e.store(n_av=13)
    assert np.array_equal(_b32(cells_a), _b32(cells)) and np.array_equal(_b32(np.concatenate([av7, av6])), _b32(av))


# --------------------------------------- 5. run_traced / probe_history ----

def test_run_traced_and_probe_history(gpu_lib):
    p, obst, cells0 = _problem(64, 32, 3, iters=13)
    x0, y0 = _seeds(p)
    with gpu_lib.Engine(p, obst) as e:                      # by hand: the reference of both
        e.load_cells(cells0)
        x, y = x0, y0
        fields = []
        for i, n in enumerate((5, 5, 3)):
            e.run_steps(n, accelerate_first=i == 0)
            fields.append(e.fields(ALL))
            x, y = lio.tracer_advance(fields[-1]["ux"], fields[-1]["uy"], x, y, float(n), "heun")
        cells, _ = e.store(n_av=0)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        _, av = e.store(n_av=13)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.tracers_begin(x0, y0)
        dts, advance = [], e.tracers_advance
        e.tracers_advance = lambda dt, scheme="heun": (dts.append(dt), advance(dt, scheme))[1]
        got_av = e.run_traced(13, 5, accelerate_first=True)
        assert dts == [5, 5, 3]
        t = e.tracers()
        got_cells, _ = e.store(n_av=0)
        with pytest.raises(ValueError):
            e.run_traced(5, 0)
        with pytest.raises(ValueError):
            e.tracers_advance(1, "rk4")
    assert _same(t["x"], x) and _same(t["y"], y)
    assert got_av.dtype == np.float32 and np.array_equal(_b32(got_av), _b32(av))
    assert np.array_equal(_b32(got_cells), _b32(cells))
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.tracers_begin(x0, y0)
        hist = e.probe_history(13, 5, which=("uy", "pressure"), accelerate_first=True)
        t = e.tracers()
    assert _same(t["x"], x0) and _same(t["y"], y0)          # probes are never advanced
    assert hist["step"].tolist() == [5, 10, 13] and tuple(hist) == ("uy", "pressure", "step")
    for name in ("uy", "pressure"):
        assert hist[name].shape == (3, N) and hist[name].dtype == np.float64
        for k in range(3):
            assert _same(hist[name][k], lio.tracer_interp(fields[k][name], x0, y0)), (name, k)


# ---------------------------------------------------------- 6. contract ----

def test_tracer_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells = _problem(37, 19, 9)
    x, y = _seeds(p)
    f64p, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    ptr = lambda a: a.ctypes.data_as(f64p)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        L, h = e._L, e._h
        out = [np.full(N, SENTINEL64, np.uint64).view(np.float64) for _ in range(3)]
        flag = np.full(N, 0xAB, np.uint8)
        untouched = lambda: all((_b64(a) == SENTINEL64).all() for a in out) and (flag == 0xAB).all()
        cnt = ctypes.c_int64(-1)
        # before begin
        assert L.lbm_tracer_count(h, ctypes.byref(cnt)) == n.LBM_OK and cnt.value == 0
        assert L.lbm_tracer_count(h, None) == n.LBM_E_INVALID
        assert L.lbm_tracer_advance(h, 1.0, n.TRACER_HEUN) == n.LBM_E_STATE
        assert L.lbm_tracer_sample(h, ptr(out[0]), ptr(out[1]), ptr(out[2])) == n.LBM_E_STATE
        assert L.lbm_tracer_store(h, ptr(out[0]), ptr(out[1]), flag.ctypes.data_as(u8p)) == n.LBM_E_STATE
        assert L.lbm_tracer_end(h) == n.LBM_OK
        # refused seeds start nothing
        for bad in (float(p.nx), -1e-9, np.nan, np.inf, -np.inf):
            xb = x.copy()
            xb[N - 1] = bad
            assert L.lbm_tracer_begin(h, N, ptr(xb), ptr(y)) == n.LBM_E_INVALID, bad
        yb = y.copy()
        yb[0] = float(p.ny)
        assert L.lbm_tracer_begin(h, N, ptr(x), ptr(yb)) == n.LBM_E_INVALID
        assert L.lbm_tracer_begin(h, 0, ptr(x), ptr(y)) == n.LBM_E_INVALID
        assert L.lbm_tracer_begin(h, N, None, ptr(y)) == n.LBM_E_INVALID
        assert e.tracer_count == 0 and L.lbm_tracer_store(h, ptr(out[0]), None, None) == n.LBM_E_STATE
        # begun, no lattice yet: store works, advance and sample do not
        e.tracers_begin(x, y)
        assert e.tracer_count == N
        assert L.lbm_tracer_advance(h, 1.0, n.TRACER_EULER) == n.LBM_E_STATE
        assert L.lbm_tracer_sample(h, ptr(out[0]), None, None) == n.LBM_E_STATE
        assert untouched()
        t = e.tracers()
        assert _same(t["x"], x) and _same(t["y"], y) and np.array_equal(t["blocked"], lio.tracer_blocked(obst, x, y))
        e.load_cells(cells)
        e.run_steps(3, accelerate_first=True)
        # bad dt / scheme
        for dt, scheme in ((np.nan, 0), (np.inf, 1), (-np.inf, 1), (1.0, 2), (1.0, -1)):
            assert L.lbm_tracer_advance(h, dt, scheme) == n.LBM_E_INVALID, (dt, scheme)
        assert _same(e.tracers()["x"], x)
        # all NULL: no launch
        launches = lambda: sum(k["launches"] for k in e.profile_summary())
        before = launches()
        assert L.lbm_tracer_sample(h, None, None, None) == n.LBM_OK and launches() == before
        # selection: only the arrays given are written
        f = e.fields(ALL)
        assert L.lbm_tracer_sample(h, None, ptr(out[1]), None) == n.LBM_OK
        assert _same(out[1], lio.tracer_interp(f["uy"], x, y))
        _b64(out[1])[...] = SENTINEL64
        assert untouched()
        assert L.lbm_tracer_store(h, None, ptr(out[1]), None) == n.LBM_OK and _same(out[1], y)
        _b64(out[1])[...] = SENTINEL64
        with pytest.raises(ValueError):
            e.tracer_sample(("speed",))
        # profile classes
        e.tracers_advance(3, "heun")
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["advance_tracers"]["launches"] == 1 and prof["sample_tracers"]["launches"] == 1
        assert prof["advance_tracers"]["total_ms"] > 0
        # a rejected begin keeps the previous set
        moved = e.tracers()
        assert not _same(moved["x"], x)
        xb = x.copy()
        xb[3] = np.nan
        assert L.lbm_tracer_begin(h, N, ptr(xb), ptr(y)) == n.LBM_E_INVALID
        kept = e.tracers()
        assert e.tracer_count == N and _same(kept["x"], moved["x"]) and _same(kept["y"], moved["y"])
        # begin twice replaces the set
        e.tracers_begin(x[:7], y[:7])
        assert e.tracer_count == 7 and _same(e.tracers()["x"], x[:7])
        s = e.tracer_sample(("ux",))
        assert tuple(s) == ("ux",) and _same(s["ux"], lio.tracer_interp(f["ux"], x[:7], y[:7]))
        # end, then count
        e.tracers_end()
        assert e.tracer_count == 0 and L.lbm_tracer_end(h) == n.LBM_OK
        assert L.lbm_tracer_advance(h, 1.0, 0) == n.LBM_E_STATE
        e.tracers_begin(x, y)          # the handle is destroyed with a set: lbm_destroy frees it
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:       # a handle that never begins launches nothing
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        assert not [k for k in e.profile_summary() if "tracers" in k["name"]]


# ------------------------------------------------------------ 7. runner ----

@pytest.mark.parametrize("scheme", SCHEMES)
def test_runner_tracers_gpu_writes_the_cpu_bytes(gpu_lib, tmp_path, scheme):
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "23"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    x, y = seeds(np.random.default_rng(2), (128, 128), n=257)
    (tmp_path / "seeds.txt").write_text("".join(f"{a!r} {b!r}\n" for a, b in zip(x.tolist(), y.tolist())))
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file), "--tracers",
            str(tmp_path / "seeds.txt"), "--trace-every", "5", "--trace-scheme", scheme]
    for device in ("gpu", "cpu"):
        d = tmp_path / device
        d.mkdir()
        r = subprocess.run(base + ["--device", device, "--out-dir", str(d)], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
    got = (tmp_path / "gpu" / "tracers.dat").read_bytes()
    assert got == (tmp_path / "cpu" / "tracers.dat").read_bytes() and len(got.splitlines()) == 257
    gx, gy, _ = lio.read_tracers(str(tmp_path / "gpu" / "tracers.dat"))
    # 23 steps from rest: the flow has reached the rows next to the accelerated one only
    assert (gx != x).sum() > 16 and (gx >= 0).all() and (gx < 128).all()
