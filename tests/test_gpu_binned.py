"""Binned sums on the device, D2Q9 (lbm_store_binned / lbm_bin_fluid_cells;
include/lbm_binned_hip.h, csrc/lbm_binned.hip).

Bar: the reference is lio.binned_sums of the same handle's store() cells -- the
numpy restatement of the header's definition (math.fsum per bin: the exactly
rounded sum), pinned by arithmetic in tests/test_binned_host.py.  One-cell bins
are BITWISE (uint64 patterns); every other bin lies within
2 (n - 1) 2^-53 sum|term| of the reference, n its fluid cells (any order of n
fp64 additions, plus the rounding of the exact sum); the counts are exact;
all-obstacle bins hold +0.0; a repeat call returns identical bits.  The grids
and bins sit around the kernel's work units: a lane's quad of 4 cells, a wave's
256 columns, a chunk of at most 32 rows inside one bin.
"""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

SENTINEL64 = 0x7FF8000000000001     # a quiet NaN pattern no computation produces
QUAD, WAVE, CHUNK = 4, 256, 32      # native.BIN_QUAD / BIN_WAVE_COLS / BIN_CHUNK_ROWS (asserted below)
OMEGA, DENSITY = 1.85, 0.1
# (9, 2100): 66 chunks of 32 rows in the whole-domain bin -- the second pass takes its wave-per-bin form from 64
GRIDS = [(301, 37), (96, 80), (1, 9), (9, 1), (9, 2100)]


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bins(nx, ny):
    """The issue's bin shapes, clipped to the grid, each once."""
    raw = [(1, 1), (nx, 1), (1, ny), (nx, ny), (4, 4), (16, 16), (3, 5), (7, 2), (nx - 1, ny - 1), (5, ny)]
    out = []
    for bw, bh in raw:
        b = (min(max(bw, 1), nx), min(max(bh, 1), ny))
        if b not in out:
            out.append(b)
    return out


def _obstacles(nx, ny, seed):
    """About 10 % random obstacles; blocked cells on both sides of every border of a bin (of
    every shape of _bins), a quad, a wave and a chunk, in staggered rows / columns so that
    fluid cells remain beside them; the block [16, 32) x [16, 32) blocked where the grid
    holds it (an all-obstacle bin for every small bin shape); one cell kept fluid."""
    rng = np.random.default_rng(seed)
    obst = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    xs = {WAVE} | set(range(QUAD, nx, 64)) | {b for bw, _ in _bins(nx, ny) for b in (bw, 2 * bw, nx // bw * bw)}
    ys = {CHUNK, 2 * CHUNK} | {b for _, bh in _bins(nx, ny) for b in (bh, 2 * bh, ny // bh * bh)}
    for i, x in enumerate(sorted(x for x in xs if 0 < x < nx)):
        obst[(3 * i) % ny, x - 1] = obst[(3 * i + 1) % ny, x] = 1
    for i, y in enumerate(sorted(y for y in ys if 0 < y < ny)):
        obst[y - 1, (5 * i) % nx] = obst[y, (5 * i + 2) % nx] = 1
    if nx >= 32 and ny >= 32:
        obst[16:32, 16:32] = 1
    else:
        obst[ny // 2, nx // 2] = 1
    obst[min(ny - 1, 2), min(nx - 1, 2)] = 0
    return obst


def _problem(nx, ny, seed, iters=8):
    p = lio.Params(nx, ny, iters, 10, DENSITY, 0.005, OMEGA)
    rng = np.random.default_rng(seed + 1)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    return p, _obstacles(nx, ny, seed), cells


def _terms(e, p, obst):
    cells, _ = e.store(n_av=0)
    return lio.binned_terms(p, obst, np.asarray(cells).reshape(p.ny, p.nx, 9))


def _assert_binned(got, terms, obst, bins, names, what=""):
    """got against the exactly rounded sums of `terms` over `bins`."""
    fluid = lio.bin_reduce((np.asarray(obst) == 0).astype(np.int64), bins, exact=False)
    assert got["fluid"].dtype == np.int64 and np.array_equal(got["fluid"], fluid), (what, bins)
    n = fluid.astype(np.float64)
    for name in names:
        ref = lio.bin_reduce(terms[name], bins)
        assert got[name].dtype == np.float64 and got[name].shape == ref.shape, (what, bins, name)
        if all(b == 1 for b in bins):
            bad = _b64(got[name]) != _b64(ref)
            assert not bad.any(), (what, bins, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            continue
        bound = 2 * np.maximum(n - 1, 0) * 2.0 ** -53 * lio.bin_reduce(np.abs(terms[name]), bins)
        err = np.abs(got[name] - ref)
        assert (err <= bound).all(), (what, bins, name, np.argwhere(err > bound)[:4].tolist(),
                                      float(err.max()), float(bound.max()))
        assert not _b64(got[name])[fluid == 0].any(), (what, bins, name)      # all-obstacle bins: +0.0


def _check(e, p, obst, shapes, what=""):
    terms = _terms(e, p, obst)
    out = {}
    for bins in shapes:
        got = e.binned(*bins)
        assert tuple(got) == e._BIN_FIELDS + ("fluid",)
        _assert_binned(got, terms, obst, bins, e._BIN_FIELDS, what)
        again = e.binned(*bins)
        for name in e._BIN_FIELDS:
            assert np.array_equal(_b64(got[name]), _b64(again[name])), (what, bins, name)
        out[bins] = got
    return out


# ------------------------------------------------------------ 1. shapes ----

@pytest.mark.parametrize("nx,ny", GRIDS)
def test_binned_grids_and_bins(gpu_lib, nx, ny):
    assert (gpu_lib.BIN_QUAD, gpu_lib.BIN_WAVE_COLS, gpu_lib.BIN_CHUNK_ROWS) == (QUAD, WAVE, CHUNK)
    p, obst, cells = _problem(nx, ny, 100 * nx + ny)
    shapes = _bins(nx, ny)
    empty = lio.bin_reduce((obst == 0).astype(np.int64), (1, 1), exact=False) == 0
    assert empty.any()
    if nx >= 32 and ny >= 32:      # an all-obstacle bin of more than one cell
        assert (lio.bin_reduce((obst == 0).astype(np.int64), (4, 4), exact=False) == 0).any()
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        _check(e, p, obst, shapes[:5], (nx, ny, "loaded"))
        e.run_steps(3, accelerate_first=True)      # an odd ...
        got = _check(e, p, obst, shapes, (nx, ny, 3))
        e.run_steps(1)                             # ... and an even number of steps: both sides of the pair
        _check(e, p, obst, shapes[:4], (nx, ny, 4))
        one = e.binned(nx, 1, which=("jx",))
        assert tuple(one) == ("jx", "fluid")
        assert np.array_equal(_b64(one["jx"]), _b64(e.binned(nx, 1)["jx"]))
        with pytest.raises(ValueError):
            e.binned(1, 1, which=("pressure",))
    whole = got[(nx, ny)]
    assert whole["rho"][0, 0] > 0 and whole["speed"][0, 0] > 0 and whole["jx"][0, 0] != 0


def test_binned_conveniences(gpu_lib):
    nx, ny = 96, 80
    p, obst, cells = _problem(nx, ny, 17)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        prof, flux, coarse = e.profile_y(), e.flux_x(), e.coarse_fields(16)
        rows, cols, blocks = e.binned(nx, 1), e.binned(1, ny), e.binned(16, 16)
    assert tuple(prof) == gpu_lib.BIN_FIELDS and all(a.shape == (ny,) for a in prof.values())
    means = lio.binned_means(rows)
    for name in gpu_lib.BIN_FIELDS:
        assert np.array_equal(_b64(prof[name]), _b64(means[name].reshape(-1))), name
    assert flux.shape == (nx,) and np.array_equal(_b64(flux), _b64(cols["jx"].reshape(-1)))
    assert tuple(coarse) == ("ux", "uy", "speed")
    means = lio.binned_means(blocks)
    for name in coarse:
        assert coarse[name].shape == (5, 6) and np.array_equal(_b64(coarse[name]), _b64(means[name])), name
    assert coarse["speed"][1, 1] == 0 and blocks["fluid"][1, 1] == 0 and coarse["speed"].max() > 0


# ----------------------------------------------- 2. every step kernel ----

@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_binned_every_kernel(gpu_lib, mode):
    n = gpu_lib
    kw, want = {
        "auto": (dict(), ("resident", "step2")),
        "stream": (dict(kernel=n.KERNEL_STREAM), ("stream",)),
        "stream_tolerance": (dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE), ("stream",)),
        "step2": (dict(kernel=n.KERNEL_STEP2), ("step2",)),
        "scalar": (dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP), ("scalar",)),
        "pipeline": (dict(kernel=n.KERNEL_PIPELINE), ("pipeline",)),
    }[mode]
    nx, ny = 96, 80
    p, obst, cells0 = _problem(nx, ny, 7)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        for i, steps in enumerate((3, 1, 4, 5)):       # odd and even launch counts, remainders included
            e.run_steps(steps, accelerate_first=i == 0)
            _check(e, p, obst, [(1, 1), (nx, 1), (7, 2), (16, 16)], (mode, steps))
        assert e.kernel_in_use() in want


@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_binned_planar_layout(gpu_lib, debug_knobs, monkeypatch, kernel):
    """The planar lattice layout (LBM_LAYOUT=planar, a debug knob)."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    nx, ny = 301, 37
    p, obst, cells0 = _problem(nx, ny, 13)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        e.run_steps(3, accelerate_first=True)
        _check(e, p, obst, [(1, 1), (3, 5), (nx, ny)], ("planar", 3))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------------ 3. decomposed ----

def _decomposed_kw(native, how):
    if how == "local4":
        return dict(parts=4, grid=(2, 2), devices=[0])
    if how == "local6":
        return dict(parts=6, grid=(3, 2), devices=[0])      # rows of 27, 27, 26; columns of 48
    return dict(parts=1, grid=(1, 1), devices=[0], flags=native.FLAG_FORCE_EXCHANGE,
                transport=native.TRANSPORT_RCCL, rank=0, world=1, unique_id=native.rccl_unique_id())


@pytest.mark.parametrize("how", ["local4", "local6", "rccl1"])
def test_binned_decomposed(gpu_lib, how):
    """96 x 80 on several sub-domains of one device: the bins of every shape but (1, 1),
    (4, 4) and (16, 16) straddle the sub-domain borders, and their partial sums are added on
    the host."""
    nx, ny = 96, 80
    p, obst, cells0 = _problem(nx, ny, 31)
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        rects = e.local_rects()
        assert len(rects) == {"local4": 4, "local6": 6, "rccl1": 1}[how]
        if how != "rccl1":
            xb = {x0 for (x0, _, _, _) in rects if x0} | {y0 for (_, y0, _, _) in rects if y0}
            assert any(b % 7 for b in xb) and any(b % 5 for b in xb)     # borders inside bins
        _check(e, p, obst, _bins(nx, ny), how)


# -------------------------------------------- 4. no engine state touched ----

@pytest.mark.parametrize("how", ["single", "local4"])
def test_binned_touches_no_engine_state(gpu_lib, how):
    """7 steps, binned() of three shapes, 6 steps: the lattice and av_vels equal those of
    the same 7 + 6 run without the calls."""
    p, obst, cells0 = _problem(96, 80, 21, iters=13)
    kw = {} if how == "single" else _decomposed_kw(gpu_lib, how)

    def chunked(with_calls):
        with gpu_lib.Engine(p, obst, **kw) as e:
            e.load_cells(cells0)
            e.run_steps(7, accelerate_first=True)
            av7 = e.store(cells=False, n_av=7)[1].copy()
            if with_calls:
                e.binned(96, 1)
                e.binned(7, 2)
                e.binned(1, 1, which=("speed",))
            e.run_steps(6)
            got_cells, av6 = e.store(n_av=6)
            return got_cells, np.concatenate([av7, av6])

    got_cells, got_av = chunked(True)
    plain_cells, plain_av = chunked(False)
    assert np.array_equal(_b32(got_cells), _b32(plain_cells)) and np.array_equal(_b32(got_av), _b32(plain_av))


# ---------------------------------------------------------- 5. contract ----

def _ptrs(n, arrays):
    out = (ctypes.POINTER(ctypes.c_double) * n)()
    for i, a in arrays.items():
        out[i] = a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    return out


def test_binned_contract(gpu_lib):
    n = gpu_lib
    nx, ny = 96, 80
    p, obst, cells = _problem(nx, ny, 9)
    nf = len(n.BIN_FIELDS)
    classes = ("binned_sums", "binned_sums fold")
    i64p = ctypes.POINTER(ctypes.c_int64)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        L, h = e._L, e._h
        out = {i: np.full((ny, nx), SENTINEL64, np.uint64).view(np.float64) for i in range(nf)}
        untouched = lambda idx: all((_b64(out[i]) == SENTINEL64).all() for i in idx)
        # before load
        assert L.lbm_store_binned(h, 1, 1, _ptrs(nf, out)) == n.LBM_E_STATE
        assert untouched(range(nf))
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.fields()
        # bin sizes outside 1..n
        count = np.full((ny, nx), -7, np.int64)
        for bw, bh in ((0, 1), (1, 0), (nx + 1, 1), (1, ny + 1), (-1, 1)):
            assert L.lbm_store_binned(h, bw, bh, _ptrs(nf, out)) == n.LBM_E_INVALID, (bw, bh)
            assert L.lbm_bin_fluid_cells(h, bw, bh, count.ctypes.data_as(i64p)) == n.LBM_E_INVALID, (bw, bh)
        assert untouched(range(nf)) and (count == -7).all()
        with pytest.raises(n.LbmError):
            e.binned(nx + 1, 1)
        # every entry NULL: LBM_OK and no launch
        assert L.lbm_store_binned(h, 4, 4, _ptrs(nf, {})) == n.LBM_OK
        assert L.lbm_store_binned(h, 4, 4, None) == n.LBM_OK
        assert L.lbm_bin_fluid_cells(h, 4, 4, None) == n.LBM_OK
        names = [k["name"] for k in e.profile_summary()]
        assert names and not [k for k in names if k in classes]
        # a selection writes only the entries given
        terms = _terms(e, p, obst)
        assert L.lbm_store_binned(h, 1, 1, _ptrs(nf, {1: out[1], 5: out[5]})) == n.LBM_OK
        assert np.array_equal(_b64(out[1]), _b64(terms["jx"])) and np.array_equal(_b64(out[5]), _b64(terms["speed"]))
        assert untouched((0, 2, 3, 4, 6, 7, 8))
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["binned_sums"]["launches"] == 1 and prof["binned_sums"]["total_ms"] > 0
        assert prof["binned_sums fold"]["launches"] == 1
        assert L.lbm_bin_fluid_cells(h, 1, 1, count.ctypes.data_as(i64p)) == n.LBM_OK
        assert np.array_equal(count, (obst == 0).astype(np.int64))


def test_binned_history(gpu_lib):
    nx, ny = 96, 80
    p, obst, cells0 = _problem(nx, ny, 3, iters=20)
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        hist = e.binned_history(20, 5, nx, 1)
        with pytest.raises(ValueError):
            e.binned_history(5, 0, nx, 1)
    assert hist["step"].tolist() == [5, 10, 15, 20] and hist["ux"].shape == (4, ny, 1)
    with gpu_lib.Engine(p, obst) as e:      # the same sums taken by hand at those steps
        e.load_cells(cells0)
        for i in range(4):
            e.run_steps(5)
            got = e.binned(nx, 1)
            for name in gpu_lib.BIN_FIELDS:
                assert np.array_equal(_b64(hist[name][i]), _b64(got[name])), (i, name)
            assert np.array_equal(hist["fluid"], got["fluid"])
    assert hist["speed"][-1].max() > 0


# ------------------------------------------------------------ 6. runner ----

def test_runner_binned(gpu_lib, tmp_path):
    """lbm_runner --binned 16x16 on the GPU against the host backend's file of the same
    run.  Each side lies within 2 (n - 1) 2^-53 sum|term| of the exact sum and within half
    a unit of the thirteenth digit of %.12E (5e-13 |value|) of its own value: the files
    differ by at most twice their sum."""
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "50"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    got = {}
    for dev in ("gpu", "cpu"):
        out = tmp_path / dev
        out.mkdir()
        r = subprocess.run([str(exe), "--device", dev, "--runs", "0", "--binned", "16x16", "--params", str(params),
                            "--obstacles", str(obst_file), "--out-dir", str(out)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
        got[dev] = lio.read_binned_state(str(out / "binned_state.dat"), 8, 8)
    assert (tmp_path / "gpu" / "final_state.dat").read_bytes() == (tmp_path / "cpu" / "final_state.dat").read_bytes()
    p = lio.Params.from_file(str(params))
    obst = np.asarray(lio.read_obstacles(p.nx, p.ny, str(obst_file))).reshape(p.ny, p.nx)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(lio.init_cells(p))
        e.run_steps(50, accelerate_first=True)
        terms = _terms(e, p, obst)
    assert np.array_equal(got["gpu"]["fluid"], got["cpu"]["fluid"])
    assert np.array_equal(got["gpu"]["fluid"], lio.bin_reduce((obst == 0).astype(np.int64), (16, 16), exact=False))
    n = got["cpu"]["fluid"].astype(np.float64)
    for name in gpu_lib.BIN_FIELDS:
        mag = lio.bin_reduce(np.abs(terms[name]), (16, 16))
        bound = 2 * (2 * np.maximum(n - 1, 0) * 2.0 ** -53 * mag + 5e-13 * mag)
        err = np.abs(got["gpu"][name] - got["cpu"][name])
        assert (err <= bound).all(), (name, float(err.max()), float(bound.max()))
    assert np.abs(got["gpu"]["jx"]).max() > 0
