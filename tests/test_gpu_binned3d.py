"""Binned sums on the device, D3Q19 (lbm3d_store_binned / lbm3d_bin_fluid_cells;
include/lbm_binned_hip.h, csrc/lbm3d_binned.hip).

Bar as in tests/test_gpu_binned.py: the reference is lio.binned_sums3d of the
same handle's store() cells; one-cell bins are BITWISE, every other bin lies
within 2 (n - 1) 2^-53 sum|term| of the exactly rounded sum, the counts are
exact, all-obstacle bins hold +0.0 and a repeat call returns identical bits.
70 x 9 x 11 is wider than a wave's 64 columns; 4 x 18 x 4 is narrower than
every bin but the smallest.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

OMEGA, DENSITY = 1.85, 0.1
WAVE3 = 64                      # native.BIN3D_WAVE_COLS (asserted below)
SENTINEL64 = 0x7FF8000000000001
# (5, 67, 3): 67 rows in the whole-domain bin -- the second pass takes its wave-per-bin form from 64 (chunk, row) pairs
GRIDS = [(70, 9, 11), (4, 18, 4), (5, 67, 3)]


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bins(nx, ny, nz):
    raw = [(1, 1, 1), (nx, 1, nz), (1, ny, nz), (nx, ny, nz), (4, 4, 4), (3, 2, 5)]
    out = []
    for b in raw:
        b = tuple(min(v, n) for v, n in zip(b, (nx, ny, nz)))
        if b not in out:
            out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed):
    """About 10 % random obstacles; blocked cells on both sides of the wave border and of the
    first borders of every bin shape along each axis; the box [0, 4)^3 blocked (an
    all-obstacle bin of (4, 4, 4) and (1, 1, 1)); populations perturbed by 5 %."""
    p = lio.Params3D(nx, ny, nz, 0, DENSITY, 0.002, OMEGA)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < 0.1).astype(np.uint8)
    for i, x in enumerate(sorted({WAVE3, 3, 4, 6, 8} & set(range(1, nx)))):
        obst[i % nz, (2 * i) % ny, x - 1] = obst[(i + 1) % nz, (2 * i + 1) % ny, x] = 1
    for i, y in enumerate(sorted({2, 4, 8} & set(range(1, ny)))):
        obst[i % nz, y - 1, (3 * i) % nx] = obst[(i + 1) % nz, y, (3 * i + 1) % nx] = 1
    for i, z in enumerate(sorted({4, 5, 8, 10} & set(range(1, nz)))):
        obst[z - 1, i % ny, (3 * i) % nx] = obst[z, (i + 1) % ny, (3 * i + 1) % nx] = 1
    obst[:4, :4, :4] = 1
    obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _terms(e, p, obst):
    cells, _ = e.store()
    return lio.binned_terms3d(p, obst, np.asarray(cells).reshape(p.nz, p.ny, p.nx, 19))


def _assert_binned(got, terms, obst, bins, names, what=""):
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
        assert not _b64(got[name])[fluid == 0].any(), (what, bins, name)


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


@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_binned3d_grids_and_bins(gpu_lib, nx, ny, nz):
    assert gpu_lib.BIN3D_WAVE_COLS == WAVE3
    p, obst, c0 = _problem(nx, ny, nz, nx + ny + nz)
    shapes = _bins(nx, ny, nz)
    assert (lio.bin_reduce((obst == 0).astype(np.int64), (4, 4, 4), exact=False) == 0).any()
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        _check(e, p, obst, shapes[:3], (nx, ny, nz, "loaded"))
        e.run_steps(3)                 # an odd ...
        got = _check(e, p, obst, shapes, (nx, ny, nz, 3))
        e.run_steps(1)                 # ... and an even number of steps
        _check(e, p, obst, shapes[:4], (nx, ny, nz, 4))
        with pytest.raises(ValueError):
            e.binned(1, 1, 1, which=("pressure",))
        with pytest.raises(ValueError):
            e.binned(1, 1)
    whole = got[(nx, ny, nz)]
    assert whole["rho"][0, 0, 0] > 0 and whole["speed"][0, 0, 0] > 0 and whole["uzuz"][0, 0, 0] > 0


@pytest.mark.parametrize("form", ["three", "two", "one", "tolerance"])
def test_binned3d_every_step_form(gpu_lib, debug_knobs, monkeypatch, form):
    env = {"three": {}, "two": {"LBM3D_THREE": "0"}, "one": {"LBM3D_TWO": "0"}, "tolerance": {}}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    p, obst, c0 = _problem(70, 9, 11, 7)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        for steps in (3, 1, 4):
            e.run_steps(steps)
            _check(e, p, obst, [(1, 1, 1), (70, 1, 11), (3, 2, 5)], (form, steps))


def test_binned3d_slabs(gpu_lib):
    """Three z slabs of 70 x 9 x 11 (4 + 4 + 3 planes): bd = 5, 4 and nz straddle or meet the
    slab borders, and the slabs' partial sums are added on the host."""
    nx, ny, nz = 70, 9, 11
    p, obst, c0 = _problem(nx, ny, nz, 41)
    with gpu_lib.Engine3D(p, obst, parts=3, devices=[0]) as e:
        slabs = e.local_slabs()
        assert len(slabs) == 3 and any(z0 % 5 for z0, _ in slabs if z0)
        e.load_cells(c0)
        e.run_steps(5)
        _check(e, p, obst, _bins(nx, ny, nz), "slabs")


def test_binned3d_rccl_world_1(gpu_lib):
    n = gpu_lib
    nx, ny, nz = 70, 9, 11
    p, obst, c0 = _problem(nx, ny, nz, 43)
    with n.Engine3D(p, obst, devices=[0], transport=n.TRANSPORT_RCCL, rank=0, world=1,
                    unique_id=n.rccl_unique_id()) as e:
        e.load_cells(c0)
        e.run_steps(5)
        _check(e, p, obst, [(1, 1, 1), (nx, 1, nz), (3, 2, 5)], "rccl1")


def test_binned3d_conveniences_and_history(gpu_lib):
    nx, ny, nz = 70, 9, 11
    p, obst, c0 = _problem(nx, ny, nz, 45)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        hist = e.binned_history(6, 2, nx, 1, nz, which=("ux", "uxuy"))
        prof, flux, coarse = e.profile_y(("ux",)), e.flux_x(), e.coarse_fields(4)
        rows, cols, blocks = e.binned(nx, 1, nz), e.binned(1, ny, nz), e.binned(4, 4, 4)
        cells_after, _ = e.store()
    assert hist["step"].tolist() == [2, 4, 6] and hist["ux"].shape == (3, 1, ny, 1) and "rho" not in hist
    assert np.array_equal(_b64(hist["ux"][-1]), _b64(rows["ux"]))
    assert prof["ux"].shape == (ny,)
    assert np.array_equal(_b64(prof["ux"]), _b64(lio.binned_means(rows)["ux"].reshape(-1)))
    assert flux.shape == (nx,) and np.array_equal(_b64(flux), _b64(cols["jx"].reshape(-1)))
    assert tuple(coarse) == ("ux", "uy", "uz", "speed") and coarse["uz"].shape == (3, 3, 18)
    assert np.array_equal(_b64(coarse["speed"]), _b64(lio.binned_means(blocks)["speed"]))
    assert coarse["speed"][0, 0, 0] == 0 and coarse["speed"].max() > 0
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:      # the calls left the run alone
        e.load_cells(c0)
        e.run_steps(6)
        plain, _ = e.store()
    assert np.array_equal(_b32(cells_after), _b32(plain))


def test_binned3d_contract(gpu_lib):
    n = gpu_lib
    nx, ny, nz = 4, 18, 4
    p, obst, c0 = _problem(nx, ny, nz, 9)
    nf = len(n.BIN_FIELDS3D)
    f64p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)

    def ptrs(arrays):
        out = (f64p * nf)()
        for i, a in arrays.items():
            out[i] = a.ctypes.data_as(f64p)
        return out

    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        out = {i: np.full((nz, ny, nx), SENTINEL64, np.uint64).view(np.float64) for i in range(nf)}
        untouched = lambda idx: all((_b64(out[i]) == SENTINEL64).all() for i in idx)
        assert L.lbm3d_store_binned(h, 1, 1, 1, ptrs(out)) == n.LBM_E_STATE
        e.load_cells(c0)
        e.run_steps(2)
        count = np.full((nz, ny, nx), -7, np.int64)
        for bins in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (nx + 1, 1, 1), (1, ny + 1, 1), (1, 1, nz + 1)):
            assert L.lbm3d_store_binned(h, *bins, ptrs(out)) == n.LBM_E_INVALID, bins
            assert L.lbm3d_bin_fluid_cells(h, *bins, count.ctypes.data_as(i64p)) == n.LBM_E_INVALID, bins
        assert untouched(range(nf)) and (count == -7).all()
        assert L.lbm3d_store_binned(h, 1, 1, 1, ptrs({})) == n.LBM_OK
        assert L.lbm3d_store_binned(h, 1, 1, 1, None) == n.LBM_OK
        assert L.lbm3d_bin_fluid_cells(h, 1, 1, 1, None) == n.LBM_OK
        terms = _terms(e, p, obst)
        assert L.lbm3d_store_binned(h, 1, 1, 1, ptrs({3: out[3], 13: out[13]})) == n.LBM_OK
        assert np.array_equal(_b64(out[3]), _b64(terms["jz"])) and np.array_equal(_b64(out[13]), _b64(terms["uzuz"]))
        assert untouched([i for i in range(nf) if i not in (3, 13)])
        assert L.lbm3d_bin_fluid_cells(h, 1, 1, 1, count.ctypes.data_as(i64p)) == n.LBM_OK
        assert np.array_equal(count, (obst == 0).astype(np.int64))
