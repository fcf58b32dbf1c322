"""Time-averaged fields and Reynolds stresses accumulated on the device, D3Q19
(lbm3d_avg_*; include/lbm_averages_hip.h, csrc/lbm3d_averages.hip).

Bar: the fp64 sums are BITWISE (uint64 patterns) lio.moment_sums of the same
handle's fields() after each chunk, and the fp32 means and central moments
BITWISE (uint32) lio.moment_means of those sums (the restatement pinned in
tests/test_averages_host.py), for both moment selections, the quad path with
its ragged tail, nx < 4, both numerics modes, both lattices of the pair and z
slabs.  Inputs follow tests/test_gpu_fields3d.py's recipe with about 10 %
obstacles.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

FIRST = ("ux", "uy", "uz", "pressure")
CHUNKS = (3, 1, 4, 2, 5)      # odd and even: both lattices of the pair get sampled
SENTINEL32 = 0x7FC00001
SENTINEL64 = 0x7FF8000000000001


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, accel=0.002):
    p = lio.Params3D(nx, ny, nz, 0, 0.1, accel, 1.7)
    rng = np.random.default_rng(seed)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    obst[rng.random((nz, ny, nx)) < 0.1] = 1
    c0 = (oracle.init_cells3d(p) * (1 + 0.02 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _names(e, second):
    return e._AVG_FIELDS if second else e._AVG_FIELDS[:len(FIRST)]


def _sample_run(e, chunks=CHUNKS):
    samples = []
    for n in chunks:
        if n:
            e.run_steps(n)
        e.avg_sample()
        f = e.fields(FIRST)
        samples.append([f[k] for k in FIRST])
    return samples


def _assert_averages(e, samples, second, what=""):
    names = _names(e, second)
    assert e.avg_samples == len(samples)
    sums = e.avg_sums()
    assert tuple(sums) == names
    ref = lio.moment_sums(samples, second)
    for name, r in zip(names, ref):
        assert sums[name].dtype == np.float64 and sums[name].shape == r.shape
        bad = _b64(sums[name]) != _b64(r)
        assert not bad.any(), (what, "sum", name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    means = e.mean_fields()
    assert tuple(means) == names
    for name, r in zip(names, lio.moment_means(ref, len(samples))):
        assert means[name].dtype == np.float32
        bad = _b32(means[name]) != _b32(r)
        assert not bad.any(), (what, "mean", name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return sums, means


# ------------------------------------------------------------ 1. shapes ----

@pytest.mark.parametrize("second", [False, True], ids=["mean", "mean_second"])
@pytest.mark.parametrize("nx,ny,nz", [(13, 9, 7), (67, 5, 3), (4, 4, 4), (130, 3, 2)])
def test_averages3d_shapes_bitwise(gpu_lib, nx, ny, nz, second):
    p, obst, c0 = _problem(nx, ny, nz, nx + ny + nz)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin(second=second)
        sums, means = _assert_averages(e, _sample_run(e), second, (nx, ny, nz))
    ob = obst != 0
    assert ob.any()
    for name in ("ux", "uy", "uz"):
        assert not _b64(sums[name])[ob].any() and not _b32(means[name])[ob].any()
    assert (_b32(means["pressure"])[ob] ==
            _b32(np.float32(p.density) * np.float32(np.float32(1) / np.float32(3)))).all()


def test_averages3d_narrow_rows(gpu_lib):
    """nx < 4: every cell on the one-cell path."""
    p, obst, c0 = _problem(3, 5, 4, 11)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin()
        _assert_averages(e, _sample_run(e, (2, 1)), True, "nx=3")


# --------------------------------------------------- 2. numerics modes ----

@pytest.mark.parametrize("mode", ["bitwise", "tolerance"])
def test_averages3d_default_pass_both_modes(gpu_lib, mode):
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if mode == "tolerance" else 0)
    p, obst, c0 = _problem(70, 31, 24, 7)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        e.avg_begin()
        _assert_averages(e, _sample_run(e), True, mode)


# --------------------------------------------------------------- 3. slabs ----

@pytest.fixture(scope="module")
def single_13x9x7(gpu_lib):
    p, obst, c0 = _problem(13, 9, 7, 41)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin()
        sums, means = _assert_averages(e, _sample_run(e), True, "single")
    for a in list(sums.values()) + list(means.values()):
        a.setflags(write=False)
    return p, obst, c0, sums, means


@pytest.mark.parametrize("parts", [2, 3])
def test_averages3d_slabs_bitwise(gpu_lib, single_13x9x7, parts):
    p, obst, c0, ref_sums, ref_means = single_13x9x7
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin()
        _sample_run(e)
        assert len(e.local_slabs()) == parts
        sums, means = e.avg_sums(), e.mean_fields()
    for name in gpu_lib.AVG_FIELDS3D:
        assert np.array_equal(_b64(sums[name]), _b64(ref_sums[name])), (parts, name)
        assert np.array_equal(_b32(means[name]), _b32(ref_means[name])), (parts, name)


# ------------------------------------------------- 4. constant lattice ----

def test_averages3d_of_a_constant_lattice(gpu_lib):
    p, obst, c0 = _problem(67, 5, 3, 5)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin()
        for _ in range(5):
            e.avg_sample()
        f = e.fields(FIRST)
        means = e.mean_fields()
    for name in FIRST:
        assert np.array_equal(_b32(means[name]), _b32(f[name])), name
    for name in gpu_lib.AVG_FIELDS3D[4:]:
        assert not _b32(means[name]).any(), name     # exactly +0


# -------------------------------------------- 5. no engine state touched ----

def test_sampling3d_touches_no_engine_state(gpu_lib):
    p, obst, c0 = _problem(70, 31, 24, 7)

    def sampled():
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            e.load_cells(c0)
            e.avg_begin()
            e.run_steps(7)
            e.avg_sample()
            e.run_steps(6)
            e.avg_sample()
            return e.store()[0], e.avg_sums()

    cells_a, sums_a = sampled()
    cells_b, sums_b = sampled()
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(13)
        cells, _ = e.store()
    assert np.array_equal(_b32(cells_a), _b32(cells)) and np.array_equal(_b32(cells_b), _b32(cells))
    for name in gpu_lib.AVG_FIELDS3D:
        assert np.array_equal(_b64(sums_a[name]), _b64(sums_b[name])), name


def test_run_averaged3d(gpu_lib):
    p, obst, c0 = _problem(13, 9, 7, 41)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin()
        e.run_averaged(23, 5)
        assert e.avg_samples == 5
        sums = e.avg_sums()
        cells, _ = e.store()
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.avg_begin()
        ref = lio.moment_sums(_sample_run(e, (5, 5, 5, 5, 3)), True)
        ref_cells, _ = e.store()
    assert np.array_equal(_b32(cells), _b32(ref_cells))
    for name, r in zip(gpu_lib.AVG_FIELDS3D, ref):
        assert np.array_equal(_b64(sums[name]), _b64(r)), name


# ---------------------------------------------------------- 6. contract ----

def _ptrs(ctype, n, arrays):
    out = (ctypes.POINTER(ctype) * n)()
    for i, a in arrays.items():
        out[i] = a.ctypes.data_as(ctypes.POINTER(ctype))
    return out


def test_averages3d_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(13, 9, 7, 41)
    nf = len(n.AVG_FIELDS3D)
    shape = (p.nz, p.ny, p.nx)
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        f32 = {i: np.full(shape, SENTINEL32, np.uint32).view(np.float32) for i in range(nf)}
        f64 = {i: np.full(shape, SENTINEL64, np.uint64).view(np.float64) for i in range(nf)}
        all32, all64 = _ptrs(ctypes.c_float, nf, f32), _ptrs(ctypes.c_double, nf, f64)
        none32, none64 = _ptrs(ctypes.c_float, nf, {}), _ptrs(ctypes.c_double, nf, {})

        def untouched():
            return all((_b32(a) == SENTINEL32).all() for a in f32.values()) and \
                all((_b64(a) == SENTINEL64).all() for a in f64.values())

        assert L.lbm3d_avg_sample(h) == n.LBM_E_STATE
        assert L.lbm3d_avg_store(h, all32) == n.LBM_E_STATE
        assert L.lbm3d_avg_store_sums(h, all64) == n.LBM_E_STATE
        assert L.lbm3d_avg_end(h) == n.LBM_OK
        for bad in (0, 2, 4, -1):
            assert L.lbm3d_avg_begin(h, bad) == n.LBM_E_INVALID, bad
        assert L.lbm3d_avg_begin(h, n.AVG_MEAN) == n.LBM_OK
        assert L.lbm3d_avg_sample(h) == n.LBM_E_STATE          # no lattice yet
        e.load_cells(c0)
        assert L.lbm3d_avg_store(h, _ptrs(ctypes.c_float, nf, {i: f32[i] for i in range(4)})) == n.LBM_E_STATE  # zero samples
        assert L.lbm3d_avg_store_sums(h, _ptrs(ctypes.c_double, nf, {3: f64[3]})) == n.LBM_OK
        assert not _b64(f64[3]).any()
        _b64(f64[3])[...] = SENTINEL64
        assert L.lbm3d_avg_store(h, none32) == n.LBM_OK and L.lbm3d_avg_store_sums(h, none64) == n.LBM_OK
        assert L.lbm3d_avg_sample(h) == n.LBM_OK
        assert L.lbm3d_avg_store(h, all32) == n.LBM_E_INVALID  # second moments of a MEAN handle
        assert L.lbm3d_avg_store_sums(h, all64) == n.LBM_E_INVALID
        assert untouched()
        fields = e.fields(FIRST)
        assert L.lbm3d_avg_store(h, _ptrs(ctypes.c_float, nf, {2: f32[2]})) == n.LBM_OK
        assert np.array_equal(_b32(f32[2]), _b32(fields["uz"]))
        _b32(f32[2])[...] = SENTINEL32
        assert untouched()
        assert L.lbm3d_avg_begin(h, n.AVG_MEAN | n.AVG_SECOND) == n.LBM_OK      # re-allocates, zeroed
        assert e.avg_samples == 0 and not any(_b64(v).any() for v in e.avg_sums(n.AVG_FIELDS3D).values())
        assert L.lbm3d_avg_sample(h) == n.LBM_OK and L.lbm3d_avg_begin(h, 3) == n.LBM_OK   # re-zeroes
        assert e.avg_samples == 0 and not any(_b64(v).any() for v in e.avg_sums(n.AVG_FIELDS3D).values())
        assert L.lbm3d_avg_sample(h) == n.LBM_OK
        assert L.lbm3d_avg_store(h, all32) == n.LBM_OK and L.lbm3d_avg_store_sums(h, all64) == n.LBM_OK
        assert np.array_equal(_b32(f32[3]), _b32(fields["pressure"]))
        assert L.lbm3d_avg_end(h) == n.LBM_OK
        assert L.lbm3d_avg_sample(h) == n.LBM_E_STATE
        e.avg_begin()        # destroyed while averaging: lbm3d_destroy frees the sums
