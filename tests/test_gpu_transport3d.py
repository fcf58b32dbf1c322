"""The scalar transport sums on the device, D3Q19 + D3Q7 (lbm3d_scalar_store_binned;
include/lbm_transport_hip.h, csrc/lbm3d_transport.hip, csrc/lbm_transport.hpp).

Bar: after every chunk of flow and scalar steps the sums are lio.scalar_binned_sums3d of the same
handle's fields() and scalar(populations=True): BITWISE (uint64 patterns) at one-cell bins, within
the fold bound 2 (n - 1) 2^-53 sum|term| of the math.fsum value at larger bins -- for both numerics,
both sides of both ping-pong pairs, handles of 2 and 3 z slabs, degenerate shapes and subsets of
the fields (the no-flow form of the kernel).  A call changes nothing on the handle.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

import thermal_cases as tc
import transport_cases as xc
from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2)
ADVANCES = (1, 2, 3, 1)
GRIDS = [(13, 7, 5), (16, 8, 4)]
OMEGA_S = 1.3
FACES = ("fx", "fy", "fz")

_same = tc.same


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, obstacles=0.1, walls=True):
    """The channel walls plus about 10 % random obstacles; populations perturbed by 5 %; phi0 in [-1, 1)."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < obstacles).astype(np.uint8)
    if walls:
        obst |= lio.channel_obstacles3d(nx, ny, nz)
        obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    phi0 = (2 * rng.random((nz, ny, nx)) - 1).astype(np.float32)
    for a in (obst, c0, phi0):
        a.setflags(write=False)
    return p, obst, c0, phi0


def _fixed(p, obst):
    cells = {(0, 0, 0), (p.nx - 1, p.ny - 1, p.nz - 1)}
    for a in (np.argwhere(obst != 0), np.argwhere(obst == 0)):
        if len(a):
            cells.add(tuple(int(v) for v in a[len(a) // 2][::-1]))
    x, y, z = np.array(sorted(cells), np.int32).T
    return x, y, z, np.linspace(2, 3, x.size).astype(np.float32)


def _begin(e, p, obst, c0, phi0):
    e.load_cells(c0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    e.scalar_fix(*_fixed(p, obst))


def _terms(e, obst):
    f = e.fields(("ux", "uy", "uz"))
    return lio.scalar_terms3d(e.scalar(populations=True)[1], f["ux"], f["uy"], f["uz"], obst)


def _sequence(e, p, obst, c0, phi0, bins_list, what="", chunks=CHUNKS):
    _begin(e, p, obst, c0, phi0)
    last = None
    for i, (steps, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(steps)
        e.scalar_advance(n)
        terms = _terms(e, obst)
        for bins in bins_list:
            got = e.scalar_binned(*bins)
            assert set(got) == set(lio.SBIN_FIELDS3D) | {"fluid"}
            xc.check_binned(got, terms, obst, bins, (what, i, bins))
        last = terms
    return last


def _bins(nx, ny, nz):
    return [(nx, ny, 1), (nx, 1, nz), (1, ny, nz), (min(3, nx), min(2, ny), min(2, nz)), (nx, ny, nz)]


# ------------------------------------------------------ 1. parity ----

@pytest.mark.parametrize("form", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_one_cell_and_larger_bins(gpu_lib, nx, ny, nz, form):
    p, obst, c0, phi0 = _problem(nx, ny, nz, 7)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        terms = _sequence(e, p, obst, c0, phi0, [(1, 1, 1)] + _bins(nx, ny, nz), (nx, ny, nz, form))
    assert all(np.abs(terms[n]).max() > 1e-5 for n in lio.SBIN_FIELDS3D)


@pytest.mark.parametrize("nx,ny,nz", [(1, 1, 1), (2, 3, 1), (5, 1, 3), (4, 4, 1)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny, nz):
    """The periodic self-neighbour along every axis and the row-end direct load."""
    p, obst, c0, phi0 = _problem(nx, ny, nz, 5, 0.2 if nx * ny * nz > 8 else 0.0, False)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        _sequence(e, p, obst, c0, phi0, [(1, 1, 1), (nx, ny, nz)], (nx, ny, nz), chunks=(3, 2))


def test_a_row_of_several_waves(gpu_lib):
    """nx = 150: a row spans three waves, so the cross-lane move meets wave borders; bins that straddle them."""
    p, obst, c0, phi0 = _problem(150, 3, 2, 150)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        _sequence(e, p, obst, c0, phi0, [(1, 1, 1), (150, 3, 2), (7, 2, 1)], 150, chunks=(2, 1))


# ------------------------------------------------------ 2. z slabs ----

@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for grid in GRIDS:
        p, obst, c0, phi0 = _problem(*grid, 11)
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            assert len(e.local_slabs()) == 1
            _sequence(e, p, obst, c0, phi0, [(1, 1, 1)], "single")
            ref = e.scalar_binned(1, 1, 1)
        for a in ref.values():
            a.setflags(write=False)
        out[grid] = (p, obst, c0, phi0, ref)
    return out


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_bits_do_not_depend_on_the_slabs(gpu_lib, single, nx, ny, nz, parts):
    p, obst, c0, phi0, ref = single[(nx, ny, nz)]
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        assert len(e.local_slabs()) == parts
        _sequence(e, p, obst, c0, phi0, [(1, 1, 1)] + _bins(nx, ny, nz), (nx, ny, nz, parts))
        got = e.scalar_binned(1, 1, 1)
    for name in ref:
        assert np.array_equal(got[name].view(np.uint64), ref[name].view(np.uint64)), name


# ------------------------------------- 3. subsets, purity, contract ----

def test_which_subsets(gpu_lib):
    n = gpu_lib
    p, obst, c0, phi0 = _problem(13, 7, 5, 3)
    with n.Engine3D(p, obst, devices=[0]) as e:
        _begin(e, p, obst, c0, phi0)
        e.run_steps(3)
        e.scalar_advance(2)
        terms = _terms(e, obst)
        full = e.scalar_binned(1, 1, 1)
        for which in (FACES, ("fy",), ("fz",), ("fx", "phi"), ("phiphi",), ("uzphi",), ("uxphi", "fz")):
            got = e.scalar_binned(1, 1, 1, which=which)
            assert set(got) == set(which) | {"fluid"}
            for name in which:
                assert np.array_equal(got[name].view(np.uint64), full[name].view(np.uint64)), (which, name)
            for bins in ((3, 2, 2), (13, 7, 1), (13, 7, 5)):
                xc.check_binned(e.scalar_binned(*bins, which=which), terms, obst, bins, (which, bins))
        none = (ctypes.POINTER(ctypes.c_double) * 8)()
        assert e._L.lbm3d_scalar_store_binned(e._h, 2, 2, 2, none) == n.LBM_OK
        assert e._L.lbm3d_scalar_store_binned(e._h, 2, 2, 2, None) == n.LBM_OK
        prof = e.scalar_profile(2)
        planes = e.scalar_binned(13, 7, 1)
        assert all(prof[k].shape == (5,) and np.array_equal(prof[k], planes[k].reshape(-1)) for k in planes)
        d = lio.scalar_diffusivity(np.float32(OMEGA_S), 3)
        assert np.array_equal(e.nusselt(2, 1.0, 4.0), lio.nusselt_number(prof["fz"], 13 * 7, d, 1.0, 4.0))
        hist = e.transport_history(5, 2, 13, 7, 1, which=FACES)
        assert hist["step"].tolist() == [2, 4, 5] and hist["fz"].shape == (3, 5, 1, 1) and e.scalar_steps == 7
        last = e.scalar_binned(13, 7, 1, which=FACES)
        assert all(np.array_equal(hist[k][-1].view(np.uint64), last[k].view(np.uint64)) for k in FACES)


def test_calls_change_nothing(gpu_lib):
    p, obst, c0, phi0 = _problem(16, 8, 4, 21)

    def run(with_calls):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            _begin(e, p, obst, c0, phi0)
            e.run_steps(3)
            e.scalar_advance(2)
            if with_calls:
                cells, g = e.store()[0], e.scalar(populations=True)[1]
                a, b = e.scalar_binned(3, 2, 2), e.scalar_binned(3, 2, 2)
                for name in a:
                    assert np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64)), name
                e.scalar_binned(1, 1, 1, which=FACES)
                assert _same(e.store()[0], cells) and _same(e.scalar(populations=True)[1], g)
                assert e.scalar_steps == 2
            e.run_steps(4)
            e.scalar_advance(3)
            return e.store()[0], e.scalar(populations=True)[1]

    (cells_a, g_a), (cells_b, g_b) = run(True), run(False)
    assert _same(cells_a, cells_b) and _same(g_a, g_b)


def test_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0, phi0 = _problem(13, 7, 5, 9)
    f64p = ctypes.POINTER(ctypes.c_double)
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        out = np.full((8, p.nz, p.ny, p.nx), 7.0)
        table = (f64p * 8)(*[out[f].ctypes.data_as(f64p) for f in range(8)])
        call = lambda bw=1, bh=1, bd=1: L.lbm3d_scalar_store_binned(h, bw, bh, bd, table)       # noqa: E731
        assert L.lbm3d_scalar_store_binned(None, 1, 1, 1, table) == n.LBM_E_INVALID
        assert call() == n.LBM_E_STATE                                    # before scalar_begin
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert call() == n.LBM_E_STATE                                    # before the lattice is loaded
        e.load_cells(c0)
        for bins in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (p.nx + 1, 1, 1), (1, p.ny + 1, 1), (1, 1, p.nz + 1), (1, -2, 1)):
            assert call(*bins) == n.LBM_E_INVALID, bins
        assert (out == 7).all()
        assert call() == n.LBM_OK and not (out == 7).any()
        e.scalar_end()
        assert call() == n.LBM_E_STATE
