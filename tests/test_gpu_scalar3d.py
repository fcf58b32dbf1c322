"""The passive scalar on the device, D3Q19 + D3Q7 (lbm3d_scalar_*;
include/lbm_scalar_hip.h, csrc/lbm3d_scalar.hip, csrc/lbm_scalar.hpp).

Bar: after every scalar_advance the populations and phi are BITWISE (uint32
patterns) lio.scalar_step3d applied to the same handle's fields() at that
moment (and lio.scalar_apply_fixed3d after every step), for both numerics,
both sides of the flow pair, advance(1 | 2 | 3), handles of 2 and 3 z slabs
(whose bits are the single-slab handle's) and degenerate shapes.  The
statistics' extremes are exact and the sum lies within the fold bound DESIGN
4.14 states for fp64 sums of the exact sum.  No other tolerance anywhere.
"""
from __future__ import annotations

import ctypes
import functools
import math

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)      # flow steps before each advance: both lattices of the pair get read
ADVANCES = (1, 2, 3, 1, 2)
GRIDS = [(13, 7, 5), (16, 8, 8)]
OMEGA_S = 1.3


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_b32(a), _b32(b))


def _fold_bound(phi):
    """a sum of n terms folded in fp64 lies within 2 (n - 1) 2^-53 sum|term| of the exact sum."""
    return 2.0 * (phi.size - 1) * 2.0 ** -53 * math.fsum(np.abs(phi.astype(np.float64)).ravel().tolist())


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, obstacles=0.1, walls=True):
    """The channel walls plus about 10 % random obstacles; populations perturbed by 5 %; phi0 in [1, 2)."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < obstacles).astype(np.uint8)
    if walls:
        obst |= lio.channel_obstacles3d(nx, ny, nz)
        obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    phi0 = (1 + rng.random((nz, ny, nx))).astype(np.float32)
    for a in (obst, c0, phi0):
        a.setflags(write=False)
    return p, obst, c0, phi0


def _fixed(p, obst, seed=3, n=9):
    rng = np.random.default_rng(seed)
    cells = {(0, 0, 0), (p.nx - 1, p.ny - 1, p.nz - 1), (p.nx // 2, p.ny // 2, p.nz // 2),
             (p.nx // 2, p.ny // 2, max(p.nz // 2 - 1, 0))}
    ob, fl = np.argwhere(obst != 0), np.argwhere(obst == 0)
    if len(ob):
        cells.add(tuple(int(v) for v in ob[0][::-1]))
    if len(fl):
        cells.add(tuple(int(v) for v in fl[-1][::-1]))
    while len(cells) < min(n, p.nx * p.ny * p.nz):
        cells.add((int(rng.integers(p.nx)), int(rng.integers(p.ny)), int(rng.integers(p.nz))))
    x, y, z = np.array(sorted(cells), np.int32).T
    return x, y, z, (3 + rng.random(x.size)).astype(np.float32)


def _advance_and_check(e, obst, g, n, fixed=None, what=""):
    f = e.fields(("ux", "uy", "uz"))
    for _ in range(n):
        g = lio.scalar_step3d(g, f["ux"], f["uy"], f["uz"], obst, OMEGA_S)
        if fixed is not None:
            g = lio.scalar_apply_fixed3d(g, *fixed)
    before = e.scalar_steps
    e.scalar_advance(n)
    assert e.scalar_steps == before + n
    phi, got = e.scalar(populations=True)
    assert got.dtype == np.float32 and got.shape == g.shape
    bad = _b32(got) != _b32(g)
    assert not bad.any(), (what, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert _same(phi, lio.scalar_phi(g)) and _same(e.scalar(), phi), (what, n)
    return g


def _sequence(e, p, obst, c0, phi0, fixed=None, what="", chunks=CHUNKS):
    e.load_cells(c0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    g = lio.scalar_init3d(phi0)
    assert _same(e.scalar(populations=True)[1], g) and e.scalar_steps == 0
    if fixed is not None:
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed3d(g, *fixed)
        assert _same(e.scalar(populations=True)[1], g)
    for steps, n in zip(chunks, ADVANCES):
        e.run_steps(steps)
        g = _advance_and_check(e, obst, g, n, fixed, what)
    return g


# ------------------------------------------------------------ 1. parity ----

@pytest.mark.parametrize("with_fixed", [False, True])
@pytest.mark.parametrize("form", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_advance_sequences_bitwise(gpu_lib, nx, ny, nz, form, with_fixed):
    p, obst, c0, phi0 = _problem(nx, ny, nz, 7)
    fixed = _fixed(p, obst) if with_fixed else None
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        g = _sequence(e, p, obst, c0, phi0, fixed, (nx, ny, nz, form, with_fixed))
    assert np.abs(lio.scalar_phi(g) - phi0).max() > 1e-3         # the scalar moved


def test_wide_rows_cross_waves_and_blocks(gpu_lib):
    """nx = 300: more than one wave of quads per row (a cross-lane move must not leave its wave) and a ragged
    tail; nx = 258: the tail of two cells."""
    for nx in (300, 258):
        p, obst, c0, phi0 = _problem(nx, 5, 3, nx)
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            _sequence(e, p, obst, c0, phi0, _fixed(p, obst), nx, chunks=(2, 1))


# ------------------------------------------------------ 2. z slabs ----

@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for grid in GRIDS:
        p, obst, c0, phi0 = _problem(*grid, 11)
        fixed = _fixed(p, obst)
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            assert len(e.local_slabs()) == 1
            g = _sequence(e, p, obst, c0, phi0, fixed, "single")
            stats = e.scalar_stats()
        g.setflags(write=False)
        out[grid] = (p, obst, c0, phi0, fixed, g, stats)
    return out


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_bits_do_not_depend_on_the_slabs(gpu_lib, single, nx, ny, nz, parts):
    p, obst, c0, phi0, fixed, ref, ref_stats = single[(nx, ny, nz)]
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        assert len(e.local_slabs()) == parts
        g = _sequence(e, p, obst, c0, phi0, fixed, (nx, ny, nz, parts))
        total, lo, hi = e.scalar_stats()
    assert _same(g, ref)
    assert (lo, hi) == ref_stats[1:] and abs(total - ref_stats[0]) <= _fold_bound(lio.scalar_phi(ref))


# ------------------------------------------------- 3. degenerate shapes ----

@pytest.mark.parametrize("nx,ny,nz", [(1, 5, 4), (6, 1, 4), (6, 5, 1), (1, 1, 1), (3, 2, 2), (4, 1, 1), (5, 4, 1)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny, nz):
    p, obst, c0, phi0 = _problem(nx, ny, nz, 5, 0.2 if nx * ny * nz > 8 else 0.0, False)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        _sequence(e, p, obst, c0, phi0, _fixed(p, obst, n=2), (nx, ny, nz), chunks=(3, 2, 1))


def test_all_obstacle_grid(gpu_lib):
    p, _, c0, phi0 = _problem(9, 4, 3, 2)
    obst = np.ones((3, 4, 9), np.uint8)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        g = _sequence(e, p, obst, c0, phi0, None, "all obstacles", chunks=(1, 2))
        total, lo, hi = e.scalar_stats()
    assert lo == np.inf and hi == -np.inf
    assert abs(total - lio.scalar_stats3d(g, obst)[0]) <= _fold_bound(lio.scalar_phi(g))


# ----------------------------------------------- 4. fixed cells, stats ----

def test_fixed_cells_and_stats(gpu_lib):
    n = gpu_lib
    p, obst, c0, phi0 = _problem(16, 8, 8, 23)
    phi0 = (phi0 - np.float32(1.5)).astype(np.float32)
    fz, fy, fx = [int(v) for v in np.argwhere(obst == 0)[7]]
    oz, oy, ox = [int(v) for v in np.argwhere(obst != 0)[3]]
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    P = lambda a, t: a.ctypes.data_as(t)
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        e.load_cells(c0)
        e.run_steps(3)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        fixed = tuple(np.array(v, np.int32) for v in ([fx, ox], [fy, oy], [fz, oz])) + (np.array([5, -2], np.float32),)
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed3d(lio.scalar_init3d(phi0), *fixed)
        assert _same(e.scalar(populations=True)[1], g)
        g = _advance_and_check(e, obst, g, 3, fixed, "fixed")
        phi = lio.scalar_phi(g)
        assert phi[fz, fy, fx] == np.float32(5) and phi[oz, oy, ox] == np.float32(-2)
        # stats: the fixed obstacle cell holds the minimum of all cells, which the fluid minimum must not see
        total, lo, hi = e.scalar_stats()
        want, wlo, whi = lio.scalar_stats3d(g, obst)
        print(f"16x8x8: total {total!r} exact {want!r} bound {_fold_bound(phi):.3e}")
        assert abs(total - want) <= _fold_bound(phi) and np.float32(lo) == wlo and np.float32(hi) == whi
        assert hi == 5.0 and lo > -2.0 == phi.min()
        again = e.scalar_stats()
        assert np.array_equal(np.array(again[:1]).view(np.uint64), np.array([total]).view(np.uint64))
        assert again[1:] == (lo, hi)
        # refused lists: the old list stays
        val = np.array([1.0, 1.0], np.float32)
        for bad in (([0, p.nx], [0, 0], [0, 0]), ([0, 0], [0, p.ny], [0, 0]), ([0, 0], [0, 0], [0, p.nz]),
                    ([0, 0], [0, 0], [-1, 0]), ([3, 3], [4, 4], [2, 2])):
            xb, yb, zb = [np.array(v, np.int32) for v in bad]
            assert L.lbm3d_scalar_set_fixed(h, 2, P(xb, i32p), P(yb, i32p), P(zb, i32p),
                                            P(val, f32p)) == n.LBM_E_INVALID, bad
        assert L.lbm3d_scalar_set_fixed(h, 1, P(xb, i32p), P(yb, i32p), None, P(val, f32p)) == n.LBM_E_INVALID
        g = _advance_and_check(e, obst, g, 1, fixed, "old list kept")
        assert L.lbm3d_scalar_set_fixed(h, 0, None, None, None, None) == n.LBM_OK
        _advance_and_check(e, obst, g, 2, None, "cleared")


# ------------------------------------- 5. no engine state touched, runs ----

def test_scalar_touches_no_engine_state_and_run_scalar(gpu_lib):
    p, obst, c0, phi0 = _problem(16, 8, 8, 21)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(c0)
        e.scalar_begin(phi0, diffusivity=0.05)
        e.scalar_fix(*_fixed(p, obst))
        e.run_steps(7)
        e.scalar_advance(3)
        e.scalar(populations=True)
        e.scalar_stats()
        e.run_steps(6)
        cells_a, _ = e.store()
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(13)
        cells, _ = e.store()
    assert np.array_equal(_b32(cells_a), _b32(cells))
    # run_scalar(13, 5): chunks 5, 5, 3, each followed by as many scalar steps
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        g = lio.scalar_init3d(phi0)
        for n in (5, 5, 3):
            e.run_steps(n)
            g = _advance_and_check(e, obst, g, n, None, "by hand")
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        av = e.run_scalar(13, 5)
        assert av.size == 0 and e.scalar_steps == 13 and _same(e.scalar(populations=True)[1], g)
        hist = e.scalar_history(4, 3)
        assert [s[0] for s in hist] == [3, 4] and e.scalar_steps == 17 and hist[-1][1:] == e.scalar_stats()
        with pytest.raises(ValueError):
            e.run_scalar(5, 1, accelerate_first=True)


# ---------------------------------------------------------- 6. contract ----

def test_scalar_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0, phi0 = _problem(13, 7, 5, 9)
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        cnt = ctypes.c_int64(-1)
        tot = ctypes.c_double(-1)
        assert L.lbm3d_scalar_advance(h, 1) == n.LBM_E_STATE
        assert L.lbm3d_scalar_steps(h, ctypes.byref(cnt)) == n.LBM_E_STATE
        assert L.lbm3d_scalar_steps(h, None) == n.LBM_E_INVALID
        assert L.lbm3d_scalar_store(h, None, None) == n.LBM_E_STATE
        assert L.lbm3d_scalar_stats(h, ctypes.byref(tot), None, None) == n.LBM_E_STATE
        assert L.lbm3d_scalar_set_fixed(h, 0, None, None, None, None) == n.LBM_E_STATE
        assert L.lbm3d_scalar_end(h) == n.LBM_OK and cnt.value == -1 and tot.value == -1
        for om in (0.0, 2.0, -0.5, float("nan"), float("inf")):
            assert L.lbm3d_scalar_begin(h, om, None) == n.LBM_E_INVALID, om
        e.scalar_begin(None, omega_s=OMEGA_S)
        assert L.lbm3d_scalar_advance(h, 1) == n.LBM_E_STATE and L.lbm3d_scalar_advance(h, -1) == n.LBM_E_INVALID
        ph, g = e.scalar(populations=True)
        assert g.shape == (7, 5, 7, 13) and not _b32(ph).any() and not _b32(g).any()
        e.load_cells(c0)
        e.run_steps(2)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert L.lbm3d_scalar_advance(h, 0) == n.LBM_OK and e.scalar_steps == 0
        g = _advance_and_check(e, obst, lio.scalar_init3d(phi0), 2, None, "contract")
        assert L.lbm3d_scalar_begin(h, 2.0, None) == n.LBM_E_INVALID
        assert e.scalar_steps == 2 and _same(e.scalar(populations=True)[1], g)
        e.scalar_end()
        assert L.lbm3d_scalar_advance(h, 1) == n.LBM_E_STATE and L.lbm3d_scalar_end(h) == n.LBM_OK
        e.scalar_begin(phi0, omega_s=OMEGA_S)     # destroyed with a scalar: lbm3d_destroy frees it
    p, obst, c0, phi0 = _problem(8, 4, 34, 4)
    with n.Engine3D(p, obst, parts=17, devices=[0]) as e:
        assert len(e.local_slabs()) == 17 > n.SCALAR_MAX_PARTS
        with pytest.raises(n.LbmError, match="more than 16 local slabs") as err:
            e.scalar_begin(phi0, omega_s=1.0)
        assert err.value.code == n.LBM_E_INVALID
