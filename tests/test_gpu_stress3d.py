"""Strain rate and wall shear from the non-equilibrium moments on the device, D3Q19
(lbm3d_store_stress / _box / lbm3d_stress_stats; include/lbm_stress_hip.h,
csrc/lbm3d_stress.hip).

Bar: every field is BITWISE (uint32 patterns) lio.neq_strain3d of the same
handle's store() cells (the restatement pinned in tests/test_stress_host.py),
on both lattices of the pair, on 1, 2 and 3 z slabs, after one-, two- and
three-step passes, around the kernel's block (256 cells along x on the 16-B
path, 4 rows, 8 planes) and for boxes.  Statistics as in
tests/test_gpu_stress.py.  On the device's own Poiseuille channel s_xy meets the
analytic profile at the wall-adjacent cells.
"""
from __future__ import annotations

import ctypes
import functools
import struct

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

OMEGA, DENSITY = 1.85, 0.1
BX, BY, BZ = 256, 4, 8        # native.STRESS3D_BLOCK (asserted below)


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _d64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, accel=0.002):
    """About 10 % random obstacles, blocked cells on the periodic faces and on both sides of
    the kernel's block borders; populations perturbed by 5 %."""
    p = lio.Params3D(nx, ny, nz, 0, DENSITY, accel, OMEGA)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < 0.1).astype(np.uint8)
    obst[0, ny // 2, 0] = obst[nz - 1, ny // 2, nx - 1] = 1
    obst[nz // 2, 0, nx // 2] = obst[nz // 2, ny - 1, nx // 3] = 1
    for xb in range(BX, nx, BX):
        obst[nz // 2, ny // 2, xb - 1] = obst[nz // 3, ny // 3, xb] = 1
    for yb in range(BY, ny, BY):
        obst[nz // 2, yb - 1, nx // 3] = obst[nz // 3, yb, (2 * nx) // 3] = 1
    for zb in range(BZ, nz, BZ):
        obst[zb - 1, ny // 3, nx // 3] = obst[zb, (2 * ny) // 3, (2 * nx) // 3] = 1
    obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _reference(e, p, obst):
    cells, _ = e.store()
    return lio.neq_strain3d(np.asarray(cells).reshape(p.nz, p.ny, p.nx, 19), obst, p.omega)


def _assert_fields(got, ref, names, what="", cut=None):
    for name in names:
        r = ref[name] if cut is None else ref[name][cut]
        assert got[name].dtype == np.float32 and got[name].shape == r.shape, (what, name, got[name].shape, r.shape)
        bad = _b32(got[name]) != _b32(r)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _same_stats(a, b):
    return [_d64(a[0]), a[1], a[2], _d64(a[3]), a[4]] == [_d64(b[0]), b[1], b[2], _d64(b[3]), b[4]]


def _assert_stats(stats, ref, obst, what=""):
    s2, ms, nw, sw, mw = stats
    near = lio.near_wall3d(obst)
    rs2, rms, rnw, rsw, rmw = lio.strain_stats(ref, obst, near)
    n = int((np.asarray(obst) == 0).sum())
    assert nw == rnw == int(near.sum()), (what, nw, rnw)
    assert _b32(np.float32(ms)) == _b32(rms) and _b32(np.float32(mw)) == _b32(rmw), (what, ms, rms, mw, rmw)
    print(what, "sum_s2", s2, rs2, "sum_wall_strain", sw, rsw, "cells", n, "near-wall", nw)
    assert abs(s2 - rs2) <= 2 * max(n - 1, 0) * 2.0 ** -53 * rs2, (what, s2, rs2)
    assert abs(sw - rsw) <= 2 * max(nw - 1, 0) * 2.0 ** -53 * rsw, (what, sw, rsw)


def _check(e, p, obst, what=""):
    ref = _reference(e, p, obst)
    got = e.strain_rate()
    assert tuple(got) == e._STRESS_FIELDS
    _assert_fields(got, ref, e._STRESS_FIELDS, what)
    stats = e.strain_stats()
    _assert_stats(stats, ref, obst, what)
    assert _same_stats(stats, e.strain_stats()), what
    ob = np.asarray(obst) != 0
    for name in e._STRESS_FIELDS:
        assert not _b32(got[name])[ob].any(), (what, name)
    return ref, got, stats


# --------------------------------------------------- 1. shapes and slabs ----

# below / at / above the block's 4 rows (3, 4, 5, 6, 9, 18), 8 planes (7, 8, 9) and 256 cells along x
SHAPES = [(5, 6, 7), (33, 9, 8), (4, 18, 4),
          (8, 3, 2), (8, 4, 2), (8, 5, 9), (BX - 4, 3, 1), (BX, 3, 1), (BX + 4, 3, 2), (BX + 3, 3, 1)]
# 1, 2 and 3 z slabs on one GPU, where the domain has the planes
CASES = [s + (parts,) for s in SHAPES for parts in (1, 2, 3) if parts <= s[2]]


def test_strain3d_one_cell(gpu_lib):
    """1 x 1 x 1: the cell is its own neighbour in every direction.  Loaded populations
    only -- the step kernels' smallest extents are exercised by tests/test_d3q19.py."""
    p, obst, c0 = _problem(1, 1, 1, 3)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        _, got, stats = _check(e, p, obst, "1x1x1")
    assert got["strain"].any() and stats[2] == 0


@pytest.mark.parametrize("nx,ny,nz,parts", CASES)
def test_strain3d_shapes_and_slabs_bitwise(gpu_lib, nx, ny, nz, parts):
    assert gpu_lib.STRESS3D_BLOCK == (BX, BY, BZ)
    p, obst, c0 = _problem(nx, ny, nz, nx + ny + nz)
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        assert len(e.local_slabs()) == parts
        e.load_cells(c0)
        _check(e, p, obst, (nx, ny, nz, parts, "loaded"))
        e.run_steps(3)
        _, got, _ = _check(e, p, obst, (nx, ny, nz, parts, 3))
        e.run_steps(1)
        _check(e, p, obst, (nx, ny, nz, parts, 4))
        assert tuple(e.strain_rate(("syz", "sxx"))) == ("syz", "sxx")
        with pytest.raises(ValueError):
            e.strain_rate(("speed",))
    assert got["strain"].any()


def test_strain3d_rccl_world_1(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(33, 9, 8, 41)
    with n.Engine3D(p, obst, devices=[0], transport=n.TRANSPORT_RCCL, rank=0, world=1,
                    unique_id=n.rccl_unique_id()) as e:
        e.load_cells(c0)
        e.run_steps(5)
        _check(e, p, obst, "rccl1")


# ------------------------------------------------------- 2. pass forms ----

@pytest.mark.usefixtures("debug_knobs")
@pytest.mark.parametrize("form", ["three", "two", "one", "tolerance"])
def test_strain3d_every_pass_form(gpu_lib, form, monkeypatch):
    """Three-step passes (default), LBM3D_THREE=0 (two-step), LBM3D_TWO=0 (one-step
    launches) and the tolerance collision; in each the reference is the restatement of the
    handle's own stored cells."""
    env = {"three": {}, "two": {"LBM3D_THREE": "0"}, "one": {"LBM3D_TWO": "0"}, "tolerance": {}}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    p, obst, c0 = _problem(34, 13, 12, 7)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        for steps in (9, 1):
            e.run_steps(steps)
            _check(e, p, obst, (form, steps))


# --------------------------------------------------------------- 3. boxes ----

BOXES = [
    (17, 4, 3, 1, 1, 1),        # one cell
    (5, 2, 4, 23, 6, 4),        # unaligned x0, across the slab border (planes 4 .. 7 of 0 .. 5 | 6 .. 10)
    (0, 0, 5, 67, 18, 2),       # full planes either side of the slab border
    (64, 0, 0, 3, 18, 11),      # the ragged tail columns through the whole depth
    (0, 0, 0, 67, 18, 11),      # the whole domain
]


@pytest.fixture(scope="module")
def stepped_67x18x11(gpu_lib):
    p, obst, c0 = _problem(67, 18, 11, 5)
    e = gpu_lib.Engine3D(p, obst, parts=2, devices=[0])
    e.load_cells(c0)
    e.run_steps(3)
    assert e.local_slabs() == [(0, 6), (6, 5)]
    ref = _reference(e, p, obst)
    yield e, ref
    e.close()


@pytest.mark.parametrize("box", BOXES)
def test_strain3d_boxes_bitwise(gpu_lib, stepped_67x18x11, box):
    e, ref = stepped_67x18x11
    x0, y0, z0, bx, by, bz = box
    got = e.strain_rate_box(*box)
    _assert_fields(got, ref, gpu_lib.STRESS_FIELDS3D, box, np.s_[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
    if box == BOXES[-1]:
        _assert_fields(e.strain_rate(), got, gpu_lib.STRESS_FIELDS3D, "whole")
    one = e.strain_rate_box(*box, which=("sxz",))
    assert tuple(one) == ("sxz",) and np.array_equal(_b32(one["sxz"]), _b32(got["sxz"]))


# ---------------------------------------------------------- 4. Poiseuille ----

def test_strain3d_poiseuille_on_the_device(gpu_lib):
    """The 4 x 18 x 4 channel of tests/test_stress_host.py, omega 1.25, 12000 steps on the
    device from the rest state: s_xy within 1e-2 of the analytic 1/2 du_x/dy at every fluid
    cell, relative to its value at the wall-adjacent cell (host run: 1.3e-3)."""
    nx, ny, nz = 4, 18, 4
    p = lio.Params3D(nx, ny, nz, 0, 1.0, 1e-5, 1.25)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(oracle.init_cells3d(p))
        e.run_steps(12000)
        sxy = e.strain_rate(("sxy",))["sxy"]
        stats = e.strain_stats()
    nu = (1 / float(np.float32(p.omega)) - 0.5) / 3
    ana = 0.5 * (float(np.float32(p.accel)) / 3) / (2 * nu) * (ny - 1 - 2 * np.arange(ny))
    dev = np.abs(sxy[:, 1:-1, :].astype(np.float64) - ana[None, 1:-1, None]).max() / ana[1]
    print("sxy deviation", dev, "wall cell", sxy[0, 1, 0], "analytic", ana[1])
    assert dev < 1e-2
    assert stats[2] == 2 * nx * nz        # the two planes of fluid cells next to the walls
    # in simple shear strain = sqrt(2) |sxy|: the mean wall strain against the analytic wall cell
    assert abs(stats[3] / stats[2] - np.sqrt(2) * ana[1]) < 1e-2 * np.sqrt(2) * ana[1]


# ------------------------------------------------------------ 5. contract ----

def test_strain3d_contract_and_history(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(33, 9, 8, 43)
    nf = len(n.STRESS_FIELDS3D)
    none = (ctypes.POINTER(ctypes.c_float) * nf)()
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        buf = np.full((p.nz, p.ny, p.nx), -7, np.float32)
        one = (ctypes.POINTER(ctypes.c_float) * nf)()
        one[3] = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        s2 = ctypes.c_double(-1)
        assert L.lbm3d_store_stress(h, one) == n.LBM_E_STATE and (buf == -7).all()
        assert L.lbm3d_stress_stats(h, ctypes.byref(s2), None, None, None, None) == n.LBM_E_STATE and s2.value == -1
        e.load_cells(c0)
        assert L.lbm3d_store_stress(h, none) == n.LBM_OK and L.lbm3d_store_stress(h, None) == n.LBM_OK
        assert L.lbm3d_stress_stats(h, None, None, None, None, None) == n.LBM_OK
        assert L.lbm3d_store_stress(h, one) == n.LBM_OK
        assert np.array_equal(_b32(buf), _b32(_reference(e, p, obst)["sxy"]))
        for bad in ((0, 0, 0, 34, 1, 1), (-1, 0, 0, 2, 2, 2), (0, 0, 7, 1, 1, 2), (0, 0, 0, 0, 1, 1), (0, 9, 0, 1, 1, 1)):
            with pytest.raises(n.LbmError) as ei:
                e.strain_rate_box(*bad)
            assert ei.value.code == n.LBM_E_INVALID, bad
        assert L.lbm3d_store_stress_box(h, None, one) == n.LBM_E_INVALID
        # 7 steps, strain_rate and strain_stats, 6 steps == 13 steps
        e.run_steps(7)
        e.strain_rate()
        e.strain_stats()
        e.run_steps(6)
        cells_a, _ = e.store()
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(13)
        cells_b, _ = e.store()
    assert np.array_equal(_b32(cells_a), _b32(cells_b))
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        samples = e.strain_history(12, every=4)
        with pytest.raises(ValueError):
            e.strain_history(4, 0)
    assert [s[0] for s in samples] == [4, 8, 12]
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        for s in samples:
            e.run_steps(4)
            assert _same_stats(e.strain_stats(), s[1:])


def test_strain3d_refuses_omega_one(gpu_lib):
    n = gpu_lib
    p = lio.Params3D(8, 6, 4, 0, DENSITY, 0.002, 1.0)
    obst = lio.channel_obstacles3d(8, 6, 4)
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(oracle.init_cells3d(p))
        e.run_steps(2)
        for call in (e.strain_rate, e.strain_stats, lambda: e.strain_rate_box(0, 0, 0, 2, 2, 2)):
            with pytest.raises(n.LbmError, match="omega") as ei:
                call()
            assert ei.value.code == n.LBM_E_INVALID
        e.run_steps(2)
        assert np.isfinite(e.store()[0]).all()
