"""Vorticity, divergence, strain rate and Q derived on the device, D3Q19
(lbm3d_store_gradients / _box / lbm3d_gradient_stats;
include/lbm_gradients_hip.h, csrc/lbm3d_gradients.hip).

Bar: every field is BITWISE (uint32 patterns) lio.velocity_gradients3d of the
same handle's fields() (the restatement pinned in tests/test_gradients_host.py)
in both numerics modes, on both lattices of the pair, on 1, 2 and 4 z slabs
down to one plane per slab, and for boxes of one cell, with an unaligned x
origin, touching each periodic face, and spanning two slabs.  Statistics as in
tests/test_gpu_gradients.py.  Inputs follow tests/test_gpu_fields3d.py's recipe
with about 10 % obstacles.
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

VEL = ("ux", "uy", "uz")


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _d64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, accel=0.002):
    p = lio.Params3D(nx, ny, nz, 0, 0.1, accel, 1.7)
    rng = np.random.default_rng(seed)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    obst[rng.random((nz, ny, nx)) < 0.1] = 1
    obst[0, ny // 2, 0] = obst[nz - 1, ny // 2, nx - 1] = 1      # on the periodic faces
    obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.02 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _reference(e, obst):
    f = e.fields(VEL)
    return lio.velocity_gradients3d(f["ux"], f["uy"], f["uz"], obst)


def _assert_fields(got, ref, names, what="", cut=None):
    for name in names:
        r = ref[name] if cut is None else ref[name][cut]
        assert got[name].dtype == np.float32 and got[name].shape == r.shape, (what, name, got[name].shape, r.shape)
        bad = _b32(got[name]) != _b32(r)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _assert_stats(stats, ref, obst, what=""):
    w2, s2, mw, md = stats
    rw2, rs2, rmw, rmd = lio.gradient_stats(ref, obst)
    n = int((np.asarray(obst) == 0).sum())
    assert _b32(np.float32(mw)) == _b32(rmw) and _b32(np.float32(md)) == _b32(rmd), (what, mw, rmw, md, rmd)
    bound = 2 * max(n - 1, 0) * 2.0 ** -53
    print(what, "sum_w2", w2, rw2, "sum_s2", s2, rs2, "bound", bound)
    assert abs(w2 - rw2) <= bound * rw2, (what, w2, rw2)
    assert abs(s2 - rs2) <= bound * rs2, (what, s2, rs2)


def _check(e, obst, what=""):
    ref = _reference(e, obst)
    got = e.gradients()
    assert tuple(got) == e._GRAD_FIELDS
    _assert_fields(got, ref, e._GRAD_FIELDS, what)
    stats = e.gradient_stats()
    _assert_stats(stats, ref, obst, what)
    again = e.gradient_stats()
    assert [_d64(v) for v in stats[:2]] == [_d64(v) for v in again[:2]] and stats[2:] == again[2:], what
    ob = np.asarray(obst) != 0
    for name in e._GRAD_FIELDS:
        assert not _b32(got[name])[ob].any(), (what, name)
    return ref, got, stats


# ------------------------------------------------- 1. shapes and numerics ----

@pytest.mark.parametrize("mode", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", [(5, 6, 7), (33, 9, 4), (64, 12, 8), (67, 18, 35), (3, 5, 4)])
def test_gradients3d_shapes_bitwise(gpu_lib, nx, ny, nz, mode):
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if mode == "tolerance" else 0)
    p, obst, c0 = _problem(nx, ny, nz, nx + ny + nz)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        _check(e, obst, (nx, ny, nz, mode, "loaded"))
        e.run_steps(3)
        _, got, _ = _check(e, obst, (nx, ny, nz, mode, 3))
        e.run_steps(1)
        _check(e, obst, (nx, ny, nz, mode, 4))
        assert tuple(e.gradients(("q", "wx"))) == ("q", "wx")
    if min(nx, ny, nz) > 2:
        assert got["vorticity"].any() and got["strain"].any()


# --------------------------------------------------------------- 2. slabs ----

@pytest.fixture(scope="module")
def single_33x9x4(gpu_lib):
    p, obst, c0 = _problem(33, 9, 4, 41)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(5)
        ref, got, stats = _check(e, obst, "single")
    for a in got.values():
        a.setflags(write=False)
    return p, obst, c0, got, stats


@pytest.mark.parametrize("parts", [2, 4])
def test_gradients3d_slabs_bitwise(gpu_lib, single_33x9x4, parts):
    """4 slabs of a 4-plane domain: one plane each, both z neighbours from other slabs."""
    p, obst, c0, ref, ref_stats = single_33x9x4
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(5)
        assert len(e.local_slabs()) == parts
        got = e.gradients()
        stats = e.gradient_stats()
        assert stats == e.gradient_stats()
        box = e.gradients_box(2, 1, 1, 30, 7, 2)            # spans two slabs (parts = 2: planes 1 | 2)
    _assert_fields(got, ref, gpu_lib.GRAD_FIELDS3D, parts)
    _assert_fields(box, ref, gpu_lib.GRAD_FIELDS3D, (parts, "box"), np.s_[1:3, 1:8, 2:32])
    n = int((obst == 0).sum())
    bound = 2 * (n - 1) * 2.0 ** -53
    assert stats[2:] == ref_stats[2:]
    for a, b in zip(stats[:2], ref_stats[:2]):
        assert abs(a - b) <= bound * b, (parts, a, b)


def test_gradients3d_rccl_world_1(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(33, 9, 4, 41)
    with n.Engine3D(p, obst, devices=[0], transport=n.TRANSPORT_RCCL, rank=0, world=1,
                    unique_id=n.rccl_unique_id()) as e:
        e.load_cells(c0)
        e.run_steps(5)
        _check(e, obst, "rccl1")


# --------------------------------------------------------------- 3. boxes ----

BOXES = [
    (17, 4, 3, 1, 1, 1),        # one cell
    (5, 2, 1, 23, 6, 7),        # unaligned x0
    (0, 0, 0, 4, 3, 2),         # touching the low face of every axis: the stencil wraps
    (60, 10, 8, 7, 8, 3),       # touching the high faces (67 x 18 x 11)
    (0, 5, 2, 67, 1, 1),        # a full row
    (64, 0, 0, 3, 18, 11),      # the ragged tail columns through the whole depth
    (0, 0, 0, 67, 18, 11),      # the whole domain
]


@pytest.fixture(scope="module")
def stepped_67x18x11(gpu_lib):
    p, obst, c0 = _problem(67, 18, 11, 5)
    e = gpu_lib.Engine3D(p, obst, parts=2, devices=[0])
    e.load_cells(c0)
    e.run_steps(3)
    ref = _reference(e, obst)
    yield e, ref
    e.close()


@pytest.mark.parametrize("box", BOXES)
def test_gradients3d_boxes_bitwise(gpu_lib, stepped_67x18x11, box):
    e, ref = stepped_67x18x11
    x0, y0, z0, bx, by, bz = box
    got = e.gradients_box(*box)
    _assert_fields(got, ref, gpu_lib.GRAD_FIELDS3D, box, np.s_[z0:z0 + bz, y0:y0 + by, x0:x0 + bx])
    if box == BOXES[-1]:
        _assert_fields(e.gradients(), got, gpu_lib.GRAD_FIELDS3D, "whole")
    one = e.gradients_box(*box, which=("strain",))
    assert tuple(one) == ("strain",) and np.array_equal(_b32(one["strain"]), _b32(got["strain"]))


# ------------------------------------------------------------ 4. contract ----

def test_gradients3d_contract_and_history(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(33, 9, 8, 43)
    nf = len(n.GRAD_FIELDS3D)
    none = (ctypes.POINTER(ctypes.c_float) * nf)()
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        buf = np.zeros((p.nz, p.ny, p.nx), np.float32)
        one = (ctypes.POINTER(ctypes.c_float) * nf)()
        one[3] = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        w2 = ctypes.c_double(-1)
        assert L.lbm3d_store_gradients(h, one) == n.LBM_E_STATE
        assert L.lbm3d_gradient_stats(h, ctypes.byref(w2), None, None, None) == n.LBM_E_STATE and w2.value == -1
        e.load_cells(c0)
        assert L.lbm3d_store_gradients(h, none) == n.LBM_OK and L.lbm3d_store_gradients(h, None) == n.LBM_OK
        assert L.lbm3d_gradient_stats(h, None, None, None, None) == n.LBM_OK
        for bad in ((0, 0, 0, 34, 1, 1), (-1, 0, 0, 2, 2, 2), (0, 0, 7, 1, 1, 2), (0, 0, 0, 0, 1, 1), (0, 9, 0, 1, 1, 1)):
            with pytest.raises(n.LbmError) as ei:
                e.gradients_box(*bad)
            assert ei.value.code == n.LBM_E_INVALID, bad
        assert L.lbm3d_store_gradients_box(h, None, one) == n.LBM_E_INVALID
        # 7 steps, gradients, 6 steps == 13 steps
        e.run_steps(7)
        e.gradients()
        e.gradient_stats()
        e.run_steps(6)
        cells_a, _ = e.store()
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(13)
        cells_b, _ = e.store()
    assert np.array_equal(_b32(cells_a), _b32(cells_b))
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        samples = e.gradient_history(12, every=4)
        with pytest.raises(ValueError):
            e.gradient_history(4, 0)
    assert [s[0] for s in samples] == [4, 8, 12]
    with n.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        for s in samples:
            e.run_steps(4)
            hand = e.gradient_stats()
            assert [_d64(v) for v in hand[:2]] == [_d64(v) for v in s[1:3]] and hand[2:] == s[3:]
