"""Scalar wall models and the per-body wall flux on the device, D3Q19 + D3Q7 (lbm3d_scalar_set_walls,
lbm3d_scalar_wall_flux, lbm3d_scalar_body_flux, lbm3d_scalar_store_wall_flux;
include/lbm_scalar_walls_hip.h, csrc/lbm3d_scalar_walls.hip, csrc/lbm_scalar_walls.hpp).

The bar of tests/test_gpu_scalar_walls.py: every advance with walls set is BITWISE lio.scalar_step3d of the
handle's fields(), then lio.scalar_apply_walls3d, then lio.scalar_apply_fixed3d; the flux map is bitwise
lio.scalar_wall_flux_cells3d of the stored populations, link counts are exact, sums lie within the fold
bound of DESIGN 4.14 of the exact sum; z slabs give the single-slab handle's bits.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import pytest

import walls_cases as wc
from lbm_amd import io as lio
from oracle import oracle
from test_gpu_scalar3d import ADVANCES, CHUNKS, OMEGA_S, _fixed, _problem

pytestmark = pytest.mark.gpu

GRID = (13, 7, 5)
i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
f64p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)


def _P(a, t):
    return a.ctypes.data_as(t)


def _fixed_on_a_wall(p, obst, walls):
    x, y, z, v = _fixed(p, obst)
    labels, kinds, _ = walls
    on = (lio.scalar_wall_links3d(obst) != 0) & (labels >= 0) & \
        (kinds[np.clip(labels, 0, kinds.size - 1)] != lio.WALL_ADIABATIC)
    at = np.argwhere(on)
    wz, wy, wx = [int(c) for c in at[len(at) // 2]]
    if not ((x == wx) & (y == wy) & (z == wz)).any():
        x, y, z, v = np.append(x, wx), np.append(y, wy), np.append(z, wz), np.append(v, 2.5)
    return x.astype(np.int32), y.astype(np.int32), z.astype(np.int32), v.astype(np.float32)


def _check_flux(e, obst, g, walls, what=""):
    labels, kinds, values = walls
    cells = lio.scalar_wall_flux_cells3d(g, obst, labels, kinds, values)
    got = e.scalar_wall_flux_field()
    assert wc.same(got, cells), (what, np.argwhere(wc.b32(got) != wc.b32(cells))[:4].tolist())
    links = lio.scalar_wall_links3d(obst)
    nlinks = np.zeros(links.shape, np.int64)
    for k in range(6):
        nlinks += (links >> np.uint32(k)) & np.uint32(1)
    wall = links != 0
    q, n = e.scalar_wall_flux()
    assert n == int(nlinks.sum()), what
    assert abs(q - math.fsum(cells[wall].astype(np.float64).tolist())) <= wc.fold_bound(cells[wall]), what
    qb, nb = e.scalar_body_flux()
    for b in range(kinds.size):
        sel = wall & (labels == b)
        assert nb[b] == int(nlinks[sel].sum()), (what, b)
        assert abs(qb[b] - math.fsum(cells[sel].astype(np.float64).tolist())) <= wc.fold_bound(cells[sel]), (what, b)
    qb2, nb2 = e.scalar_body_flux()
    assert e.scalar_wall_flux() == (q, n) and np.array_equal(qb2.view(np.uint64), qb.view(np.uint64))
    assert np.array_equal(nb2, nb)
    return cells


def _advance_and_check(e, obst, g, n, walls=None, fixed=None, what=""):
    f = e.fields(("ux", "uy", "uz"))
    for _ in range(n):
        g = lio.scalar_step3d(g, f["ux"], f["uy"], f["uz"], obst, OMEGA_S)
        if walls is not None:
            g = lio.scalar_apply_walls3d(g, obst, *walls)
        if fixed is not None:
            g = lio.scalar_apply_fixed3d(g, *fixed)
    e.scalar_advance(n)
    got = e.scalar(populations=True)[1]
    bad = wc.b32(got) != wc.b32(g)
    assert not bad.any(), (what, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return g


def _sequence(e, p, obst, c0, phi0, walls, fixed=None, what="", chunks=CHUNKS, flux=True):
    e.load_cells(c0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    g = lio.scalar_init3d(phi0)
    if fixed is not None:
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed3d(g, *fixed)
    e.scalar_walls(*walls)
    assert wc.same(e.scalar(populations=True)[1], g), what
    for i, (steps, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(steps)
        g = _advance_and_check(e, obst, g, n, walls, fixed, what)
        if flux and i in (0, len(chunks) - 1):
            _check_flux(e, obst, g, walls, what)
            assert wc.same(e.scalar(populations=True)[1], g), what
    return g


# ------------------------------------------------------------ 1. parity ----

@pytest.mark.parametrize("with_fixed", [False, True])
@pytest.mark.parametrize("form", ["bitwise", "tolerance"])
def test_advance_sequences_bitwise(gpu_lib, form, with_fixed):
    p, obst, c0, phi0 = _problem(*GRID, 7)
    walls = wc.random_bodies(obst, 13)
    fixed = _fixed_on_a_wall(p, obst, walls) if with_fixed else None
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        g = _sequence(e, p, obst, c0, phi0, walls, fixed, (form, with_fixed))
    on = lio.scalar_wall_links3d(obst) != 0
    assert set(walls[1][walls[0][on].clip(0)]) == {0, 1, 2}
    assert np.abs(lio.scalar_phi(g) - phi0).max() > 0.1


@pytest.fixture(scope="module")
def single(gpu_lib):
    p, obst, c0, phi0 = _problem(*GRID, 11)
    walls = wc.random_bodies(obst, 17)
    fixed = _fixed_on_a_wall(p, obst, walls)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        assert len(e.local_slabs()) == 1
        g = _sequence(e, p, obst, c0, phi0, walls, fixed, "single")
        flux = (e.scalar_wall_flux(), e.scalar_body_flux(), e.scalar_wall_flux_field())
    g.setflags(write=False)
    return p, obst, c0, phi0, walls, fixed, g, flux


@pytest.mark.parametrize("parts", [2, 3])
def test_bits_do_not_depend_on_the_slabs(gpu_lib, single, parts):
    p, obst, c0, phi0, walls, fixed, ref, ref_flux = single
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        assert len(e.local_slabs()) == parts
        g = _sequence(e, p, obst, c0, phi0, walls, fixed, parts, flux=False)
        flux = (e.scalar_wall_flux(), e.scalar_body_flux(), e.scalar_wall_flux_field())
    assert wc.same(g, ref) and flux[0] == ref_flux[0] and wc.same(flux[2], ref_flux[2])
    assert np.array_equal(flux[1][0].view(np.uint64), ref_flux[1][0].view(np.uint64))
    assert np.array_equal(flux[1][1], ref_flux[1][1])


# ------------------------------------------------- 2. degenerate shapes ----

@pytest.mark.parametrize("nx,ny,nz", [(1, 5, 4), (3, 2, 2), (2, 1, 1), (1, 1, 1), (6, 5, 1)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny, nz):
    """nx < 4 among them; the links of a blocked cell wrap onto its own line where an extent is 1."""
    p, _, c0, phi0 = _problem(nx, ny, nz, 5 + nx, obstacles=0.0, walls=False)
    obst = np.zeros((nz, ny, nx), np.uint8)
    if obst.size > 1:
        obst[0, 0, 0] = 1
    if obst.size > 4:
        obst[-1, -1, -1] = 1
    labels = np.where(obst != 0, np.arange(obst.size).reshape(obst.shape) % 2, -1).astype(np.int32)
    walls = (labels, np.array([1, 2], np.int32), np.array([1.5, -0.02], np.float32))
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        _sequence(e, p, obst, c0, phi0, walls, None, (nx, ny, nz), chunks=CHUNKS[:3])


def test_empty_lists_and_a_free_standing_cell(gpu_lib):
    p, _, c0, phi0 = _problem(6, 5, 4, 3, obstacles=0.0, walls=False)
    one = (np.zeros((4, 5, 6), np.int32), np.array([1], np.int32), np.array([2.0], np.float32))
    for obst in (np.ones((4, 5, 6), np.uint8), np.zeros((4, 5, 6), np.uint8)):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            _sequence(e, p, obst, c0, phi0, one, None, "empty", chunks=(1, 2))
            assert e.scalar_wall_flux() == (0.0, 0) and not e.scalar_wall_flux_field().any()
            assert e.scalar_body_flux()[0].tolist() == [0.0]
    obst = np.zeros((4, 5, 6), np.uint8)
    obst[2, 2, 3], obst[0, 0, 0], obst[3, 4, 5] = 1, 1, 1      # every link set; two corners linked across the edges
    assert lio.scalar_wall_links3d(obst)[2, 2, 3] == 0b111111 and lio.scalar_wall_links3d(obst)[0, 0, 0] == 0b111111
    walls = (np.where(obst != 0, 0, -1).astype(np.int32), np.array([1], np.int32), np.array([2.0], np.float32))
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        _sequence(e, p, obst, c0, phi0, walls, None, "free-standing", chunks=(1, 2))
        assert e.scalar_wall_flux()[1] == 18 and e.scalar_body_flux()[1].tolist() == [18]


# ---------------------------------------------------------- 3. the sums ----

def test_flux_sums_large_and_small_bodies(gpu_lib):
    """The two channel walls of 40 x 4 x 16 as one body of 2 * 640 wall cells (more than BODY_CHUNK = 512:
    three chunks), one-cell bodies, a body without a cell and unlabelled blocked cells."""
    nx, ny, nz = 40, 4, 16
    p, _, c0, phi0 = _problem(nx, ny, nz, 9, obstacles=0.0, walls=False)
    obst = np.zeros((nz, ny, nx), np.uint8)
    obst[:, 0, :], obst[:, -1, :] = 1, 1
    obst[5, 2, 7], obst[9, 1, 30], obst[12, 2, 20] = 1, 1, 1
    labels = np.full(obst.shape, -1, np.int32)
    labels[:, 0, :], labels[:, -1, :] = 0, 0
    labels[5, 2, 7], labels[9, 1, 30] = 1, 2                  # (12, 2, 20) stays unlabelled
    walls = (labels, np.array([1, 2, 1, 2], np.int32), np.array([1.0, 0.01, -2.0, 0.5], np.float32))
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        e.scalar_walls(*walls)
        e.run_steps(2)
        g = _advance_and_check(e, obst, lio.scalar_init3d(phi0), 2, walls, None, "channel")
        _check_flux(e, obst, g, walls, "channel")
        qb, nb = e.scalar_body_flux()
    # each of the three cells touches a channel wall: five links of its own, and the wall cell behind it has none
    assert nb.tolist() == [2 * 640 - 3, 5, 5, 0] and qb[3] == 0 and abs(qb[0]) > 1


# ---------------------------------- 4. table alone, unchanged state, contract ----

def test_table_only_update_state_and_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0, phi0 = _problem(*GRID, 21)
    labels, kinds, values = wc.random_bodies(obst, 8)
    nb = kinds.size
    kinds2, values2 = np.roll(kinds, 1), (values * np.float32(-0.5)).astype(np.float32)
    q, links = ctypes.c_double(7.0), ctypes.c_int64(7)
    qb, lb, qmap = np.full(nb, 7.0), np.full(nb, 7, np.int64), np.full(obst.shape, 7.0, np.float32)
    got = []
    for table_only in (True, False):
        with n.Engine3D(p, obst, devices=[0]) as e:
            L, h = e._L, e._h
            if table_only:
                calls = (lambda hh: L.lbm3d_scalar_set_walls(hh, _P(labels, i32p), nb, _P(kinds, i32p), _P(values, f32p)),
                         lambda hh: L.lbm3d_scalar_wall_flux(hh, ctypes.byref(q), ctypes.byref(links)),
                         lambda hh: L.lbm3d_scalar_body_flux(hh, _P(qb, f64p), _P(lb, i64p), nb),
                         lambda hh: L.lbm3d_scalar_store_wall_flux(hh, _P(qmap, f32p)))
                for call in calls:
                    assert call(None) == n.LBM_E_INVALID and call(h) == n.LBM_E_STATE      # before scalar_begin
                assert (q.value, links.value) == (7.0, 7) and (qb == 7).all() and (qmap == 7).all()
            e.load_cells(c0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            if table_only:
                assert calls[2](h) == n.LBM_E_STATE                                        # no walls set
                assert L.lbm3d_scalar_set_walls(h, None, nb, _P(kinds, i32p), _P(values, f32p)) == n.LBM_E_INVALID
            e.run_steps(2)
            flow = e.store()[0]
            e.scalar_walls(labels, kinds, values)
            g = _advance_and_check(e, obst, lio.scalar_init3d(phi0), 2, (labels, kinds, values), None, "first table")
            if table_only:
                bad_kind, bad_value, bad_label = kinds.copy(), values.copy(), labels.copy()
                bad_kind[0], bad_value[1] = -1, np.inf
                bad_label[tuple(np.argwhere(obst != 0)[0])] = nb
                for lab, k, v, cnt in ((labels, bad_kind, values, nb), (labels, kinds, bad_value, nb),
                                       (bad_label, kinds, values, nb), (labels, kinds, values, 0)):
                    assert L.lbm3d_scalar_set_walls(h, _P(lab, i32p), cnt, _P(k, i32p), _P(v, f32p)) == n.LBM_E_INVALID
                for cnt in (nb - 1, nb + 1, 0):
                    assert L.lbm3d_scalar_set_walls(h, None, cnt, _P(kinds2, i32p), _P(values2, f32p)) == n.LBM_E_INVALID
                assert L.lbm3d_scalar_body_flux(h, _P(qb, f64p), _P(lb, i64p), nb + 1) == n.LBM_E_STATE
                g = _advance_and_check(e, obst, g, 1, (labels, kinds, values), None, "old walls kept")
                e.scalar_wall_values(kinds2, values2)
            else:
                g = _advance_and_check(e, obst, g, 1, (labels, kinds, values), None, "first table")
                e.scalar_walls(labels, kinds2, values2)
            assert wc.same(e.scalar(populations=True)[1], g) and wc.same(e.store()[0], flow)
            g = _advance_and_check(e, obst, g, 3, (labels, kinds2, values2), None, ("second table", table_only))
            _check_flux(e, obst, g, (labels, kinds2, values2), "second table")
            got.append((g, e.scalar_body_flux()))
            assert wc.same(e.scalar(populations=True)[1], g) and wc.same(e.store()[0], flow)
            if table_only:
                e.scalar_walls(None, 0)                           # cleared: the plain scalar from here on
                g = _advance_and_check(e, obst, g, 2, None, None, "cleared")
                e.scalar_walls(labels, kinds, values)
                e.scalar_begin(phi0, omega_s=OMEGA_S)             # begin drops the walls
                assert L.lbm3d_scalar_body_flux(h, _P(qb, f64p), _P(lb, i64p), nb) == n.LBM_E_STATE
                _advance_and_check(e, obst, lio.scalar_init3d(phi0), 2, None, None, "begin drops the walls")
    assert wc.same(got[0][0], got[1][0]) and np.array_equal(got[0][1][0].view(np.uint64), got[1][1][0].view(np.uint64))


# ------------------------------------------------------------ 5. physics ----

def test_conduction_slot_equals_the_cpu_loop(gpu_lib):
    """The 3-D slot of tests/test_scalar_walls_host.py (along z) on the device: its first 50 steps equal the
    numpy loop bit for bit, and wall_flux_history returns what separate scalar_body_flux calls return."""
    obst, labels, kinds, values, phi0 = wc.slot(3)
    nz, ny, nx = obst.shape
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.0, 1.85)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e, gpu_lib.Engine3D(p, obst, devices=[0]) as e2:
        for h in (e, e2):
            h.load_cells(oracle.init_cells3d(p))
            h.scalar_begin(phi0, omega_s=1.0)
            h.scalar_walls(labels, kinds, values)
        g, flux, at = lio.scalar_init3d(phi0), [], []
        for step in range(50):
            e.run_steps(1)
            f = e.fields(("ux", "uy", "uz"))
            assert max(np.abs(f[c]).max() for c in f) < 1e-6                  # the flow rests
            g = wc.advance(g, obst, labels, kinds, values, 1.0, 1, u=(f["ux"], f["uy"], f["uz"]))
            e.scalar_advance(1)
            assert wc.same(e.scalar(populations=True)[1], g), step
            if step % 10 == 9:
                flux.append(e.scalar_body_flux()[0])
                at.append(step + 1)
        hist = e2.wall_flux_history(50, 10)
        assert hist["step"].tolist() == at and hist["links"].tolist() == [wc.WIDTH ** 2] * 2
        assert np.array_equal(hist["q"].view(np.uint64), np.stack(flux).view(np.uint64))
        assert flux[-1][0] > 0 > flux[-1][1] and flux[0][0] > flux[-1][0]
