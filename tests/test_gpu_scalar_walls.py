"""Scalar wall models and the per-body wall flux on the device, D2Q9 + D2Q5 (lbm_scalar_set_walls,
lbm_scalar_wall_flux, lbm_scalar_body_flux, lbm_scalar_store_wall_flux; include/lbm_scalar_walls_hip.h,
csrc/lbm_scalar_walls.hip, csrc/lbm_scalar_walls.hpp).

Bar: after every scalar_advance with walls set the populations are BITWISE (uint32 patterns)
lio.scalar_step of the handle's fields(), then lio.scalar_apply_walls, then lio.scalar_apply_fixed -- the
numpy restatement of the header, pinned by physics in tests/test_scalar_walls_host.py -- over the
flow-chunk and advance sequences of tests/test_gpu_scalar.py, with and without a fixed list that shares a
cell with the wall list, for several flow kernels and both numerics, decomposed handles (whose bits are
the single-domain handle's) and degenerate shapes.  The per-cell flux map equals
lio.scalar_wall_flux_cells of the stored populations bit for bit, link counts are exact, and totals and
per-body sums lie within the fold bound of DESIGN 4.14, 2 (n - 1) 2^-53 sum|term|, of the exact sum.
No other tolerance anywhere.
"""
from __future__ import annotations

import ctypes
import math
import subprocess

import numpy as np
import pytest

import walls_cases as wc
from conftest import GOLD, PKG
from lbm_amd import io as lio
from test_gpu_scalar import ADVANCES, CHUNKS, GRIDS, OMEGA_S, _fixed, _problem

pytestmark = pytest.mark.gpu

i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
f64p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)


def _P(a, t):
    return a.ctypes.data_as(t)


def _fixed_on_a_wall(p, obst, walls):
    """The fixed list of tests/test_gpu_scalar.py plus a wall cell of a body with a wall model."""
    x, y, v = _fixed(p, obst)
    labels, kinds, _ = walls
    on = (lio.scalar_wall_links(obst) != 0) & (labels >= 0) & (kinds[np.clip(labels, 0, kinds.size - 1)] != lio.WALL_ADIABATIC)
    wy, wx = [int(c) for c in np.argwhere(on)[len(np.argwhere(on)) // 2]]
    if not ((x == wx) & (y == wy)).any():
        x, y, v = np.append(x, np.int32(wx)), np.append(y, np.int32(wy)), np.append(v, np.float32(2.5))
    return x.astype(np.int32), y.astype(np.int32), v.astype(np.float32)


def _check_flux(e, obst, g, walls, what=""):
    """The three samples of the handle against the restatement of the stored populations g."""
    labels, kinds, values = walls
    cells = lio.scalar_wall_flux_cells(g, obst, labels, kinds, values)
    got = e.scalar_wall_flux_field()
    assert wc.same(got, cells), (what, np.argwhere(wc.b32(got) != wc.b32(cells))[:4].tolist())
    links = lio.scalar_wall_links(obst)
    nlinks = np.zeros(links.shape, np.int64)
    for k in range(4):
        nlinks += (links >> np.uint32(k)) & np.uint32(1)
    q, n = e.scalar_wall_flux()
    wall = links != 0
    assert n == int(nlinks.sum()), what
    assert abs(q - math.fsum(cells[wall].astype(np.float64).tolist())) <= wc.fold_bound(cells[wall]), what
    qb, nb = e.scalar_body_flux()
    assert qb.shape == nb.shape == kinds.shape
    for b in range(kinds.size):
        sel = wall & (labels == b)
        assert nb[b] == int(nlinks[sel].sum()), (what, b)
        assert abs(qb[b] - math.fsum(cells[sel].astype(np.float64).tolist())) <= wc.fold_bound(cells[sel]), (what, b)
    q2, n2 = e.scalar_wall_flux()
    qb2, nb2 = e.scalar_body_flux()
    assert (q2, n2) == (q, n) and np.array_equal(qb2.view(np.uint64), qb.view(np.uint64)) and np.array_equal(nb2, nb)
    return cells


def _advance_and_check(e, obst, g, n, walls=None, fixed=None, what=""):
    f = e.fields(("ux", "uy"))
    for _ in range(n):
        g = lio.scalar_step(g, f["ux"], f["uy"], obst, OMEGA_S)
        if walls is not None:
            g = lio.scalar_apply_walls(g, obst, *walls)
        if fixed is not None:
            g = lio.scalar_apply_fixed(g, *fixed)
    e.scalar_advance(n)
    got = e.scalar(populations=True)[1]
    bad = wc.b32(got) != wc.b32(g)
    assert not bad.any(), (what, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return g


def _sequence(e, p, obst, cells0, phi0, walls, fixed=None, what="", chunks=CHUNKS, flux=True):
    e.load_cells(cells0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    g = lio.scalar_init(phi0)
    if fixed is not None:
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed(g, *fixed)
    e.scalar_walls(*walls)
    assert wc.same(e.scalar(populations=True)[1], g), what           # setting the walls applies nothing
    for i, (steps, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(steps, accelerate_first=i == 0)
        g = _advance_and_check(e, obst, g, n, walls, fixed, what)
        if flux and i in (0, len(chunks) - 1):
            _check_flux(e, obst, g, walls, what)
            assert wc.same(e.scalar(populations=True)[1], g), what   # a sample changes no bit
    return g


# ------------------------------------------------------------ 1. parity ----

@pytest.mark.parametrize("with_fixed", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_advance_sequences_bitwise(gpu_lib, nx, ny, with_fixed):
    p, obst, cells0, phi0 = _problem(nx, ny, 100 * nx + ny)
    walls = wc.random_bodies(obst, nx)
    fixed = _fixed_on_a_wall(p, obst, walls) if with_fixed else None
    with gpu_lib.Engine(p, obst) as e:
        g = _sequence(e, p, obst, cells0, phi0, walls, fixed, (nx, ny, with_fixed))
    plain = lio.scalar_init(phi0)
    assert set(walls[1][walls[0][lio.scalar_wall_links(obst) != 0].clip(0)]) == {0, 1, 2}
    assert np.abs(lio.scalar_phi(g) - lio.scalar_phi(plain)).max() > 0.1         # the walls acted


@pytest.mark.parametrize("mode", ["stream", "stream_tolerance", "step2", "pipeline"])
def test_advance_flow_kernels_and_numerics_bitwise(gpu_lib, mode):
    n = gpu_lib
    kw = {"stream": dict(kernel=n.KERNEL_STREAM), "stream_tolerance": dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE),
          "step2": dict(kernel=n.KERNEL_STEP2), "pipeline": dict(kernel=n.KERNEL_PIPELINE)}[mode]
    p, obst, cells0, phi0 = _problem(132, 70, 7)
    walls = wc.random_bodies(obst, 70)
    with n.Engine(p, obst, **kw) as e:
        _sequence(e, p, obst, cells0, phi0, walls, _fixed_on_a_wall(p, obst, walls), mode, chunks=CHUNKS[:3], flux=False)
        assert e.kernel_in_use() == mode.split("_")[0]
        assert e.numerics() == ("tolerance" if mode == "stream_tolerance" else "bitwise")


# ------------------------------------------------------ 2. decomposed ----

@pytest.fixture(scope="module")
def single(gpu_lib):
    """{grid: ...} of the single-domain handles after the sequence: the reference of the decomposed cases,
    computed once and left unchanged."""
    out = {}
    for nx, ny in GRIDS:
        p, obst, cells0, phi0 = _problem(nx, ny, 31 + nx)
        walls = wc.random_bodies(obst, 5 + nx)
        fixed = _fixed_on_a_wall(p, obst, walls)
        with gpu_lib.Engine(p, obst, parts=1) as e:
            g = _sequence(e, p, obst, cells0, phi0, walls, fixed, "single")
            flux = (e.scalar_wall_flux(), e.scalar_body_flux(), e.scalar_wall_flux_field())
        for a in (obst, cells0, phi0, g) + fixed + walls:
            a.setflags(write=False)
        out[(nx, ny)] = (p, obst, cells0, phi0, walls, fixed, g, flux)
    return out


@pytest.mark.parametrize("grid", [(1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_bits_do_not_depend_on_the_decomposition(gpu_lib, single, nx, ny, grid):
    p, obst, cells0, phi0, walls, fixed, ref, ref_flux = single[(nx, ny)]
    with gpu_lib.Engine(p, obst, parts=grid[0] * grid[1], grid=grid, devices=[0]) as e:
        assert len(e.local_rects()) == grid[0] * grid[1]
        g = _sequence(e, p, obst, cells0, phi0, walls, fixed, (nx, ny, grid), flux=False)
        flux = (e.scalar_wall_flux(), e.scalar_body_flux(), e.scalar_wall_flux_field())
    assert wc.same(g, ref)
    # one list over the whole domain, whatever the sub-domains: the sums have the same bits too
    assert flux[0] == ref_flux[0] and wc.same(flux[2], ref_flux[2])
    assert np.array_equal(flux[1][0].view(np.uint64), ref_flux[1][0].view(np.uint64))
    assert np.array_equal(flux[1][1], ref_flux[1][1])


# ------------------------------------------------- 3. degenerate shapes ----

@pytest.mark.parametrize("nx,ny", [(1, 8), (8, 1), (1, 1), (2, 1), (5, 3)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny):
    p, obst, cells0, phi0 = _problem(nx, ny, 5 + nx + 10 * ny, obstacles=0.0)
    obst = obst.copy()
    if nx * ny > 1:
        obst[0, 0] = 1                       # in a one-cell-wide domain its links wrap onto the same line
    if nx * ny > 4:
        obst[ny - 1, nx - 1] = 1
    labels = np.where(obst != 0, np.arange(nx * ny).reshape(ny, nx) % 2, -1).astype(np.int32)
    walls = (labels, np.array([1, 2], np.int32), np.array([1.5, -0.02], np.float32))
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, walls, None, (nx, ny))


def test_empty_lists_launch_nothing(gpu_lib):
    """An all-obstacle grid and an obstacle-free grid have no wall cell: no link, no launch of the pass or of
    a sample, zeros out."""
    n = gpu_lib
    p, _, cells0, phi0 = _problem(13, 6, 2)
    for obst in (np.ones((6, 13), np.uint8), np.zeros((6, 13), np.uint8)):
        walls = (np.zeros((6, 13), np.int32), np.array([1], np.int32), np.array([2.0], np.float32))
        with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
            g = _sequence(e, p, obst, cells0, phi0, walls, None, "empty", chunks=(1, 2))
            assert e.scalar_wall_flux() == (0.0, 0) and not e.scalar_wall_flux_field().any()
            qb, nb = e.scalar_body_flux()
            assert qb.tolist() == [0.0] and nb.tolist() == [0]
            assert not [k for k in e.profile_summary() if "scalar_wall" in k["name"]]
        assert wc.same(lio.scalar_apply_walls(g, obst, *walls), g)


def test_links_across_the_periodic_edge_and_a_free_standing_cell(gpu_lib):
    p, _, cells0, phi0 = _problem(9, 6, 4)
    obst = np.zeros((6, 9), np.uint8)
    obst[0, 0], obst[5, 8], obst[3, 4] = 1, 1, 1       # two corner cells linked across both edges; one with 4 links
    obst[2, 8], obst[2, 0] = 1, 1                      # neighbours across the x edge: no link between them
    links = lio.scalar_wall_links(obst)
    assert links[3, 4] == 0b1111 and links[0, 0] == 0b1111 and links[2, 8] == 0b1110 and links[2, 0] == 0b1011
    labels = np.where(obst != 0, np.arange(54).reshape(6, 9) % 3, -1).astype(np.int32)
    walls = (labels, np.array([1, 2, 1], np.int32), np.array([2.0, 0.03, -1.0], np.float32))
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, walls, None, "edges")


# ---------------------------------------------------------- 4. the sums ----

def test_flux_sums_large_and_small_bodies(gpu_lib):
    """The two walls of a 300 x 70 channel as one body of 600 wall cells (more than BODY_CHUNK = 512: several
    chunks, the second launch), one-cell bodies, a body whose only cell is enclosed (no wall cell), a body
    without any cell, and unlabelled blocked cells."""
    nx, ny = 300, 70
    p, obst, cells0, phi0 = _problem(nx, ny, 9, obstacles=0.0)
    obst = obst.copy()
    obst[0], obst[-1] = 1, 1
    obst[30:33, 100:103] = 1                           # a block: its centre is enclosed
    singles = [(10, 20), (11, 50), (40, 250), (41, 251)]
    for y, x in singles:
        obst[y, x] = 1
    obst[20, 200:205] = 1                              # unlabelled
    labels = np.full((ny, nx), -1, np.int32)
    labels[0], labels[-1] = 0, 0
    labels[30:33, 100:103] = 1
    labels[31, 101] = 2                                # the enclosed cell
    for i, (y, x) in enumerate(singles):
        labels[y, x] = 3 + i
    kinds = np.array([1, 2, 1, 1, 2, 0, 1, 2], np.int32)      # body 7 has no cell
    values = np.array([1.0, 0.01, 9.0, -0.5, 0.02, 4.0, 2.0, 0.5], np.float32)
    walls = (labels, kinds, values)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        e.scalar_walls(*walls)
        e.run_steps(3, accelerate_first=True)
        g = _advance_and_check(e, obst, lio.scalar_init(phi0), 2, walls, None, "channel")
        cells = _check_flux(e, obst, g, walls, "channel")
        qb, nb = e.scalar_body_flux()
    assert nb.tolist() == [600, 12, 0, 4, 4, 4, 4, 0] and qb[2] == 0 and qb[7] == 0 and qb[5] == 0
    assert qb[4] == pytest.approx(0.08, rel=1e-6) and abs(qb[0]) > 1 and cells[31, 101] == 0
    print("channel: body sums", qb.tolist())


# --------------------------------------------------- 5. the table alone ----

def test_table_only_update_equals_a_rebuild(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 21)
    labels, kinds, values = wc.random_bodies(obst, 8)
    kinds2, values2 = np.roll(kinds, 1), (values * np.float32(-0.5)).astype(np.float32)
    got = []
    for table_only in (True, False):
        with n.Engine(p, obst) as e:
            L, h = e._L, e._h
            e.load_cells(cells0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            if table_only:        # NULL labels before any walls are set: there is no list to keep
                assert L.lbm_scalar_set_walls(h, None, kinds.size, _P(kinds, i32p), _P(values, f32p)) == n.LBM_E_INVALID
            e.scalar_walls(labels, kinds, values)
            e.run_steps(3, accelerate_first=True)
            g = _advance_and_check(e, obst, lio.scalar_init(phi0), 2, (labels, kinds, values), None, "first table")
            if table_only:
                # the NULL-labels path takes the count of the list it keeps, and nothing else
                for nb in (kinds.size - 1, kinds.size + 1, 0):
                    assert L.lbm_scalar_set_walls(h, None, nb, _P(kinds2, i32p), _P(values2, f32p)) == n.LBM_E_INVALID
                assert L.lbm_scalar_set_walls(h, None, kinds.size, None, _P(values2, f32p)) == n.LBM_E_INVALID
                e.scalar_wall_values(kinds2, values2)
            else:
                e.scalar_walls(labels, kinds2, values2)
            assert wc.same(e.scalar(populations=True)[1], g)
            g = _advance_and_check(e, obst, g, 3, (labels, kinds2, values2), None, ("second table", table_only))
            _check_flux(e, obst, g, (labels, kinds2, values2), "second table")
            got.append((g, e.scalar_body_flux()))
    assert wc.same(got[0][0], got[1][0]) and np.array_equal(got[0][1][0].view(np.uint64), got[1][1][0].view(np.uint64))


# ------------------------------------------------- 6. unchanged state ----

def test_walls_and_samples_change_no_state(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(64, 32, 12)
    walls = wc.random_bodies(obst, 3)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e, n.Engine(p, obst, flags=n.FLAG_PROFILE) as never:
        for h in (e, never):
            h.load_cells(cells0)
            h.scalar_begin(phi0, omega_s=OMEGA_S)
            h.run_scalar(4, 1, accelerate_first=True)
        flow, g = e.store()[0], e.scalar(populations=True)[1]
        e.scalar_walls(*walls)
        e.scalar_wall_flux(), e.scalar_body_flux(), e.scalar_wall_flux_field()
        assert wc.same(e.store()[0], flow) and wc.same(e.scalar(populations=True)[1], g)
        assert not [k for k in e.profile_summary() if k["name"] == "scalar_walls"]
        e.run_scalar(3, 1)
        names = {k["name"]: k["launches"] for k in e.profile_summary()}
        assert names["scalar_walls"] == 3 and names["scalar_wall_flux"] == 1 and names["scalar_wall_flux map"] == 1
        assert names["scalar_wall_flux bodies"] == 1
        assert wc.same(e.store()[0], flow) is False
        # cleared in mid-run: the next advances are those of the plain scalar
        e.scalar_walls(None, 0)
        _advance_and_check(e, obst, e.scalar(populations=True)[1], 2, None, None, "cleared")
        # and from one state on, a handle whose walls were set and cleared runs as one that never had any
        cells, phi = never.store()[0], never.scalar()
        for h in (e, never):
            h.load_cells(cells)
            h.scalar_begin(phi, omega_s=OMEGA_S)
        e.scalar_walls(*walls)
        e.scalar_walls(None, 0)
        for h in (e, never):
            h.run_scalar(5, 1)
        assert wc.same(e.scalar(populations=True)[1], never.scalar(populations=True)[1])
        assert wc.same(e.store()[0], never.store()[0])
        assert e.scalar_wall_flux() == (0.0, 0)
        assert not [k for k in never.profile_summary() if "scalar_wall" in k["name"]]


# ---------------------------------------------------------- 7. contract ----

def test_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 9)
    labels, kinds, values = wc.random_bodies(obst, 9)
    nb = kinds.size
    q, links = ctypes.c_double(7.0), ctypes.c_int64(7)
    qb, lb, qmap = np.full(nb, 7.0), np.full(nb, 7, np.int64), np.full((p.ny, p.nx), 7.0, np.float32)
    with n.Engine(p, obst) as e:
        L, h = e._L, e._h
        set_walls = lambda lab, k, v, cnt=nb: L.lbm_scalar_set_walls(h, _P(lab, i32p), cnt, _P(k, i32p), _P(v, f32p))  # noqa: E731
        calls = (lambda hh: L.lbm_scalar_set_walls(hh, _P(labels, i32p), nb, _P(kinds, i32p), _P(values, f32p)),
                 lambda hh: L.lbm_scalar_wall_flux(hh, ctypes.byref(q), ctypes.byref(links)),
                 lambda hh: L.lbm_scalar_body_flux(hh, _P(qb, f64p), _P(lb, i64p), nb),
                 lambda hh: L.lbm_scalar_store_wall_flux(hh, _P(qmap, f32p)))
        for call in calls:
            assert call(None) == n.LBM_E_INVALID and call(h) == n.LBM_E_STATE          # before scalar_begin
        assert (q.value, links.value) == (7.0, 7) and (qb == 7).all() and (qmap == 7).all()
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert calls[2](h) == n.LBM_E_STATE                                            # no walls set
        assert calls[1](h) == n.LBM_OK and (q.value, links.value) == (0.0, 0)
        e.scalar_walls(labels, kinds, values)
        e.run_steps(2, accelerate_first=True)
        g = _advance_and_check(e, obst, lio.scalar_init(phi0), 1, (labels, kinds, values), None, "set")
        # refused: the old walls stay
        bad_kind, bad_value, bad_label = kinds.copy(), values.copy(), labels.copy()
        bad_kind[0], bad_value[1] = 3, np.nan
        bad_label[np.argwhere(obst != 0)[0][0], np.argwhere(obst != 0)[0][1]] = nb
        assert set_walls(labels, bad_kind, values) == n.LBM_E_INVALID
        assert set_walls(labels, kinds, bad_value) == n.LBM_E_INVALID
        assert set_walls(bad_label, kinds, values) == n.LBM_E_INVALID and b"nbodies" in L.lbm_last_error(h)
        assert set_walls(labels, kinds, values, 0) == n.LBM_E_INVALID
        assert L.lbm_scalar_set_walls(h, _P(labels, i32p), nb, None, _P(values, f32p)) == n.LBM_E_INVALID
        assert L.lbm_scalar_set_walls(h, None, 0, _P(kinds, i32p), None) == n.LBM_E_INVALID
        assert L.lbm_scalar_body_flux(h, _P(qb, f64p), _P(lb, i64p), nb + 1) == n.LBM_E_STATE
        assert wc.same(e.scalar(populations=True)[1], g)
        g = _advance_and_check(e, obst, g, 2, (labels, kinds, values), None, "old walls kept")
        _check_flux(e, obst, g, (labels, kinds, values), "old walls kept")
        # a fixed cell on a wall cell is legal and wins
        fixed = _fixed_on_a_wall(p, obst, (labels, kinds, values))
        e.scalar_fix(*fixed)
        g = _advance_and_check(e, obst, lio.scalar_apply_fixed(g, *fixed), 1, (labels, kinds, values), fixed, "fixed wins")
        # scalar_begin drops the walls
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert calls[2](h) == n.LBM_E_STATE
        _advance_and_check(e, obst, lio.scalar_init(phi0), 2, None, None, "begin drops the walls")
        e.scalar_walls(labels, kinds, values)
        e.scalar_end()
        assert calls[1](h) == n.LBM_E_STATE
        with pytest.raises(ValueError):
            e.scalar_walls(labels[:-1], kinds, values)
        with pytest.raises(ValueError):
            e.scalar_wall_values(kinds, values[:-1])


# ------------------------------------------------ 8. physics, history, CLI ----

def test_conduction_slot_equals_the_cpu_loop(gpu_lib):
    """The slot of tests/test_scalar_walls_host.py on the device: its first 50 steps equal the numpy loop bit
    for bit (the flow rests), and wall_flux_history returns what separate scalar_body_flux calls return."""
    obst, labels, kinds, values, phi0 = wc.slot(2)
    ny, nx = obst.shape
    p = lio.Params(nx, ny, 8, 10, 0.1, 0.0, 1.85)
    with gpu_lib.Engine(p, obst) as e, gpu_lib.Engine(p, obst) as e2:
        for h in (e, e2):
            h.load_cells(lio.init_cells(p))
            h.scalar_begin(phi0, omega_s=1.0)
            h.scalar_walls(labels, ("value", "value"), values)
        g, flux, at = lio.scalar_init(phi0), [], []
        for step in range(50):
            e.run_steps(1)
            f = e.fields(("ux", "uy"))
            assert np.abs(f["ux"]).max() < 1e-6 and np.abs(f["uy"]).max() < 1e-6       # the flow rests
            g = wc.advance(g, obst, labels, kinds, values, 1.0, 1, u=(f["ux"], f["uy"]))
            e.scalar_advance(1)
            assert wc.same(e.scalar(populations=True)[1], g), step
            if step % 10 == 9:
                flux.append(e.scalar_body_flux()[0])
                at.append(step + 1)
                want = lio.scalar_wall_flux(g, obst, labels, kinds, values)[1][0]
                assert np.abs(flux[-1] - want).max() <= wc.fold_bound(np.full(wc.WIDTH, np.abs(want).max()))
        hist = e2.wall_flux_history(50, 10)
        assert hist["step"].tolist() == at and hist["links"].tolist() == [wc.WIDTH, wc.WIDTH]
        assert np.array_equal(hist["q"].view(np.uint64), np.stack(flux).view(np.uint64))
        assert flux[-1][0] > 0 > flux[-1][1] and flux[0][0] > flux[-1][0]      # the hot wall heats, ever less


def test_runner_scalar_walls_option(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "17"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    labels, nb = lio.label_bodies(obst)
    assert nb >= 1
    kinds = (np.arange(nb) % 3 + 1) % 3                     # body 0: value, 1: flux, 2: adiabatic, ...
    values = np.where(kinds == 2, 0.01, 2.0).astype(np.float32) * (1 + np.arange(nb, dtype=np.float32))
    listed = [b for b in range(nb) if kinds[b] != 0]
    (tmp_path / "walls.txt").write_text("".join(f"{b} {kinds[b]} {float(values[b])!r}\n" for b in listed))
    (tmp_path / "dye.txt").write_text("5 5 1.0\n")
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file)]
    scalar = ["--scalar", str(tmp_path / "dye.txt"), "--scalar-omega", "1.3"]
    r = subprocess.run(base + scalar + ["--scalar-walls", str(tmp_path / "walls.txt"), "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got_kind, got_value, got_q, got_links = lio.read_wall_flux(str(tmp_path / "wall_flux.dat"))
    values = np.where(kinds == 0, 0, values).astype(np.float32)
    phi0 = np.zeros((p.ny, p.nx), np.float32)
    phi0[5, 5] = 1.0
    with gpu_lib.Engine(p, obst) as e:                       # the same coupled run through the binding
        e.load_cells(lio.init_cells(p))
        e.scalar_begin(phi0, omega_s=1.3)
        e.scalar_walls(labels, kinds, values)
        e.run_scalar(17, 1, accelerate_first=True)
        q, links = e.scalar_body_flux()
    assert np.array_equal(got_kind, kinds) and wc.same(got_value, values) and np.array_equal(got_links, links)
    assert np.array_equal(got_q.view(np.uint64), q.view(np.uint64)) and np.abs(q).max() > 0
    help_text = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--scalar-walls" in help_text.stdout + help_text.stderr
    (tmp_path / "bad.txt").write_text(f"{nb} 1 2.0\n")
    for args, word in ((["--scalar-walls", str(tmp_path / "walls.txt")], "--scalar"),
                       (scalar + ["--scalar-walls", str(tmp_path / "walls.txt"), "--device", "cpu"], "--scalar-walls"),
                       (scalar + ["--scalar-walls", str(tmp_path / "bad.txt")], "--scalar-walls")):
        r = subprocess.run(base + args + ["--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and word in r.stderr, (args, r.stderr)
