"""D3Q19 momentum-exchange wall forces computed on the device (lbm3d_wall_force /
lbm3d_store_wall_force / lbm3d_set_bodies / lbm3d_body_forces;
include/lbm_forces_hip.h, csrc/lbm3d_forces.hip).

Bar: the per-cell map is BITWISE lio.wall_force_cells3d of the cells
Engine3D.store() returns from the same handle (every pass form, both numerics,
both lattices of the pair, z slabs -- links across slab faces -- and the RCCL
transport); totals and per-body sums within (n - 1) 2^-53 sum|term| of
math.fsum of the map, links exact, repeat calls identical.  The direction
table itself is pinned by physics: the momentum balance of the fluid over two
consecutive steps (see tests/test_forces_host.py).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle
from test_gpu_forces import _bits, check_totals_and_bodies

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, accel=0.002):
    """tests/test_gpu_fields3d.py's recipe with 10 % random obstacles."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, accel, 1.7)
    rng = np.random.default_rng(seed)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    obst[rng.random((nz, ny, nx)) < 0.1] = 1
    c0 = (oracle.init_cells3d(p) * (1 + 0.02 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _assert_map(got, obst, cells, what=""):
    ref = lio.wall_force_cells3d(obst, cells)
    assert len(got) == 3
    for name, g, r in zip("xyz", got, ref):
        assert g.dtype == np.float32 and g.shape == r.shape, (what, name)
        bad = _bits(g) != _bits(r)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return ref


def _check_against_store(e, obst, what, labels=None, nbodies=0):
    cells, _ = e.store()
    ref = _assert_map(e.wall_force_field(), obst, cells, what)
    check_totals_and_bodies(e, lio.wall_links3d(obst), ref, labels, nbodies, what=str(what))
    return cells


@pytest.mark.parametrize("nx,ny,nz", [(13, 9, 7), (67, 5, 3), (130, 3, 2), (1, 5, 3), (3, 1, 1), (1, 1, 1)])
def test_wall_force3d_map_of_loaded_cells_bitwise(gpu_lib, nx, ny, nz):
    """Ragged shapes, rows padded to the pitch, extents of 1 and 2 (a cell that is its
    own neighbour, or meets the same neighbour along +e and -e)."""
    p, obst, c0 = _problem(nx, ny, nz, nx + ny + nz)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        got = e.wall_force_field()
        _assert_map(got, obst, c0, (nx, ny, nz))
        links = lio.wall_links3d(obst)
        for g in got:
            assert not _bits(g)[links == 0].any()   # exactly +0
        check_totals_and_bodies(e, links, got, what=f"{nx}x{ny}x{nz}")


@pytest.mark.usefixtures("debug_knobs")
@pytest.mark.parametrize("form", ["three", "two", "one", "tolerance"])
def test_wall_force3d_after_steps_every_pass_form(gpu_lib, form, monkeypatch):
    """After 9 steps and after 1 more (the other lattice of the pair); 3 more steps then
    end on the lattice an engine that never asked for forces reaches."""
    env = {"three": {}, "two": {"LBM3D_THREE": "0"}, "one": {"LBM3D_TWO": "0"}, "tolerance": {}}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    p, obst, c0 = _problem(70, 31, 24, 7)
    labels, nbodies = lio.label_bodies(obst)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        for steps in (9, 1):
            e.run_steps(steps)
            _check_against_store(e, obst, (form, steps))
        e.set_bodies(labels, nbodies)
        e.body_forces()
        e.run_steps(3)
        after, _ = e.store()
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        for steps in (9, 1, 3):
            e.run_steps(steps)
        plain, _ = e.store()
    assert np.array_equal(_bits(after), _bits(plain))


@pytest.mark.parametrize("parts", [1, 2, 3, 7])
def test_wall_force3d_slabs_and_bodies(gpu_lib, parts):
    """One slab and z slabs on GPU 0 (ragged extents): links across slab faces and the
    periodic wrap, bodies that span slabs."""
    p, obst, c0 = _problem(20, 11, 15, 3)
    labels, nbodies = lio.label_bodies(obst)
    assert nbodies >= 2
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(5)
        assert len(e.local_slabs()) == parts
        e.set_bodies(labels, nbodies)
        _check_against_store(e, obst, ("slabs", parts), labels, nbodies)
        lab2 = np.where(labels == 0, -1, labels)          # the walls belong to no body
        e.set_bodies(lab2, nbodies)
        _check_against_store(e, obst, ("slabs, negative label", parts), lab2, nbodies)
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.set_bodies(labels, 1)
        assert ei.value.code == gpu_lib.LBM_E_INVALID
        e.set_bodies(None, 0)
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.body_forces()
        assert ei.value.code == gpu_lib.LBM_E_STATE


def test_wall_force3d_rccl_world_of_one(gpu_lib):
    p, obst, c0 = _problem(24, 10, 9, 11)
    labels, nbodies = lio.label_bodies(obst)
    with gpu_lib.Engine3D(p, obst, transport=gpu_lib.TRANSPORT_RCCL, rank=0, world=1, devices=[0],
                          unique_id=gpu_lib.rccl_unique_id()) as e:
        e.load_cells(c0)
        e.run_steps(5)
        e.set_bodies(labels, nbodies)
        _check_against_store(e, obst, "rccl", labels, nbodies)


def test_wall_force3d_state_and_degenerate(gpu_lib):
    p = lio.Params3D(6, 5, 4, 0, 0.1, 0.002, 1.7)
    c0 = oracle.init_cells3d(p)
    with gpu_lib.Engine3D(p, lio.channel_obstacles3d(6, 5, 4), devices=[0]) as e:
        for call in (e.wall_force, e.wall_force_field, e.body_forces, lambda: e.set_bodies(None, 0)):
            with pytest.raises(gpu_lib.LbmError) as ei:
                call()
            assert ei.value.code == gpu_lib.LBM_E_STATE, call
    for obst in (np.zeros((4, 5, 6), np.uint8), np.ones((4, 5, 6), np.uint8)):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            e.load_cells(c0)
            assert e.wall_force() == (0.0, 0.0, 0.0, 0)
            for g in e.wall_force_field():
                assert not _bits(g).any()


@pytest.mark.parametrize("tolerance", [False, True], ids=["bitwise", "tolerance"])
def test_momentum_balance3d(gpu_lib, tolerance):
    """The only physics check of the 3-D direction table.  Over one step the fluid's
    momentum changes by the body force minus what the walls took:
        P_f(n+1) - P_f(n) = A - (F(n) + F(n+1)) / 2,  A = (n_fluid density accel / 3, 0, 0)
    (every fluid cell is accelerated along +x).  Wall planes plus one box body, cells
    from e.store().  Bound: 16 * 2^-24 * (fluid mass), a few fp32 ulps of density per
    colliding cell; a wrong sign or a swapped direction misses by about |F|."""
    nx, ny, nz = 24, 14, 12
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.005, 1.7)
    obst = lio.channel_obstacles3d(nx, ny, nz).copy()
    obst[3:8, 3:10, 5:13] = 1          # a box off every axis' centre
    rng = np.random.default_rng(5)
    e3 = np.array(lio.E3, np.float64)
    # a start that moves along +y and +z too, so that every component of F is far above the bound
    bias = 1 + 0.10 * (e3[:, 1] > 0) + 0.10 * (e3[:, 2] > 0)
    c0 = (oracle.init_cells3d(p) * bias * (1 + 0.02 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    fluid = obst == 0

    def momentum(cells):
        return cells[fluid].astype(np.float64).sum(0) @ e3

    with gpu_lib.Engine3D(p, obst, devices=[0], flags=gpu_lib.FLAG_TOLERANCE if tolerance else 0) as e:
        e.load_cells(c0)
        e.run_steps(3)
        state = []
        for _ in range(4):
            cells, _ = e.store()
            state.append((momentum(cells), np.array(e.wall_force()[:3])))
            e.run_steps(1)
    mass = float(c0[fluid].astype(np.float64).sum())
    a = np.array([fluid.sum() * float(np.float32(p.density)) * float(np.float32(p.accel)) / 3, 0.0, 0.0])
    bound = 16 * 2.0 ** -24 * mass
    for (p1, f1), (p2, f2) in zip(state, state[1:]):
        res = (p2 - p1) - (a - (f1 + f2) / 2)
        print(f"residual {res}, bound {bound:.3e}, F {f2}, A {a[0]:.3e}")
        assert np.all(np.abs(res) <= bound), (res, bound)
    # the check has teeth: every component of F is far above the bound in some sample
    assert np.all(np.max(np.abs([f for _, f in state]), axis=0) > 10 * bound)


@pytest.mark.usefixtures("debug_knobs")
def test_wall_force3d_512x512x448_64bit_offsets(gpu_lib, monkeypatch):
    """117 M cells in one slab: plane 447 starts 2.2e9 floats into the lattice, so a
    wall-list offset formed in 32 bits would wrap there.  The channel started at rest
    stays invariant in x and z bit for bit (tests/test_gpu_fields3d.py checks that on
    the stored cells), so the map is one column's map everywhere; the column comes from
    a 16 x 512 x 4 engine.  The placement probe is off as in the fields test."""
    monkeypatch.setenv("LBM3D_PLACEMENT_TRIES", "1")
    nx, ny, nz = 512, 512, 448
    small = lio.Params3D(16, ny, 4, 0, 0.1, 0.001, 1.85)
    sobst = lio.channel_obstacles3d(16, ny, 4)
    with gpu_lib.Engine3D(small, sobst, devices=[0]) as e:
        e.init_equilibrium()
        e.run_steps(3)
        cells, _ = e.store()
    column = [c[1, :, 5] for c in lio.wall_force_cells3d(sobst, cells)]
    assert np.abs(column[1][[0, -1]]).min() > 1e-3     # the walls carry the pressure
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.001, 1.85)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    labels = np.where(obst != 0, 0, -1).astype(np.int32)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.init_equilibrium()
        e.run_steps(3)
        fmap = e.wall_force_field()
        total = e.wall_force()
        e.set_bodies(labels, 1)
        body = e.body_forces()
    del labels
    for name, g, col in zip("xyz", fmap, column):
        assert np.array_equal(_bits(g), np.broadcast_to(_bits(col)[None, :, None], g.shape)), name
    n = 2 * nx * nz                                    # wall cells; five links each
    assert total[3] == 5 * n and int(body[3][0]) == 5 * n
    for i, col in enumerate(column):
        terms = col[[0, -1]].astype(np.float64)
        ref = float(terms.sum()) * (nx * nz)           # one rounding, far inside the bound
        bound = (n - 1) * 2.0 ** -53 * float(np.abs(terms).sum()) * (nx * nz)
        print(f"f{'xyz'[i]}: total {total[i]!r} body {float(body[i][0])!r} ref {ref!r} bound {bound:.3e}")
        assert abs(total[i] - ref) <= 2 * bound and abs(float(body[i][0]) - ref) <= 2 * bound
