"""D3Q19 macroscopic fields, box extracts and lattice stats computed on the device
(lbm3d_store_fields / lbm3d_store_fields_box / lbm3d_field_stats;
include/lbm3d_fields_hip.h, csrc/lbm3d_fields.hip).

Bar: the five fields are BITWISE (compared as uint32 patterns) the values
lio.macroscopic3d -- the fp32 numpy restatement of the definition, pinned to
the oracle in tests/test_fields3d_host.py -- derives from the AoS cells
Engine3D.store() returns from the same handle: for every pass form and
numerics mode, both lattices of the ping-pong pair, both access paths (16-B
quads with the ragged nx % 4 tail, one cell per lane), z slabs, the RCCL
transport and the placement knobs.  Inputs follow tests/test_d3q19.py's
recipe (channel walls, 5 % random obstacles, 2 % perturbation): densities stay
positive, no NaN arises.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

FIELDS = ("ux", "uy", "uz", "speed", "pressure")
SENTINEL = 0x7FC00001   # a quiet NaN pattern no computation produces
THIRD = np.float32(1) / np.float32(3)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_fields(got, ref, what="", sl=np.s_[:, :, :]):
    """got: {name: array}; ref: lio.macroscopic3d's tuple, compared on its slice sl."""
    for name, r in zip(FIELDS, ref):
        if name in got:
            assert got[name].dtype == np.float32 and got[name].shape == r[sl].shape, (what, name, got[name].shape)
            bad = _bits(got[name]) != _bits(r[sl])
            assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed, accel=0.002):
    p = lio.Params3D(nx, ny, nz, 0, 0.1, accel, 1.7)
    rng = np.random.default_rng(seed)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    obst[rng.random((nz, ny, nx)) < 0.05] = 1
    c0 = (oracle.init_cells3d(p) * (1 + 0.02 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _rho32(cells):
    rho = cells[..., 0]
    for k in range(1, 19):
        rho = rho + cells[..., k]
    return rho


def _check_against_store(e, p, obst, what, stats=False):
    """fields() of the handle's current lattice against its own store()."""
    cells, _ = e.store()
    ref = lio.macroscopic3d(p, obst, cells)
    _assert_fields(e.fields(), ref, what)
    if stats:
        _assert_stats(e.field_stats(), cells, obst, ref, what)
    return cells, ref


def _assert_stats(got, cells, obst, ref, what=""):
    mass, umax = got
    rho = _rho32(cells)
    mass_ref = float(rho.astype(np.float64).sum())
    n = rho.size
    fluid = obst == 0
    umax_ref = np.float32(ref[3][fluid].max()) if fluid.any() else np.float32(0)
    print(f"{what}: mass {mass!r} ref {mass_ref!r} rel {abs(mass - mass_ref) / mass_ref:.3e} "
          f"bound {2 * (n - 1) * 2.0 ** -53:.3e}; max |u| {umax!r} ref {float(umax_ref)!r}")
    # any summation order of n fp64 terms stays within (n - 1) u of the exact sum, relative; two orders: twice that
    assert abs(mass - mass_ref) <= 2 * (n - 1) * 2.0 ** -53 * mass_ref, what
    assert _bits(np.float32(umax)) == _bits(umax_ref), what


# ------------------------------------------------------- 1. bare kernel ----

@pytest.mark.parametrize("nx,ny,nz", [(13, 9, 7), (64, 8, 5), (1, 5, 3), (130, 3, 2), (67, 5, 3), (132, 6, 4),
                                      (3, 1, 1), (1, 1, 1)])
def test_fields3d_of_loaded_cells_bitwise(gpu_lib, nx, ny, nz):
    """Quads only, quads plus a ragged tail, nx < 4 (one cell per lane), rows
    padded to px, a single row / plane."""
    p, obst, c0 = _problem(nx, ny, nz, nx + ny + nz)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        cells, _ = e.store()
        got = e.fields()
    assert np.array_equal(cells, c0)
    assert set(got) == set(FIELDS)
    _assert_fields(got, lio.macroscopic3d(p, obst, cells), (nx, ny, nz))
    ob = obst != 0
    assert ob.any()
    for name in ("ux", "uy", "uz", "speed"):
        assert not _bits(got[name])[ob].any(), name   # exactly +0
    assert (_bits(got["pressure"])[ob] == _bits(np.float32(p.density) * THIRD)).all()


@pytest.mark.parametrize("nx,ny,nz", [(8, 1200, 64), (5, 262200, 1)])
def test_fields3d_grid_strides_bitwise(gpu_lib, nx, ny, nz):
    """More planes than the launch's z blocks (8 x 1200 x 64: 300 row blocks, 54
    plane blocks) and more rows than a grid's y extent (262200 rows > 4 x 65535):
    the kernel strides over the rest; stats fold the strided cells too."""
    p, obst, c0 = _problem(nx, ny, nz, 5)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        got = e.fields()
        stats = e.field_stats()
    ref = lio.macroscopic3d(p, obst, c0)
    _assert_fields(got, ref, (nx, ny, nz))
    _assert_stats(stats, c0, obst, ref, (nx, ny, nz))


# --------------------------------------- 2. after steps, every pass form ----

@pytest.mark.usefixtures("debug_knobs")
@pytest.mark.parametrize("form", ["three", "two", "one", "tolerance"])
def test_fields3d_after_steps_every_pass_form(gpu_lib, form, monkeypatch):
    """Three-step passes (default), LBM3D_THREE=0 (two-step), LBM3D_TWO=0 (one-step
    launches) and the tolerance collision: after 9 steps and after 1 more (the
    other lattice of the pair), then 3 more steps end on the lattice an engine
    that never called the new functions reaches."""
    env = {"three": {}, "two": {"LBM3D_THREE": "0"}, "one": {"LBM3D_TWO": "0"}, "tolerance": {}}[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    p, obst, c0 = _problem(70, 31, 24, 7)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        for steps in (9, 1):
            e.run_steps(steps)
            _check_against_store(e, p, obst, (form, steps), stats=True)
            e.fields_box(3, 2, 7, 9, 5, 10)
        e.run_steps(3)
        after, _ = e.store()
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        e.load_cells(c0)
        for steps in (9, 1, 3):
            e.run_steps(steps)
        plain, _ = e.store()
    assert np.array_equal(after, plain)
    if form != "tolerance":
        ref, _ = oracle.run3d(p, obst, 13, c0)
        assert np.array_equal(after, ref)


# --------------------------------------------------------------- 3. slabs ----

@pytest.mark.parametrize("parts", [2, 3, 7])
def test_fields3d_slabs_bitwise(gpu_lib, parts):
    """z slabs on GPU 0 (ragged extents): every slab lands at its planes."""
    p, obst, c0 = _problem(20, 11, 15, parts)
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(5)
        assert len(e.local_slabs()) == parts
        _check_against_store(e, p, obst, ("slabs", parts), stats=True)


def test_fields3d_rccl_world_of_one_bitwise(gpu_lib):
    p, obst, c0 = _problem(24, 10, 9, 11)
    with gpu_lib.Engine3D(p, obst, transport=gpu_lib.TRANSPORT_RCCL, rank=0, world=1, devices=[0],
                          unique_id=gpu_lib.rccl_unique_id()) as e:
        e.load_cells(c0)
        e.run_steps(5)
        cells, ref = _check_against_store(e, p, obst, "rccl", stats=True)
        _assert_fields(e.fields_box(0, 0, 4, 24, 10, 1), ref, "rccl z-plane", np.s_[4:5, :, :])


# ----------------------------------------------------------- 4. placement ----

@pytest.mark.usefixtures("debug_knobs")
@pytest.mark.parametrize("env", [{"LBM3D_KSPAD": "320"}, {"LBM_LATTICE_PAD": "4096"}])
@pytest.mark.parametrize("nx,ny,nz,parts", [(64, 8, 5, 1), (70, 31, 24, 3)])
def test_fields3d_lattice_placement_bitwise(gpu_lib, nx, ny, nz, parts, env, monkeypatch):
    """Padded speed planes and both lattices in one allocation: rows stay 16-B
    aligned, the strides come from the handle."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p, obst, c0 = _problem(nx, ny, nz, nx + ny * nz)
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        for steps in (6, 1):
            e.run_steps(steps)
            _check_against_store(e, p, obst, (env, parts, steps), stats=True)


# --------------------------------------------------------------- 5. boxes ----

BOXES = {   # (x0, y0, z0, nx, ny, nz) on 70 x 31 x 24
    "z-plane": (0, 0, 9, 70, 31, 1),
    "y-plane": (0, 13, 0, 70, 1, 24),
    "x-plane": (41, 0, 0, 1, 31, 24),
    "x-plane at 0": (0, 0, 0, 1, 31, 24),
    "misaligned": (3, 2, 7, 9, 5, 10),          # crosses the slab boundaries at z = 8 and 16 (parts = 3)
    "aligned inner quads": (8, 1, 6, 13, 4, 5),  # x0 % 4 == 0: quads and a tail inside a row
    "one cell": (69, 30, 23, 1, 1, 1),
    "last slab": (5, 0, 17, 60, 31, 7),
}


@pytest.fixture(scope="module", params=[1, 3])
def box_engine(request, gpu_lib):
    p, obst, c0 = _problem(70, 31, 24, 21)
    with gpu_lib.Engine3D(p, obst, parts=request.param, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(4)
        cells, _ = e.store()
        yield e, request.param, lio.macroscopic3d(p, obst, cells)


@pytest.mark.parametrize("name", list(BOXES))
def test_fields3d_box_is_the_slice(box_engine, name):
    e, parts, ref = box_engine
    x0, y0, z0, nx, ny, nz = BOXES[name]
    got = e.fields_box(x0, y0, z0, nx, ny, nz)
    assert set(got) == set(FIELDS)
    _assert_fields(got, ref, (name, parts), np.s_[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx])


def test_fields3d_full_box_is_fields(box_engine):
    e, parts, ref = box_engine
    full, box = e.fields(), e.fields_box(0, 0, 0, 70, 31, 24)
    _assert_fields(full, ref, ("fields", parts))
    for name in FIELDS:
        assert np.array_equal(_bits(full[name]), _bits(box[name])), name


@pytest.mark.parametrize("box", [(0, 0, 0, 0, 31, 24), (0, 0, 0, 70, 0, 24), (0, 0, 0, 70, 31, 0), (0, 0, 0, -1, 1, 1),
                                 (-1, 0, 0, 4, 4, 4), (0, -1, 0, 4, 4, 4), (0, 0, -1, 4, 4, 4), (1, 0, 0, 70, 1, 1),
                                 (67, 0, 0, 4, 1, 1), (0, 30, 0, 1, 2, 1), (0, 0, 23, 1, 1, 2),
                                 (2 ** 31 - 1, 0, 0, 2, 1, 1)])
def test_fields3d_invalid_box(box_engine, gpu_lib, box):
    """No periodic wrap: empty, negative and domain-leaving boxes are refused."""
    e, _, _ = box_engine
    with pytest.raises(gpu_lib.LbmError) as err:
        e.fields_box(*box)
    assert err.value.code == gpu_lib.LBM_E_INVALID


# --------------------------------------------------- 6. subsets and NULLs ----

def _sentinel(shape, guard=64):
    a = np.full(int(np.prod(shape)) + guard, SENTINEL, np.uint32)
    return a, a.view(np.float32).ctypes.data_as(ctypes.POINTER(ctypes.c_float))


def test_fields3d_subsets_nulls_and_state(gpu_lib):
    n = gpu_lib
    L = n.load_library()
    p, obst, c0 = _problem(67, 5, 3, 3)
    ref = lio.macroscopic3d(p, obst, c0)
    cells = 67 * 5 * 3
    with n.Engine3D(p, obst, devices=[0]) as e:
        h = e._h
        box = n.Box3D(0, 0, 0, 67, 5, 3)
        mass, umax = ctypes.c_double(), ctypes.c_float()
        arr, ptr = _sentinel((3, 5, 67))
        # before a lattice is loaded: LBM_E_STATE, nothing written
        assert L.lbm3d_store_fields(h, None, None, None, None, ptr) == n.LBM_E_STATE
        assert L.lbm3d_store_fields_box(h, ctypes.byref(box), None, None, None, None, ptr) == n.LBM_E_STATE
        assert L.lbm3d_field_stats(h, ctypes.byref(mass), ctypes.byref(umax)) == n.LBM_E_STATE
        assert (arr == SENTINEL).all()
        e.load_cells(c0)
        # all NULL: LBM_OK
        assert L.lbm3d_store_fields(h, None, None, None, None, None) == n.LBM_OK
        assert L.lbm3d_store_fields_box(h, ctypes.byref(box), None, None, None, None, None) == n.LBM_OK
        assert L.lbm3d_field_stats(h, None, None) == n.LBM_OK
        assert L.lbm3d_store_fields_box(h, None, None, None, None, None, ptr) == n.LBM_E_INVALID
        # pressure only: exactly that array, exactly its cells
        assert L.lbm3d_store_fields(h, None, None, None, None, ptr) == n.LBM_OK
        assert np.array_equal(arr[:cells], _bits(ref[4]).ravel()) and (arr[cells:] == SENTINEL).all()
        # each field alone lands in its own argument
        for i, name in enumerate(FIELDS):
            arr, ptr = _sentinel((3, 5, 67))
            args = [None] * 5
            args[i] = ptr
            assert L.lbm3d_store_fields(h, *args) == n.LBM_OK, name
            assert np.array_equal(arr[:cells], _bits(ref[i]).ravel()) and (arr[cells:] == SENTINEL).all(), name
        # a box subset: uz and speed of a misaligned box
        sub = n.Box3D(2, 1, 1, 7, 3, 2)
        a_uz, p_uz = _sentinel((2, 3, 7))
        a_sp, p_sp = _sentinel((2, 3, 7))
        assert L.lbm3d_store_fields_box(h, ctypes.byref(sub), None, None, p_uz, p_sp, None) == n.LBM_OK
        for a, r in ((a_uz, ref[2]), (a_sp, ref[3])):
            assert np.array_equal(a[:42], _bits(r[1:3, 1:4, 2:9]).ravel()) and (a[42:] == SENTINEL).all()
        # one stat alone
        assert L.lbm3d_field_stats(h, ctypes.byref(mass), None) == n.LBM_OK
        assert L.lbm3d_field_stats(h, None, ctypes.byref(umax)) == n.LBM_OK
        assert (mass.value, umax.value) == e.field_stats()
        # the binding's subset
        got = e.fields(("uy", "pressure"))
        assert set(got) == {"uy", "pressure"}
        _assert_fields(got, ref, "subset")
        with pytest.raises(ValueError):
            e.fields(("ux", "rho"))


# --------------------------------------------------------------- 7. stats ----

@pytest.mark.parametrize("parts", [1, 3])
def test_fields3d_stats(gpu_lib, parts):
    p, obst, c0 = _problem(70, 31, 24, 33)
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(6)
        cells, _ = e.store()
        first = e.field_stats()
        again = e.field_stats()
    _assert_stats(first, cells, obst, lio.macroscopic3d(p, obst, cells), ("stats", parts))
    assert np.float64(again[0]).view(np.uint64) == np.float64(first[0]).view(np.uint64)
    assert _bits(np.float32(again[1])) == _bits(np.float32(first[1]))
    assert first[1] > 0


@pytest.mark.parametrize("parts", [1, 3])
def test_fields3d_stats_all_obstacles(gpu_lib, parts):
    p, _, c0 = _problem(21, 6, 9, 2)
    obst = np.ones((9, 6, 21), np.uint8)
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        mass, umax = e.field_stats()
        got = e.fields(("speed",))
    assert _bits(np.float32(umax)) == 0 and not _bits(got["speed"]).any()
    mass_ref = float(_rho32(c0).astype(np.float64).sum())   # obstacle cells carry mass too
    assert abs(mass - mass_ref) <= 2 * (c0[..., 0].size - 1) * 2.0 ** -53 * mass_ref


# ---------------------------------------------------------- 8. large slab ----

@pytest.mark.usefixtures("debug_knobs")
@pytest.mark.parametrize("nz", [64, 448])
def test_fields3d_512x512_slab_64bit_offsets(gpu_lib, nz, monkeypatch):
    """512 x 512 x nz initialised on the device, 3 steps: the first and the last
    z-plane and a y-plane through fields_box, and the stats, against the stored
    cells.  nz = 64 (16.8 M cells, 3.5e8 floats with the ghost planes) stays
    below 2^31 floats; at nz = 448 (117 M cells) plane 447 starts 2.2e9 floats
    into the lattice, so a 32-bit float offset would wrap there, and the
    y-plane crosses the wrap.  The channel started at rest stays invariant in x
    and z bit for bit (checked), so the whole lattice's stats follow from one
    column of a plane.  The placement probe is off as in
    test_d3q19_512cube_64bit_indexing."""
    monkeypatch.setenv("LBM3D_PLACEMENT_TRIES", "1")
    nx, ny = 512, 512
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.001, 1.85)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.init_equilibrium()
        e.run_steps(3)
        cells, _ = e.store()
        planes = {z: e.fields_box(0, 0, z, nx, ny, 1) for z in (0, nz - 1)}
        yplane = e.fields_box(0, 255, 0, nx, 1, nz)
        mass, umax = e.field_stats()
    for z, got in planes.items():
        _assert_fields(got, lio.macroscopic3d(p, obst[z:z + 1], cells[z:z + 1]), ("z-plane", z))
    _assert_fields(yplane, lio.macroscopic3d(p, obst[:, 255:256], cells[:, 255:256]), "y-plane")
    column = cells[:1, :, :1]
    assert np.array_equal(cells, np.broadcast_to(column, cells.shape))
    speed = lio.macroscopic3d(p, obst[:1, :, :1], column)[3]
    assert _bits(np.float32(umax)) == _bits(speed[obst[:1, :, :1] == 0].max()) and umax > 0
    # the column's fp64 sum times the columns: one rounding, far inside the bound
    mass_ref = float(_rho32(column).astype(np.float64).sum()) * (nx * nz)
    assert abs(mass - mass_ref) <= 2 * (nx * ny * nz - 1) * 2.0 ** -53 * mass_ref
