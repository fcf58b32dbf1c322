"""Forcing zones on the device, D3Q19 (lbm3d_forcing_*; include/lbm_forcing_hip.h, csrc/lbm3d_forcing.hip,
csrc/lbm_forcing.hpp); the 3-D twin of tests/test_gpu_forcing.py.

Bar: after every forcing_apply the stored lattice is BITWISE (uint32 patterns) the restatement
(lio.forcing_kick3d, zone after zone in index order) of what the same handle stored just before, on both
sides of the flow pair, for both numerics, both compiled forms, every box of the 2-D list with
(z0, d) = (0, nz), (1, 1), (nz - 1, 1), 1, 2 and 3 z slabs, degenerate shapes, hard states and the boxes
past the launch clamps; the impulse lies within the fold bound of math.fsum of the restatement's terms; a run
of 1, 2, 3 or 5 steps afterwards continues bit for bit as a second handle does that loaded the kicked cells;
run_forced is its definition and, at stride 1, the CPU loop bit for bit.  No tolerance is new.
"""
from __future__ import annotations

import numpy as np
import pytest

import caps_cases as cc
import forcing_cases as fc
from lbm_amd import io as lio
from oracle import oracle
from test_forcing_host import BRINKMAN_BOUND, CROSS_BOUND, POISEUILLE_BOUND

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)
GRIDS = [(13, 7, 5), (16, 8, 8)]
FORMS = ["uniform", "fields"]

_b32, _same = fc.b32, fc.same


def _problem(nx, ny, nz, seed, obstacles=0.1, walls=True):
    """The channel walls plus about 10 % random obstacles; populations perturbed by 5 %."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < obstacles).astype(np.uint8)
    if walls:
        obst |= lio.channel_obstacles3d(nx, ny, nz)
        obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    c0[obst != 0, 2::5] = np.float32(-0.0)
    return p, obst, c0


def _whole(grid, form, seed=1, index=0):
    return fc.box_zone(index, (0, 0, 0) + tuple(grid), seed, form == "fields", idle=0.2)


def _apply_and_check(e, obst, zones, n=1.0, what="", impulse=True, nan_as_one=False, where=None):
    before = e.store()[0]
    imp = e.forcing_apply(n, impulse=impulse)
    got = e.store()[0]
    want, terms = fc.restate(before, obst, zones, n)
    cc.assert_same_bits(got, want, str(what), where, nan_as_one=nan_as_one)
    assert _same(got[..., 0], before[..., 0]), what
    if impulse:
        assert imp.shape == (8, 3)
        fc.check_impulse(imp, terms, what)
    else:
        assert imp is None
    return got


def _sequence(e, obst, c0, zones, what="", chunks=CHUNKS):
    e.load_cells(c0)
    e.forcing_clear()
    fc.set_zones(e, zones)
    assert e.forcing_zones() == sorted(z["index"] for z in zones)
    cells = None
    for i, c in enumerate(chunks):
        e.run_steps(c)
        cells = _apply_and_check(e, obst, zones, (1.0, float(c), 0.5)[i % 3], (what, i), impulse=i % 2 == 0)
    return cells


# ---------------------------------------------------------- kick, bitwise ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("numerics", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_kick_sequences_bitwise(gpu_lib, nx, ny, nz, numerics, form):
    p, obst, c0 = _problem(nx, ny, nz, 7)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if numerics == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        kicked = _sequence(e, obst, c0, [_whole((nx, ny, nz), form)], (nx, ny, nz, numerics, form))
        assert not _same(kicked, c0)


def test_wide_rows_cross_waves_and_blocks(gpu_lib):
    """nx = 300: more than one wave of quads per row and a ragged tail; nx = 258: a tail of two cells; a box
    whose edges cut quads in the second wave."""
    for nx in (300, 258):
        p, obst, c0 = _problem(nx, 5, 3, nx)
        zones = [_whole((nx, 5, 3), "fields"), fc.box_zone(2, (253, 1, 1, nx - 254, 3, 2), 5, False)]
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            _sequence(e, obst, c0, zones, nx, chunks=(2, 1))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_boxes_cut_the_quads_every_way(gpu_lib, nx, ny, nz, form):
    p, obst, c0 = _problem(nx, ny, nz, nx + nz)
    boxes = fc.boxes3d(nx, ny, nz)
    assert len(boxes) >= 17
    with gpu_lib.Engine3D(p, obst, parts=2, devices=[0]) as e:
        e.load_cells(c0)
        for i, box in enumerate(boxes):
            e.forcing_clear()
            z = fc.box_zone(i % 8, box, 10 * nx + i, form == "fields")
            fc.set_zones(e, [z])
            sl = tuple(slice(o, o + n) for o, n in zip(box[:3][::-1], box[3:][::-1]))
            before = e.store()[0]
            got = _apply_and_check(e, obst, [z], 1.0 + i % 3, (box, form), impulse=i % 2 == 0)
            outside = np.ones((nz, ny, nx), bool)
            outside[sl] = False
            assert _same(got[outside], before[outside])
            assert obst[sl].all() or not _same(got[sl], before[sl])


def test_overlapping_zones_and_an_idle_part(gpu_lib):
    nx, ny, nz = 16, 8, 8
    p, obst, c0 = _problem(nx, ny, nz, 3)
    c0 = c0.copy()
    c0[..., 4] = np.float32(-0.0)
    lam = np.zeros((nz, ny, nx), np.float32)
    lam[:, :, 4:11] = 0.3
    zones = [fc.zone(6, (0, 0, 0), (nx, ny, nz), lam, (0.02, 0.0, -0.01)), fc.box_zone(1, (2, 1, 1, 9, 5, 6), 1, False),
             fc.box_zone(4, (5, 2, 0, 10, 5, 4), 2, True)]
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e, gpu_lib.Engine3D(p, obst, devices=[0]) as e2:
        for h in (e, e2):
            h.load_cells(c0)
            fc.set_zones(h, zones if h is e else zones[::-1])
        got = _apply_and_check(e, obst, zones, 1.0, "overlap")
        imp = e.forcing_apply(2.0, impulse=True)
        e2.forcing_apply(1.0)
        assert _same(e2.store()[0], got)
        imp2 = e2.forcing_apply(2.0, impulse=True)
        assert np.array_equal(imp.view(np.uint64), imp2.view(np.uint64)) and imp[[1, 4, 6]].any(axis=1).all()
        e.forcing_clear()
        e.load_cells(c0)
        fc.set_zones(e, zones[:1])
        got = _apply_and_check(e, obst, zones[:1], 1.0, "idle part")
        idle = lam == 0
        assert _same(got[idle], c0[idle]) and (_b32(got[idle][:, 4]) == 0x80000000).all()


# --------------------------------------------- continuation, decomposition ----

def _crossing_zones(grid):
    nx, ny, nz = grid
    return [_whole(grid, "uniform", 6), fc.box_zone(1, (1, 1, 1, nx - 3, ny - 2, nz - 2), 8, True)]


def _continuation(n, p, obst, c0, zones, kw, what):
    """Kick, then run k steps -- on the kicked handle and on a second one that loaded the kicked cells -- for
    k = 1, 2, 3, 5: one-, two- and three-step passes all start from kicked ghost planes."""
    with n.Engine3D(p, obst, **kw) as a, n.Engine3D(p, obst, **kw) as b:
        a.load_cells(c0)
        fc.set_zones(a, zones)
        a.run_steps(3)
        cells, forms = None, []
        for i, k in enumerate((1, 2, 3, 5)):
            kicked = _apply_and_check(a, obst, zones, 1.0 + i % 2, (what, k))
            b.load_cells(kicked)
            a.run_steps(k)
            forms.append(a.run_stats()[:3])
            b.run_steps(k)
            cells, cells_b = a.store()[0], b.store()[0]
            cc.assert_same_bits(cells, cells_b, str((what, k)))
        return cells, forms


@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for grid in GRIDS:
        p, obst, c0 = _problem(*grid, 11)
        cells, _ = _continuation(gpu_lib, p, obst, c0, _crossing_zones(grid), dict(devices=[0]), "single")
        for a in (obst, c0, cells):
            a.setflags(write=False)
        out[grid] = (p, obst, c0, cells)
    return out


@pytest.mark.parametrize("numerics", ["bitwise", "tolerance"])
def test_a_run_continues_from_the_kicked_lattice(gpu_lib, numerics):
    p, obst, c0 = _problem(16, 8, 8, 19)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if numerics == "tolerance" else 0)
    _, forms = _continuation(gpu_lib, p, obst, c0, _crossing_zones((16, 8, 8)), kw, numerics)
    assert forms[0] == (0, 0, 1) and forms[1] == (0, 1, 0)
    assert forms[2] in ((1, 0, 0), (0, 1, 1)) and sum(f[0] for f in forms) > 0


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_slabs_kick_and_continue_bitwise(gpu_lib, single, nx, ny, nz, parts):
    p, obst, c0, ref = single[(nx, ny, nz)]
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        assert len(e.local_slabs()) == parts
    cells, _ = _continuation(gpu_lib, p, obst, c0, _crossing_zones((nx, ny, nz)), dict(parts=parts, devices=[0]),
                             (nx, ny, nz, parts))
    assert _same(cells, ref)


# ------------------------------------------------------ degenerate shapes ----

@pytest.mark.parametrize("nx,ny,nz", [(1, 1, 1), (5, 3, 2), (8, 4, 3), (3, 2, 2), (4, 1, 1)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny, nz):
    """Among them nx < 4: one cell per lane."""
    p, obst, c0 = _problem(nx, ny, nz, 5, 0.2 if nx * ny * nz > 8 else 0.0, False)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        for form in FORMS:
            _sequence(e, obst, c0, [_whole((nx, ny, nz), form)], (nx, ny, nz, form), chunks=(3, 2, 1))


def test_all_obstacle_grid_keeps_every_bit(gpu_lib):
    p, _, c0 = _problem(9, 4, 3, 2, walls=False)
    c0 = c0.copy()
    c0[..., 3] = np.float32(-0.0)
    obst = np.ones((3, 4, 9), np.uint8)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        for form in FORMS:
            zones = [_whole((9, 4, 3), form)]
            e.forcing_clear()
            fc.set_zones(e, zones)
            assert _same(_apply_and_check(e, obst, zones, 1.0, "all obstacles"), c0)
            assert not e.forcing_apply(1.0, impulse=True).any()


# -------------------------------------------------------- past the clamps ----

def _caps_state(box, seed):
    nx, ny, nz = box
    rng = np.random.default_rng(seed)
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    obst = (rng.random((nz, ny, nx), dtype=np.float32) < 0.1).astype(np.uint8)
    one = oracle.init_cells3d(lio.Params3D(1, 1, 1, 0, 0.1, 0.002, 1.85)).reshape(19)
    cells = (one * (np.float32(0.875) + np.float32(0.25) * rng.random((nz, ny, nx, 19), dtype=np.float32))).astype(np.float32)
    return p, obst, cells, rng


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("box", [cc.BOXES_STRIDED[0], cc.BOX_ROWS], ids=lambda b: "x".join(map(str, b)))
def test_whole_domain_zone__forcing_zone3d_past_the_clamps(gpu_lib, box, form):
    """8 x 512 x 130: slab_grid is 1 x 128 x 128 blocks, planes 128 and 129 are a second trip of the plane loop;
    5 x 262200 x 1: gridDim.y is clamped and rows 262140 .. are a second trip of the row loop."""
    nx, ny, nz = box
    p, obst, c0, rng = _caps_state(box, sum(box))
    last = cc.slab_last_trip_mask(*box)
    assert last.any() and not last.all() and obst[last].any() and (obst[last] == 0).any()
    if form == "fields":
        lam = (np.float32(0.5) * rng.random((nz, ny, nx), dtype=np.float32)).astype(np.float32)
        z = fc.zone(0, (0, 0, 0), box, lam, (0.02, -0.01, 0.005), (1e-3, 2e-3, -1e-3))
    else:
        z = fc.zone(0, (0, 0, 0), box, 0.25, (0.02, -0.01, 0.005), (1e-3, 2e-3, -1e-3))
    gx, gy, gz = cc.slab_grid(*box)

    def where(zz, y, x, k):
        return (f"plane {zz}: trip {zz // gz} of the plane loop; row {y}: trip {y // (gy * cc.S3Y)} of the row loop; "
                f"lane {x // 4 % cc.S3X}, cell {x % 4}, speed {k}")
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        assert e.local_slabs() == [(0, nz)]
        e.load_cells(c0)
        fc.set_zones(e, [z])
        imp = e.forcing_apply(1.0, impulse=True)
        got = e.store()[0]
    want, terms = fc.restate(c0, obst, [z], 1.0)
    cc.assert_touched(want, c0, last[..., None], "kick")
    cc.assert_same_bits(got, want, f"{box} forcing_zone3d {form}", where)
    fc.check_impulse(imp, terms, (box, form))
    for c in range(3):
        assert abs(float(terms[0][..., c][last].astype(np.float64).sum())) > 100 * fc.fold_bound(terms[0][..., c])


# ------------------------------------------------------------ hard states ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_hard_states(gpu_lib, nx, ny, nz, form):
    """A fluid cell of density zero, subnormal populations, NaN (with payloads), Inf and 2^100 under
    obstacles: the restatement's bits, NaN payloads compared as one; obstacle cells keep theirs raw."""
    p, obst, c0 = _problem(nx, ny, nz, 77 + nx)
    c0 = c0.copy()
    rng = np.random.default_rng(5)
    fl, ob = np.argwhere(obst == 0), np.argwhere(obst != 0)
    pick = lambda a, n: a[rng.choice(len(a), n, replace=False)]          # noqa: E731
    for z, y, x in pick(fl, 4):
        c0[z, y, x] = 0.0
    for z, y, x in pick(fl, 8):
        c0[z, y, x] *= np.float32(2.0 ** -130)
    raw = c0.view(np.uint32)
    for i, (z, y, x) in enumerate(pick(ob, 9)):
        if i % 3 == 0:
            raw[z, y, x, :] = 0x7FC00123 if i % 2 else 0xFFC00456
        elif i % 3 == 1:
            c0[z, y, x, ::2] = np.inf
            c0[z, y, x, 1::2] = -np.inf
        else:
            c0[z, y, x] = np.float32(2.0 ** 100)
    zones = [_whole((nx, ny, nz), form, 9), fc.zone(4, (1, 1, 1), (nx - 2, ny - 2, nz - 2), 1.0, (0.03, 0.01, -0.02))]
    with np.errstate(all="ignore"), gpu_lib.Engine3D(p, obst, parts=2, devices=[0]) as e:
        e.load_cells(c0)
        fc.set_zones(e, zones)
        assert np.array_equal(_b32(e.store()[0]), _b32(c0))
        got = _apply_and_check(e, obst, zones, 1.0, (nx, ny, nz, form), nan_as_one=True)
        assert np.array_equal(_b32(got[obst != 0]), _b32(c0[obst != 0]))
        assert np.isfinite(got[obst == 0]).all()


# --------------------------------------------------------------- contract ----

def test_forcing_contract(gpu_lib):
    import ctypes
    n = gpu_lib
    p, obst, c0 = _problem(13, 7, 5, 9)
    nan, inf = float("nan"), float("inf")
    K = lambda *v: (ctypes.c_float * 7)(*v)                                          # noqa: E731
    good = K(0.1, 0.01, 0.0, 0.0, 1e-4, 0.0, 0.0)
    with n.Engine3D(p, obst, parts=2, devices=[0]) as e:
        L, h = e._L, e._h
        assert L.lbm3d_forcing_set_zone(None, 0, 0, 0, 0, 4, 4, 2, None, good) == n.LBM_E_INVALID
        assert L.lbm3d_forcing_clear(None) == n.LBM_E_INVALID and L.lbm3d_forcing_apply(None, 1.0, None) == n.LBM_E_INVALID
        assert L.lbm3d_forcing_zones(None, None, None) == n.LBM_E_INVALID
        assert L.lbm3d_forcing_set_zone(h, 1, 2, 1, 1, 9, 5, 3, None, good) == n.LBM_OK
        assert L.lbm3d_forcing_apply(h, 1.0, None) == n.LBM_E_STATE                  # before the lattice is loaded
        e.load_cells(c0)
        arr = np.full((3, 5, 9), 0.1, np.float32)
        arr[2, 4, 8] = inf
        table = (ctypes.POINTER(ctypes.c_float) * 7)(None, None, None, None, None, None, n._ptr(arr))
        for bad in ((-1, 0, 0, 0, 4, 4, 2, None, good), (8, 0, 0, 0, 4, 4, 2, None, good),
                    (0, 10, 0, 0, 4, 4, 2, None, good), (0, 0, 4, 0, 4, 4, 2, None, good), (0, 0, 0, 4, 4, 4, 2, None, good),
                    (0, 0, 0, -1, 4, 4, 2, None, good), (0, 0, 0, 0, 4, 4, -2, None, good),
                    (0, 0, 0, 0, 4, 4, 2, None, K(-0.1, 0, 0, 0, 0, 0, 0)), (0, 0, 0, 0, 4, 4, 2, None, K(0.1, 0, 0, nan, 0, 0, 0)),
                    (0, 0, 0, 0, 4, 4, 2, None, K(0.1, 0, 0, 0, 0, 0, inf)), (1, 2, 1, 1, 9, 5, 3, table, good)):
            assert L.lbm3d_forcing_set_zone(h, *bad) == n.LBM_E_INVALID, bad[:7]
            assert L.lbm3d_last_error(h)
        assert e.forcing_zones() == [1]
        for bad in (nan, inf, -1.0):
            assert L.lbm3d_forcing_apply(h, bad, None) == n.LBM_E_INVALID
        assert L.lbm3d_forcing_apply(h, 0.0, None) == n.LBM_OK
        assert _same(e.store()[0], c0) and (_b32(c0) == 0x80000000).any()               # every bit, -0.0f included
        with pytest.raises(ValueError):
            e.forcing_zone(0, (0, 0), (4, 4))
        zones = [fc.zone(1, (2, 1, 1), (9, 5, 3), 0.1, (0.01, 0.0, 0.0), (1e-4, 0.0, 0.0))]
        _apply_and_check(e, obst, zones, 1.0, "contract")
        e.forcing_clear()
        kept = e.store()[0]
        assert not e.forcing_apply(1.0, impulse=True).any() and _same(e.store()[0], kept)


# --------------------------------------------- run_forced is its definition ----

def test_run_forced_equals_the_loop_and_the_cpu_loop(gpu_lib):
    p, obst, c0 = _problem(16, 8, 8, 21)
    zones = _crossing_zones((16, 8, 8))
    refs = {}
    for stride in (1, 3):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:                  # by hand
            e.load_cells(c0)
            fc.set_zones(e, zones)
            done = 0
            while done < 13:
                n = min(stride, 13 - done)
                e.forcing_apply(n)
                e.run_steps(n)
                done += n
            refs[stride] = e.store()[0]
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            e.load_cells(c0)
            fc.set_zones(e, zones)
            av = e.run_forced(13, stride)
            assert av.size == 0 and _same(e.store()[0], refs[stride])
            with pytest.raises(ValueError):
                e.run_forced(5, accelerate_first=True)
    assert not _same(refs[1], refs[3])
    want, _ = fc.cpu_forced(p, obst, c0, zones, 13, dims=3)
    cc.assert_same_bits(refs[1], want, "run_forced(13) against the CPU loop")
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        fc.set_zones(e, zones)
        hist = e.forcing_history(13, 5)
        assert [s[0] for s in hist] == [5, 10, 13] and all(s[1].shape == (8, 3) for s in hist)
        assert _same(e.store()[0], refs[1]) and hist[0][1][[0, 1]].any(axis=1).all() and not hist[0][1][2:].any()


@pytest.mark.parametrize("lam", [0.0, 0.01])
def test_slot_profiles_on_the_device(gpu_lib, lam):
    p, obst, c0, zones = fc.slot(3, lam)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        fc.set_zones(e, zones)
        e.run_forced(fc.SLOT_STEPS)
        cells = e.store()[0]
    err, across = fc.slot_profile_error(p, obst, cells, lam, 3)
    print(f"3-D slot on the device, lam = {lam}: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= (POISEUILLE_BOUND if lam == 0 else BRINKMAN_BOUND[lam]) and across <= CROSS_BOUND
