"""Forcing zones on the device, D2Q9 (lbm_forcing_*; include/lbm_forcing_hip.h, csrc/lbm_forcing.hip,
csrc/lbm_forcing.hpp).

Bar: after every forcing_apply the stored lattice is BITWISE (uint32 patterns) the restatement
(lio.forcing_kick, zone after zone in index order; pinned by physics in tests/test_forcing_host.py) of what
the same handle stored just before -- on both sides of the flow pair, for every step kernel, both compiled
forms (uniform, fields), every way a box's edge can cut the quads, decomposed handles, degenerate shapes,
hard states and a launch past the grid clamp; the impulse lies within the fold bound of math.fsum of the
restatement's terms and is identical between two handles in the same state; a run afterwards continues bit
for bit, av_vels included, as a second handle does that loaded the kicked cells; run_forced is its
definition and, at stride 1 on the default kernel, the CPU loop (oracle step + lio) bit for bit; the
Poiseuille and Darcy-Brinkman slots meet the host test's bounds on the device.  No tolerance is new.
"""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

import caps_cases as cc
import forcing_cases as fc
from conftest import GOLD, PKG
from lbm_amd import io as lio
from test_forcing_host import BRINKMAN_BOUND, CROSS_BOUND, POISEUILLE_BOUND
from test_gpu_thermal import MODES, _mode

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)      # flow steps before each kick: both lattices of the pair get kicked
GRIDS = [(37, 19), (64, 32)]
FORMS = ["uniform", "fields"]

_b32, _same = fc.b32, fc.same


def _problem(nx, ny, seed, iters=8, obstacles=0.1):
    """About 10 % random obstacles on a 5 % perturbed equilibrium."""
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx)) < obstacles).astype(np.uint8)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    return p, obst, cells


def _whole(nx, ny, form, seed=1, index=0):
    return fc.box_zone(index, (0, 0, nx, ny), seed, form == "fields", idle=0.2)


def _apply_and_check(e, obst, zones, n=1.0, what="", impulse=True, nan_as_one=False):
    """One forcing_apply: the handle's store() against the restatement of what it stored just before, the
    impulse against the restatement's terms.  Returns the kicked cells."""
    before = e.store(n_av=0)[0]
    imp = e.forcing_apply(n, impulse=impulse)
    got = e.store(n_av=0)[0]
    want, terms = fc.restate(before, obst, zones, n)
    cc.assert_same_bits(got, want, str(what), nan_as_one=nan_as_one)
    assert _same(got[..., 0], before[..., 0]), what                               # the rest speed
    if impulse:
        assert imp.shape == (8, 2)
        fc.check_impulse(imp, terms, what)
    else:
        assert imp is None
    return got


def _sequence(e, p, obst, cells0, zones, what="", chunks=CHUNKS):
    e.load_cells(cells0)
    e.forcing_clear()
    fc.set_zones(e, zones)
    assert e.forcing_zones() == sorted(z["index"] for z in zones)
    cells = None
    for i, c in enumerate(chunks):
        e.run_steps(c, accelerate_first=i == 0)
        cells = _apply_and_check(e, obst, zones, (1.0, float(c), 0.5)[i % 3], (what, i), impulse=i % 2 == 0)
    return cells


# ---------------------------------------------------------- kick, bitwise ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_kick_sequences_bitwise(gpu_lib, nx, ny, form):
    p, obst, cells0 = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        kicked = _sequence(e, p, obst, cells0, [_whole(nx, ny, form)], (nx, ny, form))
        assert not _same(kicked, cells0) and obst.any()


@pytest.mark.parametrize("mode", MODES)
def test_kick_every_kernel_bitwise(gpu_lib, mode):
    kw, want = _mode(gpu_lib, mode)
    p, obst, cells0 = _problem(132, 70, 7)
    with gpu_lib.Engine(p, obst, **kw) as e:
        for form in FORMS:
            _sequence(e, p, obst, cells0, [_whole(132, 70, form), fc.box_zone(3, (5, 9, 70, 33), 4, form != "fields")],
                      (mode, form))
        assert e.kernel_in_use() in want
        assert e.numerics() == ("tolerance" if mode == "stream_tolerance" else "bitwise")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny", GRIDS + [(38, 7)])
def test_boxes_cut_the_quads_every_way(gpu_lib, nx, ny, form):
    """The whole domain, (x0, w) = (1, 5), (4, 4), (3, 2), (nx - 3, 3) and a single cell; 37 and 38 are no
    multiples of 4."""
    p, obst, cells0 = _problem(nx, ny, nx + ny)
    boxes = fc.boxes2d(nx, ny)
    assert len(boxes) == 6
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        for i, box in enumerate(boxes):
            e.forcing_clear()
            z = fc.box_zone(i % 8, box, 10 * nx + i, form == "fields")
            fc.set_zones(e, [z])
            sl = (slice(box[1], box[1] + box[3]), slice(box[0], box[0] + box[2]))
            before = e.store(n_av=0)[0]
            got = _apply_and_check(e, obst, [z], 1.0 + i, (nx, ny, box, form))
            outside = np.ones((ny, nx), bool)
            outside[sl] = False
            assert _same(got[outside], before[outside])
            assert obst[sl].all() or not _same(got[sl], before[sl])


def test_overlapping_zones_apply_in_index_order(gpu_lib):
    nx, ny = 37, 19
    p, obst, cells0 = _problem(nx, ny, 3)
    zones = [fc.box_zone(5, (2, 3, 20, 10), 1, False), fc.box_zone(2, (10, 6, 25, 12), 2, True),
             fc.zone(7, (12, 7), (4, 3), 1.0, (0.02, -0.01))]
    with gpu_lib.Engine(p, obst) as e, gpu_lib.Engine(p, obst) as e2:
        e.load_cells(cells0)
        e2.load_cells(cells0)
        for z in zones:
            e.forcing_zone(**z)
        for z in zones[::-1]:
            e2.forcing_zone(**z)                                 # the order of the calls does not matter
        got = _apply_and_check(e, obst, zones, 1.0, "overlap")
        imp = e.forcing_apply(2.0, impulse=True)
        e2.forcing_apply(1.0)
        assert _same(e2.store(n_av=0)[0], got)
        imp2 = e2.forcing_apply(2.0, impulse=True)
        assert np.array_equal(imp.view(np.uint64), imp2.view(np.uint64)) and imp[[2, 5, 7]].all()     # identical bits
        # the reverse order gives another lattice: the order is part of the definition
        other, _ = fc.restate(cells0, obst, [dict(z, index=7 - z["index"]) for z in zones], 1.0)
        assert not _same(other, got)
        # a zone that is set again replaces the old one; an extent 0 removes it
        e.forcing_zone(5, (0, 0), (0, 4))
        assert e.forcing_zones() == [2, 7]
        e.forcing_zone(2, (1, 1), (3, 3), lam=0.5)
        zones = [fc.zone(2, (1, 1), (3, 3), 0.5), zones[2]]
        _apply_and_check(e, obst, zones, 1.0, "replaced")


def test_idle_part_of_a_fields_zone_keeps_every_bit(gpu_lib):
    nx, ny = 64, 32
    p, obst, cells0 = _problem(nx, ny, 12)
    cells0[..., 3] = np.float32(-0.0)                            # the W speed: every live cell gains x momentum
    lam = np.zeros((ny, nx), np.float32)
    lam[:, 8:40] = 0.3
    f = np.zeros((ny, nx), np.float32)
    f[4:9, 2:11] = 1e-3
    z = fc.zone(0, (0, 0), (nx, ny), lam, (0.02, 0.0), (f, 0.0))
    idle = (lam == 0) & (f == 0)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        fc.set_zones(e, [z])
        got = _apply_and_check(e, obst, [z], 1.0, "idle part")
        assert _same(got[idle], cells0[idle]) and (_b32(got[idle][:, 3]) == 0x80000000).all()
        live = ~idle & (obst == 0)
        assert idle.any() and live.any() and (_b32(got[live][:, 3]) != 0x80000000).all()


# --------------------------------------------- continuation, decomposition ----

def _continuation(n, p, obst, cells0, zones, kw, what):
    """Kick, then run k steps -- on the kicked handle and on a second one that loaded the kicked cells -- for
    k = 1, 2, 5 and the fused depth + 1.  Returns the lattice after k = 5."""
    with n.Engine(p, obst, **kw) as a, n.Engine(p, obst, **kw) as b:
        a.load_cells(cells0)
        fc.set_zones(a, zones)
        a.run_steps(3, accelerate_first=True)
        after5 = None
        for i, k in enumerate((1, 2, 5, a.steps_per_launch() + 1)):
            kicked = _apply_and_check(a, obst, zones, 1.0 + i % 2, (what, k))
            b.load_cells(kicked)
            a.run_steps(k)
            b.run_steps(k)
            cells, av = a.store(n_av=k)
            cells_b, av_b = b.store(n_av=k)
            cc.assert_same_bits(cells, cells_b, str((what, k)))
            assert np.array_equal(_b32(av), _b32(av_b)) and av.size == k, (what, k)
            if i == 2:
                after5 = cells
        return after5


def _crossing_zones(nx, ny):
    """A fields-form box across every sub-domain border of the 1 x 2, 2 x 1 and 2 x 2 grids, under a uniform
    whole-domain zone."""
    return [_whole(nx, ny, "uniform", 6), fc.box_zone(1, (nx // 2 - 5, ny // 2 - 4, 11, 9), 8, True)]


@pytest.mark.parametrize("mode", MODES)
def test_a_run_continues_from_the_kicked_lattice(gpu_lib, mode):
    kw, _ = _mode(gpu_lib, mode)
    p, obst, cells0 = _problem(132, 70, 17, iters=40)
    _continuation(gpu_lib, p, obst, cells0, _crossing_zones(132, 70), kw, mode)


@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for nx, ny in GRIDS:
        p, obst, cells0 = _problem(nx, ny, 31 + nx, iters=40)
        cells = _continuation(gpu_lib, p, obst, cells0, _crossing_zones(nx, ny), dict(parts=1), "single")
        for a in (obst, cells0, cells):
            a.setflags(write=False)
        out[(nx, ny)] = (p, obst, cells0, cells)
    return out


@pytest.mark.parametrize("grid", [(1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_decomposed_handles_kick_and_continue_bitwise(gpu_lib, single, nx, ny, grid):
    p, obst, cells0, ref = single[(nx, ny)]
    kw = dict(parts=grid[0] * grid[1], grid=grid, devices=[0])
    with gpu_lib.Engine(p, obst, **kw) as e:
        rects = e.local_rects()
        assert len(rects) == grid[0] * grid[1]
        if grid[1] == 2 and nx == 37:
            assert any(r[0] % 4 for r in rects)              # a sub-domain off the 16-B alignment
        x0, y0, w, h = fc.box_of(_crossing_zones(nx, ny)[1])
        for rx, ry, rw, rh in rects:                          # the box meets every sub-domain
            assert x0 < rx + rw and rx < x0 + w and y0 < ry + rh and ry < y0 + h
    cells = _continuation(gpu_lib, p, obst, cells0, _crossing_zones(nx, ny), kw, (nx, ny, grid))
    assert _same(cells, ref)                                 # a decomposed handle's bits are the single-domain handle's


# ------------------------------------------------------ degenerate shapes ----

@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 1), (1, 5), (4, 1), (5, 3), (8, 2)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny):
    p, obst, cells0 = _problem(nx, ny, 5 + nx + 10 * ny, obstacles=0.2 if nx * ny > 4 else 0.0)
    with gpu_lib.Engine(p, obst) as e:
        for form in FORMS:
            _sequence(e, p, obst, cells0, [_whole(nx, ny, form)], (nx, ny, form), chunks=(3, 2, 1))


def test_all_obstacle_grid_keeps_every_bit(gpu_lib):
    p, _, cells0 = _problem(13, 6, 2)
    cells0[..., 3] = np.float32(-0.0)
    obst = np.ones((6, 13), np.uint8)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        for form in FORMS:
            zones = [_whole(13, 6, form)]
            e.forcing_clear()
            fc.set_zones(e, zones)
            assert _same(_apply_and_check(e, obst, zones, 1.0, "all obstacles"), cells0)
            assert not e.forcing_apply(1.0, impulse=True).any()


# -------------------------------------------------------- past the clamps ----

@pytest.mark.parametrize("form", FORMS)
def test_whole_domain_zone__forcing_zone_trip2_of_2(gpu_lib, form):
    """4098 x 2047: 2 098 175 quads, a second trip of 1023 quads of the last row ending on the ragged
    two-cell quad (tests/caps_cases.py)."""
    nx, ny = cc.BIG_NX, cc.BIG_NY
    rng = np.random.default_rng(4098)
    p = lio.Params(nx, ny, 4, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx), dtype=np.float32) < 0.1).astype(np.uint8)
    last = cc.quad_last_trip_mask(nx, ny)
    obst[ny - 1, [8, 9, nx - 2]] = 1
    obst[ny - 1, 1000:1004] = 0
    cells0 = (lio.init_cells(p) * (np.float32(0.875) + np.float32(0.25) * rng.random((ny, nx, 9), dtype=np.float32)))
    cells0 = cells0.astype(np.float32)
    assert obst[last].any() and (obst[last] == 0).any()
    if form == "fields":
        lam = (np.float32(0.5) * rng.random((ny, nx), dtype=np.float32)).astype(np.float32)
        z = fc.zone(0, (0, 0), (nx, ny), lam, (0.02, -0.01), (1e-3, 2e-3))
    else:
        z = fc.zone(0, (0, 0), (nx, ny), 0.25, (0.02, -0.01), (1e-3, 2e-3))
    where = lambda y, x, k: cc.quad_where(nx, ny, y, x) + f", speed {k}"          # noqa: E731
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        fc.set_zones(e, [z])
        imp = e.forcing_apply(1.0, impulse=True)
        got = e.store(n_av=0)[0]
        again = e.forcing_apply(0.0, impulse=True)
    want, terms = fc.restate(cells0, obst, [z], 1.0)
    cc.assert_touched(want, cells0, last[..., None], "kick")
    cc.assert_same_bits(got, want, f"forcing_zone {form}", where)
    fc.check_impulse(imp, terms, form)
    for c in range(2):                                       # the second trip is folded in
        assert abs(float(terms[0][..., c][last].astype(np.float64).sum())) > 100 * fc.fold_bound(terms[0][..., c])
    assert not again.any()


# ------------------------------------------------------------ hard states ----

QNAN, QNAN_NEG = 0x7FC00123, 0xFFC00456


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nx,ny,split", [(37, 19, False), (64, 32, False), (37, 19, True)])
def test_hard_states(gpu_lib, nx, ny, split, form):
    """A fluid cell of density zero, subnormal populations, NaN (with payloads), Inf and 2^100 under
    obstacles: the restatement's bits, NaN payloads compared as one; obstacle cells keep theirs raw.  No index
    depends on a value: nothing can fault."""
    p, obst, cells0 = _problem(nx, ny, 77 + nx)
    rng = np.random.default_rng(5)
    fl, ob = np.argwhere(obst == 0), np.argwhere(obst != 0)
    pick = lambda a, n: a[rng.choice(len(a), n, replace=False)]          # noqa: E731
    for y, x in pick(fl, 6):
        cells0[y, x] = 0.0
    for y, x in pick(fl, 12):
        cells0[y, x] *= np.float32(2.0 ** -130)                            # subnormal populations
    for y, x in pick(fl, 4):
        cells0[y, x, 1::2] = np.float32(-0.0)
    raw = cells0.view(np.uint32)
    for i, (y, x) in enumerate(pick(ob, 9)):
        if i % 3 == 0:
            raw[y, x, :] = QNAN if i % 2 else QNAN_NEG
        elif i % 3 == 1:
            cells0[y, x, ::2] = np.inf
            cells0[y, x, 1::2] = -np.inf
        else:
            cells0[y, x] = np.float32(2.0 ** 100)
    zones = [_whole(nx, ny, form, 9), fc.zone(4, (3, 2), (nx - 6, ny - 4), 1.0, (0.03, 0.01))]
    kw = dict(parts=2, grid=(1, 2), devices=[0]) if split else {}
    with np.errstate(all="ignore"), gpu_lib.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        fc.set_zones(e, zones)
        before = e.store(n_av=0)[0]
        assert np.array_equal(_b32(before), _b32(cells0))
        got = _apply_and_check(e, obst, zones, 1.0, (nx, ny, split, form), nan_as_one=True)
        assert np.array_equal(_b32(got[obst != 0]), _b32(cells0[obst != 0]))          # payloads included
        assert np.isfinite(got[obst == 0]).all()


# --------------------------------------------------------------- contract ----

def test_forcing_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells0 = _problem(37, 19, 9)
    nan, inf = float("nan"), float("inf")
    f32p = ctypes.POINTER(ctypes.c_float)
    K = lambda *v: (ctypes.c_float * 5)(*v)                                       # noqa: E731
    good = K(0.1, 0.01, 0.0, 1e-4, 0.0)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE, parts=2, grid=(1, 2), devices=[0]) as e:
        L, h = e._L, e._h
        assert L.lbm_forcing_set_zone(None, 0, 0, 0, 4, 4, None, good) == n.LBM_E_INVALID
        assert L.lbm_forcing_clear(None) == n.LBM_E_INVALID and L.lbm_forcing_zones(None, None, None) == n.LBM_E_INVALID
        assert L.lbm_forcing_apply(None, 1.0, None) == n.LBM_E_INVALID
        assert L.lbm_forcing_set_zone(h, 1, 2, 3, 20, 10, None, good) == n.LBM_OK       # zones may be set before the load
        assert L.lbm_forcing_apply(h, 1.0, None) == n.LBM_E_STATE                    # before the lattice is loaded
        cells0[..., 4] = np.float32(-0.0)
        e.load_cells(cells0)
        launches = lambda: sum(k["launches"] for k in e.profile_summary())          # noqa: E731
        before = launches()
        arr = np.full((10, 20), 0.1, np.float32)
        arr[3, 4] = nan
        neg = np.full((10, 20), 0.1, np.float32)
        neg[9, 19] = -1e-6
        T = lambda *ptrs: (f32p * 5)(*ptrs)                                          # noqa: E731
        bad_zones = [
            (-1, 0, 0, 4, 4, None, good), (8, 0, 0, 4, 4, None, good),               # the index
            (0, 30, 0, 8, 4, None, good), (0, 0, 16, 4, 4, None, good), (0, -1, 0, 4, 4, None, good),   # the box
            (0, 0, 0, -4, 4, None, good), (0, 0, 0, 4, -1, None, good),
            (0, 0, 0, 4, 4, None, K(nan, 0, 0, 0, 0)), (0, 0, 0, 4, 4, None, K(0.1, inf, 0, 0, 0)),
            (0, 0, 0, 4, 4, None, K(0.1, 0, 0, 0, -inf)), (0, 0, 0, 4, 4, None, K(-0.5, 0, 0, 0, 0)),
            (1, 2, 3, 20, 10, T(None, None, n._ptr(arr), None, None), good),
            (1, 2, 3, 20, 10, T(n._ptr(neg), None, None, None, None), good),
        ]
        for bad in bad_zones:
            assert L.lbm_forcing_set_zone(h, *bad) == n.LBM_E_INVALID, bad[:5]
            assert L.lbm_last_error(h)
        assert b"lam" in L.lbm_last_error(h)
        assert e.forcing_zones() == [1]                                              # the zones set before stay
        for bad in (nan, inf, -inf, -1.0):
            assert L.lbm_forcing_apply(h, bad, None) == n.LBM_E_INVALID
        assert b"steps" in L.lbm_last_error(h)
        assert launches() == before and _same(e.store(n_av=0)[0], cells0)
        # steps == 0: LBM_OK, no launch, every bit stays (an added zero would flip the -0.0f)
        assert L.lbm_forcing_apply(h, 0.0, None) == n.LBM_OK and L.lbm_forcing_apply(h, -0.0, None) == n.LBM_OK
        assert launches() == before and _same(e.store(n_av=0)[0], cells0)
        assert not [k for k in e.profile_summary() if k["name"] == "forcing"]
        with pytest.raises(ValueError):
            e.forcing_zone(0, (0, 0, 0), (4, 4))
        with pytest.raises(ValueError):
            e.forcing_zone(0, (0, 0), (4, 4), lam=np.zeros((3, 3), np.float32))
        # one launch per zone and intersecting part: zone 1 (columns 2 .. 21) meets both parts of 1 x 2, zone 3
        # (columns 30 .. 36) only the second
        rects = e.local_rects()
        assert rects[0][2] in (18, 19) and len(rects) == 2
        zones = [fc.zone(1, (2, 3), (20, 10), 0.1, (0.01, 0.0), (1e-4, 0.0)), fc.zone(3, (30, 0), (7, 19), 0.0, None, (0.0, 1e-3))]
        e.forcing_zone(**zones[1])
        _apply_and_check(e, obst, zones, 1.0, "profile", impulse=False)
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["forcing"]["launches"] == 3 and prof["forcing"]["total_ms"] > 0
        _apply_and_check(e, obst, zones, 2.0, "profile", impulse=True)
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["forcing"]["launches"] == 6
        # no zone set: LBM_OK, no launch
        e.forcing_clear()
        assert e.forcing_zones() == []
        before, kept = launches(), e.store(n_av=0)[0]
        assert e.forcing_apply(1.0, impulse=True).tolist() == [[0.0, 0.0]] * 8
        assert launches() == before and _same(e.store(n_av=0)[0], kept)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:       # a handle that never sets a zone launches nothing new
        e.load_cells(cells0)
        e.run_steps(4, accelerate_first=True)
        assert e.forcing_apply(1.0) is None and e.forcing_zones() == []
        assert not [k for k in e.profile_summary() if "forcing" in k["name"]]


# --------------------------------------------- run_forced is its definition ----

def test_run_forced_equals_the_loop_over_the_two_calls(gpu_lib):
    p, obst, cells0 = _problem(64, 32, 3, iters=13)
    zones = _crossing_zones(64, 32)
    refs = {}
    for stride in (1, 3):
        with gpu_lib.Engine(p, obst) as e:                  # by hand
            e.load_cells(cells0)
            fc.set_zones(e, zones)
            av, done = [], 0
            while done < 13:
                n = min(stride, 13 - done)
                e.forcing_apply(n)
                e.run_steps(n, accelerate_first=done == 0)
                av.append(e.store(cells=False, n_av=n)[1].copy())
                done += n
            want = (e.store(n_av=0)[0], np.concatenate(av))
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            fc.set_zones(e, zones)
            av = e.run_forced(13, stride, accelerate_first=True)
            got = (e.store(n_av=0)[0], av)
            with pytest.raises(ValueError):
                e.run_forced(5, stride=0)
        assert all(_same(a, b) for a, b in zip(got, want)), stride
        refs[stride] = want
        with gpu_lib.Engine(p, obst) as e:                  # the zones are felt: the free run differs
            e.load_cells(cells0)
            e.run_steps(13, accelerate_first=True)
            assert not _same(e.store(n_av=0)[0], want[0])
    assert not _same(refs[1][0], refs[3][0])
    with gpu_lib.Engine(p, obst) as e, gpu_lib.Engine(p, obst) as b:
        e.load_cells(cells0)
        b.load_cells(cells0)
        fc.set_zones(e, zones)
        fc.set_zones(b, zones)
        hist = e.forcing_history(13, 5, stride=3)
        assert [s[0] for s in hist] == [5, 10, 13] and all(s[1].shape == (8, 2) for s in hist)
        want = []
        for chunk in (5, 5, 3):                             # chunks of 5 in strides of 3: 3 + 2, 3 + 2, 3
            total, done = np.zeros((8, 2)), 0
            while done < chunk:
                m = min(3, chunk - done)
                total += b.forcing_apply(m, impulse=True)
                b.run_steps(m)
                done += m
            want.append(total)
        for (_, got_sum), w in zip(hist, want):
            assert np.array_equal(got_sum.view(np.uint64), w.view(np.uint64))
        assert _same(e.store(n_av=0)[0], b.store(n_av=0)[0])


def test_run_forced_equals_the_cpu_loop_bitwise(gpu_lib):
    """50 steps at stride 1 on the default kernel: a fringe (lam = 1 towards a profile) in a periodic box with
    a porous block and a body force, against "lio.forcing_kick, oracle.step"."""
    nx, ny = 48, 24
    p, obst, cells0 = _problem(nx, ny, 21, iters=50)
    prof = (0.04 * np.sin(np.pi * (np.arange(ny) + 0.5) / ny)).astype(np.float32)
    zones = [fc.zone(0, (0, 0), (nx, ny), 0.0, None, (1e-5, 0.0)),
             fc.zone(1, (2, 0), (3, ny), 1.0, (np.repeat(prof[:, None], 3, axis=1), 0.0)),
             fc.zone(2, (20, 6), (9, 11), 0.05)]
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        fc.set_zones(e, zones)
        e.run_forced(50)
        cells = e.store(n_av=0)[0]
        assert e.kernel_in_use() in ("resident", "step2")
    want, _ = fc.cpu_forced(p, obst, cells0, zones, 50)
    cc.assert_same_bits(cells, want, "run_forced(50)")
    free, _ = fc.cpu_forced(p, obst, cells0, [], 50)
    assert not _same(want, free)


# ------------------------------------------------- physics on the device ----

@pytest.mark.parametrize("lam", [0.0, 0.01])
def test_slot_profiles_on_the_device(gpu_lib, lam):
    p, obst, cells0, zones = fc.slot(2, lam)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        fc.set_zones(e, zones)
        e.run_forced(fc.SLOT_STEPS - 50)
        hist = e.forcing_history(50, 50)
        cells = e.store(n_av=0)[0]
    err, across = fc.slot_profile_error(p, obst, cells, lam, 2)
    bound = POISEUILLE_BOUND if lam == 0 else BRINKMAN_BOUND[lam]
    print(f"slot on the device, lam = {lam}: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= bound and across <= CROSS_BOUND
    # the impulse per step: the body force f rho on every fluid cell, less what the drag takes back
    rho = cells.astype(np.float64).sum(-1)[obst == 0]
    per_step = hist[0][1][0] / 50
    u = lio.macroscopic(p, obst, cells)[1].astype(np.float64)[obst == 0]
    want = fc.SLOT_F * rho.sum() - lam * (rho * u).sum()
    print(f"impulse per step {per_step[1]!r}, f sum rho - lam sum rho u = {want!r}; across {per_step[0]!r}")
    assert abs(per_step[1] - want) <= 1e-3 * abs(fc.SLOT_F * rho.sum()) and abs(per_step[0]) <= 1e-3 * abs(want)
    assert hist[0][0] == 50 and not hist[0][1][1:].any()


# ----------------------------------------------------------------- runner ----

def test_runner_forcing_option(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    help_text = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--forcing" in help_text.stdout + help_text.stderr
    assert "--forcing-stride" in help_text.stdout + help_text.stderr
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "23"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    rows = [(0, 0, 0, 128, 128, 0.0, 0.0, 0.0, 1e-5, 0.0), (3, 10, 20, 37, 50, 0.05, 0.0, 0.0, 0.0, 0.0),
            (1, 2, 0, 3, 128, 1.0, 0.03, -0.001, 0.0, 2e-6)]
    zfile = tmp_path / "zones.txt"
    zfile.write_text("# zone x0 y0 w h lam utx uty fx fy\n" + "".join(" ".join(repr(v) for v in r) + "\n" for r in rows))
    zones = [fc.zone(r[0], r[1:3], r[3:5], r[5], r[6:8], r[8:10]) for r in rows]
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file)]
    for stride in (1, 4):
        d = tmp_path / f"s{stride}"
        d.mkdir()
        r = subprocess.run(base + ["--forcing", str(zfile), "--forcing-stride", str(stride), "--out-dir", str(d)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
        final = (d / "final_state.dat").read_text()
        with gpu_lib.Engine(p, obst) as e:                   # the same forced run through the binding
            e.load_cells(lio.init_cells(p))
            fc.set_zones(e, zones)
            (_, total), = e.forcing_history(23, 23, stride, accelerate_first=True)
            cells = e.store(n_av=0)[0]
            e.load_cells(lio.init_cells(p))                  # and the free run, which must differ
            e.run_steps(23, accelerate_first=True)
            assert not _same(cells, e.store(n_av=0)[0])
        want = tmp_path / f"want{stride}.dat"
        assert lio.write_results(str(want), p, obst, cells)
        assert final == want.read_text()
        got = (d / "forcing.dat").read_text().split("\n")
        assert [l for l in got if l] == [f"{i} {total[i, 0]:.17g} {total[i, 1]:.17g}" for i in (0, 1, 3)]
    r = subprocess.run(base + ["--forcing", str(zfile), "--device", "cpu", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--forcing" in r.stderr
    bad = tmp_path / "bad.txt"
    bad.write_text("0 0 0 128 128 0.0 0.0 0.0 1e-5\n")                               # a number short
    r = subprocess.run(base + ["--forcing", str(bad), "--out-dir", str(tmp_path)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--forcing" in r.stderr
    bad.write_text("0 100 0 64 128 0.0 0.0 0.0 1e-5 0.0\n")                          # leaves the domain
    r = subprocess.run(base + ["--forcing", str(bad), "--out-dir", str(tmp_path)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "domain" in r.stderr
