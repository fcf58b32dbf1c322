"""The sub-grid model on the device, D3Q19 (lbm3d_sgs_*; include/lbm_sgs_hip.h, csrc/lbm3d_sgs.hip,
csrc/lbm_sgs.hpp); the 3-D twin of tests/test_gpu_sgs.py.

Bar: after every sgs_apply the stored lattice is BITWISE (uint32 patterns) the restatement (lio.sgs_filter3d)
of what the same handle stored just before, on both sides of the flow pair, for both numerics, both modes,
constant and array coefficients, a width that is no multiple of 4, one quad wide, fewer than four columns,
1, 2 and 3 z slabs and the boxes past the launch clamps; eddy_viscosity() and the statistics are the
restatement's; a run of 1, 2, 3 or 5 steps afterwards continues bit for bit as a second handle does that
loaded the filtered cells; run_les is the CPU loop bit for bit; the equivalence and the Smagorinsky slot meet
the host test's bounds on the device.  No tolerance is new.
"""
from __future__ import annotations

import math

import numpy as np
import pytest

import caps_cases as cc
import forcing_cases as fc
import sgs_cases as sc
from lbm_amd import io as lio
from lbm_amd import native
from oracle import oracle
from test_gpu_sgs import check_stats
from test_sgs_host import CROSS_BOUND, MODES, SLOT_BOUND, WAVE_BOUND

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)
GRIDS = [(13, 7, 5), (16, 8, 8), (4, 3, 3)]
FORMS = ["constant", "array"]
OMEGA = 1.85

_b32, _same = fc.b32, fc.same


def _problem(nx, ny, nz, seed, obstacles=0.1, walls=True):
    """The channel walls plus about 10 % random obstacles; populations perturbed by 5 %."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, OMEGA)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < obstacles).astype(np.uint8)
    if walls and ny > 2:
        obst |= lio.channel_obstacles3d(nx, ny, nz)
        obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    c0[obst != 0, 2::5] = np.float32(-0.0)
    return p, obst, c0


def _coef(grid, mode, form, seed=1):
    return sc.random_coef(tuple(grid)[::-1], mode, seed, form == "array", omega=OMEGA, idle=0.2)


def _apply_and_check(e, obst, mode, coef, n=1.0, what="", stats=True, where=None):
    before = e.store()[0]
    nut1 = e.eddy_viscosity()
    assert _same(e.store()[0], before), what                                      # the lattice is not touched
    assert _same(nut1, lio.sgs_filter3d(before, obst, OMEGA, mode, coef, 1.0)[1]), what
    st = e.sgs_apply(n, stats=stats)
    got = e.store()[0]
    want, nut, idle = lio.sgs_filter3d(before, obst, OMEGA, mode, coef, n, with_idle=True)
    cc.assert_same_bits(got, want, str(what), where)
    if stats:
        check_stats(st, nut, idle, what)
    else:
        assert st is None
    return got


def _sequence(e, obst, c0, mode, coef, what="", chunks=CHUNKS):
    e.load_cells(c0)
    e.sgs_model(mode, coef)
    cells = None
    for i, c in enumerate(chunks):
        e.run_steps(c)
        cells = _apply_and_check(e, obst, mode, coef, (1.0, float(c), 0.5)[i % 3], (what, i), stats=i % 2 == 0)
    return cells


# -------------------------------------------------------- filter, bitwise ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("numerics", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_filter_sequences_bitwise(gpu_lib, nx, ny, nz, numerics, mode, form):
    p, obst, c0 = _problem(nx, ny, nz, 7)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if numerics == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        out = _sequence(e, obst, c0, mode, _coef((nx, ny, nz), mode, form), (nx, ny, nz, numerics, mode, form))
        assert not _same(out, c0)


def test_wide_rows_cross_waves_and_blocks(gpu_lib):
    """nx = 300: more than one wave of quads per row and a ragged tail; nx = 258: a tail of two cells; nx = 3:
    one cell per lane."""
    for nx in (300, 258, 3):
        p, obst, c0 = _problem(nx, 5, 3, nx)
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            _sequence(e, obst, c0, "smagorinsky", _coef((nx, 5, 3), "smagorinsky", "array"), nx, chunks=(2, 1))


def test_idle_cells_keep_every_bit(gpu_lib):
    nx, ny, nz = 16, 8, 8
    p, obst, c0 = _problem(nx, ny, nz, 3)
    c0 = c0.copy()
    c0[..., 4] = np.float32(-0.0)
    w1 = np.full((nz, ny, nx), OMEGA, np.float32)
    w1[:, :, 4:11] = 1.3
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.sgs_model("omega", w1)
        got = _apply_and_check(e, obst, "omega", w1, 1.0, "idle part")
        idle = (w1 == np.float32(OMEGA)) | (obst != 0)
        assert _same(got[idle], c0[idle]) and (_b32(got[idle][:, 4]) == 0x80000000).all()
        assert (_b32(got[~idle][:, 4]) != 0x80000000).all()
        e.sgs_model("smagorinsky", 0.0)                          # Cs = 0: every cell is idle
        assert e.sgs_apply(2.0, stats=True) == (0, 0.0, 0.0) and _same(e.store()[0], got)
        assert not e.eddy_viscosity().any()


# --------------------------------------------- continuation, decomposition ----

def _continuation(n, p, obst, c0, mode, coef, kw, what):
    """Filter, then run k steps -- on the filtered handle and on a second one that loaded the filtered cells --
    for k = 1, 2, 3, 5: one-, two- and three-step passes all start from filtered ghost planes."""
    with n.Engine3D(p, obst, **kw) as a, n.Engine3D(p, obst, **kw) as b:
        a.load_cells(c0)
        a.sgs_model(mode, coef)
        a.run_steps(3)
        cells, forms = None, []
        for i, k in enumerate((1, 2, 3, 5)):
            filtered = _apply_and_check(a, obst, mode, coef, 1.0 + i % 2, (what, k))
            b.load_cells(filtered)
            a.run_steps(k)
            forms.append(a.run_stats()[:3])
            b.run_steps(k)
            cells, cells_b = a.store()[0], b.store()[0]
            cc.assert_same_bits(cells, cells_b, str((what, k)))
        return cells, forms


@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for grid in GRIDS[:2]:
        p, obst, c0 = _problem(*grid, 11)
        coef = _coef(grid, "smagorinsky", "array", 8)
        cells, _ = _continuation(gpu_lib, p, obst, c0, "smagorinsky", coef, dict(devices=[0]), "single")
        for a in (obst, c0, cells, coef):
            a.setflags(write=False)
        out[grid] = (p, obst, c0, coef, cells)
    return out


@pytest.mark.parametrize("numerics", ["bitwise", "tolerance"])
def test_a_run_continues_from_the_filtered_lattice(gpu_lib, numerics):
    p, obst, c0 = _problem(16, 8, 8, 19)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if numerics == "tolerance" else 0)
    _, forms = _continuation(gpu_lib, p, obst, c0, "omega", _coef((16, 8, 8), "omega", "array"), kw, numerics)
    assert forms[0] == (0, 0, 1) and forms[1] == (0, 1, 0)
    assert forms[2] in ((1, 0, 0), (0, 1, 1)) and sum(f[0] for f in forms) > 0


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("nx,ny,nz", GRIDS[:2])
def test_slabs_filter_and_continue_bitwise(gpu_lib, single, nx, ny, nz, parts):
    p, obst, c0, coef, ref = single[(nx, ny, nz)]
    kw = dict(parts=parts, devices=[0])
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        assert len(e.local_slabs()) == parts
    cells, _ = _continuation(gpu_lib, p, obst, c0, "smagorinsky", coef, kw, (nx, ny, nz, parts))
    assert _same(cells, ref)
    with gpu_lib.Engine3D(p, obst, **kw) as e:               # constant coefficient, the other mode
        _sequence(e, obst, c0, "omega", 1.2, (nx, ny, nz, parts, "constant"), chunks=(2, 1))


# -------------------------------------------------------- past the clamps ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("box", [cc.BOXES_STRIDED[0], cc.BOX_ROWS], ids=lambda b: "x".join(map(str, b)))
def test_whole_domain__sgs_filter3d_past_the_clamps(gpu_lib, box, form):
    """8 x 512 x 130: slab_grid is 1 x 128 x 128 blocks, planes 128 and 129 are a second trip of the plane loop;
    5 x 262200 x 1: gridDim.y is clamped and rows 262140 .. are a second trip of the row loop.  The reference
    is lbm3d_sgs_filter_ref, which tests/test_sgs_host.py holds to lio.sgs_filter3d bit for bit."""
    nx, ny, nz = box
    rng = np.random.default_rng(sum(box))
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, OMEGA)
    obst = (rng.random((nz, ny, nx), dtype=np.float32) < 0.1).astype(np.uint8)
    one = oracle.init_cells3d(lio.Params3D(1, 1, 1, 0, 0.1, 0.002, OMEGA)).reshape(19)
    c0 = (one * (np.float32(0.875) + np.float32(0.25) * rng.random((nz, ny, nx, 19), dtype=np.float32))).astype(np.float32)
    last = cc.slab_last_trip_mask(*box)
    assert last.any() and not last.all() and obst[last].any() and (obst[last] == 0).any()
    coef = (np.float32(0.05) + np.float32(0.3) * rng.random((nz, ny, nx), dtype=np.float32)) if form == "array" else 0.2
    gx, gy, gz = cc.slab_grid(*box)

    def where(zz, y, x, k):
        return (f"plane {zz}: trip {zz // gz} of the plane loop; row {y}: trip {y // (gy * cc.S3Y)} of the row loop; "
                f"lane {x // 4 % cc.S3X}, cell {x % 4}, speed {k}")
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        assert e.local_slabs() == [(0, nz)]
        e.load_cells(c0)
        e.sgs_model("smagorinsky", coef)
        nut1 = e.eddy_viscosity()
        st = e.sgs_apply(1.0, stats=True)
        got = e.store()[0]
    want, nut = native.sgs_filter3d_ref(c0, obst, OMEGA, "smagorinsky", coef, 1.0)
    cc.assert_touched(want, c0, last[..., None], "filter")
    cc.assert_same_bits(got, want, f"{box} sgs_filter3d {form}", where)
    assert _same(nut1, nut)
    live = nut[obst == 0].astype(np.float64)
    assert st[0] == live.size and st[2] == float(nut.max())
    assert abs(st[1] - math.fsum(live.tolist())) <= fc.fold_bound(live)
    assert float(nut[last].astype(np.float64).sum()) > 100 * fc.fold_bound(live)     # the second trip is folded in


# --------------------------------------------------------------- contract ----

def test_sgs_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(13, 7, 5, 9)
    nan, inf = float("nan"), float("inf")
    nut = np.full((5, 7, 13), 7, np.float32)
    with n.Engine3D(p, obst, parts=2, devices=[0]) as e:
        L, h = e._L, e._h
        assert L.lbm3d_sgs_set(None, 1, 0.1, None) == n.LBM_E_INVALID
        assert L.lbm3d_sgs_apply(None, 1.0, None) == n.LBM_E_INVALID
        assert L.lbm3d_sgs_store_nut(None, n._ptr(nut)) == n.LBM_E_INVALID
        assert L.lbm3d_sgs_set(h, 2, 1.3, None) == n.LBM_OK                          # a model may be set before the load
        assert L.lbm3d_sgs_apply(h, 1.0, None) == n.LBM_E_STATE                      # before the lattice is loaded
        assert L.lbm3d_sgs_store_nut(h, n._ptr(nut)) == n.LBM_E_STATE and (nut == 7).all()
        e.load_cells(c0)
        arr = np.full((5, 7, 13), 0.1, np.float32)
        arr[4, 6, 12] = inf
        for bad in ((3, 0.1, None), (1, -0.1, None), (1, nan, None), (1, 0.0, n._ptr(arr)), (2, 0.0, None),
                    (2, 2.0, None), (2, inf, None)):
            assert L.lbm3d_sgs_set(h, *bad) == n.LBM_E_INVALID, bad[:2]
            assert L.lbm3d_last_error(h)
        for bad in (nan, inf, -1.0):
            assert L.lbm3d_sgs_apply(h, bad, None) == n.LBM_E_INVALID
        assert L.lbm3d_sgs_apply(h, 0.0, None) == n.LBM_OK
        assert _same(e.store()[0], c0) and (_b32(c0) == 0x80000000).any()               # every bit, -0.0f included
        _apply_and_check(e, obst, "omega", float(np.float32(1.3)), 1.0, "kept")         # the model set before stays
        e.load_cells(c0)
        e.sgs_model("omega", 1.99)                               # three steps from 1.85 towards 1.99 overshoot 2
        assert L.lbm3d_sgs_apply(h, 3.0, None) == n.LBM_E_INVALID and b"(0, 2)" in L.lbm3d_last_error(h)
        assert _same(e.store()[0], c0)
        with pytest.raises(ValueError):
            e.sgs_model("smagorinsky", np.zeros((3, 3), np.float32))
        e.sgs_model("off")
        assert e.sgs_apply(1.0, stats=True) == (0, 0.0, 0.0) and _same(e.store()[0], c0)
        assert not e.eddy_viscosity().any()
    p1 = lio.Params3D(13, 7, 5, 0, 0.1, 0.002, 1.0)
    with n.Engine3D(p1, obst, devices=[0]) as e:             # omega = 1: nothing to rescale
        e.load_cells(c0)
        e.sgs_model("smagorinsky", 0.1)
        assert e._L.lbm3d_sgs_apply(e._h, 1.0, None) == n.LBM_E_INVALID
        assert b"omega = 1" in e._L.lbm3d_last_error(e._h) and _same(e.store()[0], c0)


# ------------------------------------------------- run_les is its definition ----

def test_run_les_equals_the_cpu_loop_bitwise(gpu_lib):
    p, obst, c0 = _problem(16, 8, 8, 21)
    zones = [fc.zone(0, (0, 0, 0), (16, 8, 8), 0.0, None, (1e-5, 0.0, 0.0)),
             fc.box_zone(1, (1, 1, 1, 13, 6, 6), 8, True)]
    cs = _coef((16, 8, 8), "smagorinsky", "array", 6)
    refs = {}
    for stride in (1, 3):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            e.load_cells(c0)
            fc.set_zones(e, zones)
            e.sgs_model("smagorinsky", cs)
            av = e.run_les(50, stride, forced=True)
            refs[stride] = e.store()[0]
            assert av.size == 0
            with pytest.raises(ValueError):
                e.run_les(5, accelerate_first=True)
        want, _ = sc.cpu_les(p, obst, c0, "smagorinsky", cs, 50, stride, zones)
        cc.assert_same_bits(refs[stride], want, f"run_les(50, {stride}) against the CPU loop")
    assert not _same(refs[1], refs[3])
    free, _ = fc.cpu_forced(p, obst, c0, zones, 50, dims=3)
    assert not _same(refs[1], free)                          # the model is felt
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        fc.set_zones(e, zones)
        e.sgs_model("smagorinsky", cs)
        hist = e.les_history(50, 20, forced=True)
        assert [s[0] for s in hist] == [20, 40, 50] and all(s[1] > 0 and 0 < s[2] <= s[3] for s in hist)
        assert _same(e.store()[0], refs[1])


# ------------------------------------------------- physics on the device ----

def test_equivalence_on_the_device(gpu_lib):
    def run(p, obst, cells0, steps):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            e.load_cells(cells0)
            e.sgs_model("omega", sc.WAVE_OMEGA1)
            e.run_les(steps)
            return e.store()[0]
    gap = sc.wave_gap(3, run=run)
    print(f"3-D equivalence on the device: max |filtered omega0 run - plain omega1 run| {gap:.3e}")
    assert gap <= WAVE_BOUND[3]


def test_smagorinsky_slot_on_the_device(gpu_lib):
    p, obst, c0, zones = sc.slot(3)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        fc.set_zones(e, zones)
        e.sgs_model("smagorinsky", sc.SLOT_CS)
        e.run_les(sc.SLOT_STEPS, forced=True)
        cells = e.store()[0]
    err, across = sc.slot_profile_error(p, obst, cells, 3)
    print(f"3-D Smagorinsky slot on the device: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= SLOT_BOUND and across <= CROSS_BOUND
