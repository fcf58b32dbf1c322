"""The sub-grid model on the device, D2Q9 (lbm_sgs_*; include/lbm_sgs_hip.h, csrc/lbm_sgs.hip, csrc/lbm_sgs.hpp).

Bar: after every sgs_apply the stored lattice is BITWISE (uint32 patterns) the restatement (lio.sgs_filter;
pinned by physics in tests/test_sgs_host.py) of what the same handle stored just before -- on both sides of
the flow pair, for every step kernel and both numerics, both modes, constant and array coefficients, widths
that are no multiple of 4, one quad wide, decomposed handles (a sub-domain off the 16-B alignment among them)
and a launch past the grid clamp; eddy_viscosity() is the restatement's nut at n = 1 and leaves the lattice
alone; the statistics' count and maximum are exact and the sum lies within the fold bound of math.fsum; a run
afterwards continues bit for bit, av_vels included, as a second handle does that loaded the filtered cells;
run_les is its definition and the CPU loop (oracle step + lio) bit for bit; the equivalence and the
Smagorinsky slot meet the host test's bounds on the device.  No tolerance is new.
"""
from __future__ import annotations

import ctypes
import math
import subprocess

import numpy as np
import pytest

import caps_cases as cc
import forcing_cases as fc
import sgs_cases as sc
from conftest import GOLD, PKG
from lbm_amd import io as lio
from lbm_amd import native
from test_sgs_host import CROSS_BOUND, MODES, SLOT_BOUND, WAVE_BOUND

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)      # flow steps before each application: both lattices of the pair get filtered
GRIDS = [(37, 19), (64, 32), (4, 6)]
FORMS = ["constant", "array"]
KERNELS = ["auto", "resident", "stream", "stream_tolerance", "step2", "vec4"]
OMEGA = 1.85

_b32, _same = fc.b32, fc.same


def _kernel(n, mode):
    return {
        "auto": (dict(), ("resident", "step2")),
        "resident": (dict(kernel=n.KERNEL_RESIDENT), ("resident",)),
        "stream": (dict(kernel=n.KERNEL_STREAM), ("stream",)),
        "stream_tolerance": (dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE), ("stream",)),
        "step2": (dict(kernel=n.KERNEL_STEP2), ("step2",)),
        "vec4": (dict(kernel=n.KERNEL_VEC4, flags=n.FLAG_ONE_STEP), ("vec4",)),
    }[mode]


def _problem(nx, ny, seed, iters=8, obstacles=0.1):
    """About 10 % random obstacles on a 5 % perturbed equilibrium."""
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, OMEGA)
    obst = (rng.random((ny, nx)) < obstacles).astype(np.uint8)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    return p, obst, cells


def _coef(shape, mode, form, seed=1):
    return sc.random_coef(shape, mode, seed, form == "array", omega=OMEGA, idle=0.2)


def check_stats(stats, nut, idle, what=""):
    """(cells, sum, max) of one application against the restatement's nut and idle map."""
    cells, total, peak = lio.sgs_stats(nut, idle)
    live = nut[~idle].astype(np.float64)
    assert stats[0] == cells and stats[2] == peak, (what, stats, cells, peak)
    assert abs(stats[1] - math.fsum(live.tolist())) <= fc.fold_bound(live), (what, stats[1], total)


def _apply_and_check(e, obst, mode, coef, n=1.0, what="", stats=True):
    """One sgs_apply: the handle's store() against the restatement of what it stored just before, the
    eddy viscosity and the statistics against the restatement's.  Returns the filtered cells."""
    before = e.store(n_av=0)[0]
    nut1 = e.eddy_viscosity()
    assert _same(e.store(n_av=0)[0], before), what                               # the lattice is not touched
    assert _same(nut1, lio.sgs_filter(before, obst, OMEGA, mode, coef, 1.0)[1]), what
    st = e.sgs_apply(n, stats=stats)
    got = e.store(n_av=0)[0]
    want, nut, idle = lio.sgs_filter(before, obst, OMEGA, mode, coef, n, with_idle=True)
    cc.assert_same_bits(got, want, str(what))
    if stats:
        check_stats(st, nut, idle, what)
    else:
        assert st is None
    return got


def _sequence(e, obst, cells0, mode, coef, what="", chunks=CHUNKS):
    e.load_cells(cells0)
    e.sgs_model(mode, coef)
    cells = None
    for i, c in enumerate(chunks):
        e.run_steps(c, accelerate_first=i == 0)
        cells = _apply_and_check(e, obst, mode, coef, (1.0, float(c), 0.5)[i % 3], (what, i), stats=i % 2 == 0)
    return cells


# -------------------------------------------------------- filter, bitwise ----

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_filter_sequences_bitwise(gpu_lib, nx, ny, mode, form):
    p, obst, cells0 = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        out = _sequence(e, obst, cells0, mode, _coef((ny, nx), mode, form), (nx, ny, mode, form))
        assert not _same(out, cells0)


@pytest.mark.parametrize("kernel", KERNELS)
def test_filter_every_kernel_bitwise(gpu_lib, kernel):
    kw, want = _kernel(gpu_lib, kernel)
    p, obst, cells0 = _problem(132, 70, 7)
    with gpu_lib.Engine(p, obst, **kw) as e:
        for mode, form in (("smagorinsky", "array"), ("omega", "constant")):
            _sequence(e, obst, cells0, mode, _coef((70, 132), mode, form), (kernel, mode, form))
        assert e.kernel_in_use() in want
        assert e.numerics() == ("tolerance" if kernel == "stream_tolerance" else "bitwise")


def test_idle_cells_keep_every_bit(gpu_lib):
    nx, ny = 64, 32
    p, obst, cells0 = _problem(nx, ny, 12)
    cells0[..., 3] = np.float32(-0.0)
    cs = np.zeros((ny, nx), np.float32)
    cs[:, 8:42] = 0.2
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.sgs_model("smagorinsky", cs)
        got = _apply_and_check(e, obst, "smagorinsky", cs, 1.0, "idle part")
        idle = (cs == 0) | (obst != 0)
        assert _same(got[idle], cells0[idle]) and (_b32(got[idle][:, 3]) == 0x80000000).all()
        assert (_b32(got[~idle][:, 3]) != 0x80000000).all()
        e.sgs_model("omega", OMEGA)                              # the handle's own rate: every cell is idle
        assert e.sgs_apply(2.0, stats=True) == (0, 0.0, 0.0) and _same(e.store(n_av=0)[0], got)
        assert not e.eddy_viscosity().any()


def test_two_handles_return_identical_statistics(gpu_lib):
    p, obst, cells0 = _problem(37, 19, 3)
    cs = _coef((19, 37), "smagorinsky", "array", 4)
    out = []
    for _ in range(2):
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            e.sgs_model("smagorinsky", cs)
            out.append(e.sgs_apply(1.0, stats=True))
    assert out[0] == out[1] and out[0][0] > 0 and out[0][1] > 0


# --------------------------------------------- continuation, decomposition ----

def _continuation(n, p, obst, cells0, mode, coef, kw, what):
    """Filter, then run k steps -- on the filtered handle and on a second one that loaded the filtered cells --
    for k = 1, 2, 5 and the fused depth + 1.  Returns the lattice after k = 5."""
    with n.Engine(p, obst, **kw) as a, n.Engine(p, obst, **kw) as b:
        a.load_cells(cells0)
        a.sgs_model(mode, coef)
        a.run_steps(3, accelerate_first=True)
        after5 = None
        for i, k in enumerate((1, 2, 5, a.steps_per_launch() + 1)):
            filtered = _apply_and_check(a, obst, mode, coef, 1.0 + i % 2, (what, k))
            b.load_cells(filtered)
            a.run_steps(k)
            b.run_steps(k)
            cells, av = a.store(n_av=k)
            cells_b, av_b = b.store(n_av=k)
            cc.assert_same_bits(cells, cells_b, str((what, k)))
            assert np.array_equal(_b32(av), _b32(av_b)) and av.size == k, (what, k)
            if i == 2:
                after5 = cells
        return after5


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_run_continues_from_the_filtered_lattice(gpu_lib, kernel):
    kw, _ = _kernel(gpu_lib, kernel)
    p, obst, cells0 = _problem(132, 70, 17, iters=40)
    _continuation(gpu_lib, p, obst, cells0, "smagorinsky", _coef((70, 132), "smagorinsky", "array"), kw, kernel)


@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for nx, ny in GRIDS[:2]:
        p, obst, cells0 = _problem(nx, ny, 31 + nx, iters=40)
        coef = _coef((ny, nx), "omega", "array", 8)
        cells = _continuation(gpu_lib, p, obst, cells0, "omega", coef, dict(parts=1), "single")
        for a in (obst, cells0, cells, coef):
            a.setflags(write=False)
        out[(nx, ny)] = (p, obst, cells0, coef, cells)
    return out


@pytest.mark.parametrize("grid", [(1, 2), (2, 2)])
@pytest.mark.parametrize("nx,ny", GRIDS[:2])
def test_decomposed_handles_filter_and_continue_bitwise(gpu_lib, single, nx, ny, grid):
    p, obst, cells0, coef, ref = single[(nx, ny)]
    kw = dict(parts=grid[0] * grid[1], grid=grid, devices=[0])
    with gpu_lib.Engine(p, obst, **kw) as e:
        rects = e.local_rects()
        assert len(rects) == grid[0] * grid[1]
        if nx == 37:
            assert any(r[0] % 4 for r in rects)              # a sub-domain off the 16-B alignment
    cells = _continuation(gpu_lib, p, obst, cells0, "omega", coef, kw, (nx, ny, grid))
    assert _same(cells, ref)                                 # a decomposed handle's bits are the single-domain handle's
    with gpu_lib.Engine(p, obst, **kw) as e:                 # constant coefficient, Smagorinsky, statistics per part
        _sequence(e, obst, cells0, "smagorinsky", 0.17, (nx, ny, grid, "constant"), chunks=(2, 1))


# -------------------------------------------------------- past the clamp ----

@pytest.mark.parametrize("form", FORMS)
def test_whole_domain__sgs_filter_trip2_of_2(gpu_lib, form):
    """4098 x 2047: 2 098 175 quads, a second trip of 1023 quads of the last row ending on the ragged two-cell
    quad (tests/caps_cases.py).  The reference is lbm_sgs_filter_ref, which tests/test_sgs_host.py holds to
    lio.sgs_filter bit for bit."""
    nx, ny = cc.BIG_NX, cc.BIG_NY
    rng = np.random.default_rng(4098)
    p = lio.Params(nx, ny, 4, 10, 0.1, 0.005, OMEGA)
    obst = (rng.random((ny, nx), dtype=np.float32) < 0.1).astype(np.uint8)
    last = cc.quad_last_trip_mask(nx, ny)
    obst[ny - 1, [8, 9, nx - 2]] = 1
    obst[ny - 1, 1000:1004] = 0
    cells0 = (lio.init_cells(p) * (np.float32(0.875) + np.float32(0.25) * rng.random((ny, nx, 9), dtype=np.float32)))
    cells0 = cells0.astype(np.float32)
    assert obst[last].any() and (obst[last] == 0).any()
    coef = (np.float32(0.05) + np.float32(0.3) * rng.random((ny, nx), dtype=np.float32)) if form == "array" else 0.2
    where = lambda y, x, k: cc.quad_where(nx, ny, y, x) + f", speed {k}"          # noqa: E731
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.sgs_model("smagorinsky", coef)
        nut1 = e.eddy_viscosity()
        st = e.sgs_apply(1.0, stats=True)
        got = e.store(n_av=0)[0]
        again = e.sgs_apply(0.0, stats=True)
    want, nut = native.sgs_filter_ref(cells0, obst, OMEGA, "smagorinsky", coef, 1.0)
    cc.assert_touched(want, cells0, last[..., None], "filter")
    cc.assert_same_bits(got, want, f"sgs_filter {form}", where)
    assert _same(nut1, nut)
    live = nut[obst == 0].astype(np.float64)
    assert st[0] == live.size and st[2] == float(nut.max())
    assert abs(st[1] - math.fsum(live.tolist())) <= fc.fold_bound(live)
    assert float(nut[last].astype(np.float64).sum()) > 100 * fc.fold_bound(live)     # the second trip is folded in
    assert again == (0, 0.0, 0.0)


# --------------------------------------------------------------- contract ----

def test_sgs_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells0 = _problem(37, 19, 9)
    nan, inf = float("nan"), float("inf")
    stats = (ctypes.c_double * 3)(7, 7, 7)
    nut = np.full((19, 37), 7, np.float32)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE, parts=2, grid=(1, 2), devices=[0]) as e:
        L, h = e._L, e._h
        assert L.lbm_sgs_set(None, 1, 0.1, None) == n.LBM_E_INVALID
        assert L.lbm_sgs_apply(None, 1.0, None) == n.LBM_E_INVALID and L.lbm_sgs_store_nut(None, n._ptr(nut)) == n.LBM_E_INVALID
        assert L.lbm_sgs_set(h, 1, 0.1, None) == n.LBM_OK                          # a model may be set before the load
        assert L.lbm_sgs_apply(h, 1.0, None) == n.LBM_E_STATE                      # before the lattice is loaded
        assert L.lbm_sgs_store_nut(h, n._ptr(nut)) == n.LBM_E_STATE and (nut == 7).all()
        cells0[..., 4] = np.float32(-0.0)
        e.load_cells(cells0)
        launches = lambda: sum(k["launches"] for k in e.profile_summary())          # noqa: E731
        before = launches()
        arr = np.full((19, 37), 0.1, np.float32)
        arr[3, 4] = nan
        neg = np.full((19, 37), 0.1, np.float32)
        neg[18, 36] = -1e-6
        for bad in ((3, 0.1, None), (-1, 0.1, None), (1, -0.1, None), (1, nan, None), (1, inf, None),
                    (1, 0.0, n._ptr(arr)), (1, 0.0, n._ptr(neg)), (2, 0.0, None), (2, 2.0, None), (2, nan, None),
                    (2, 0.0, n._ptr(np.full((19, 37), 2.5, np.float32)))):
            assert L.lbm_sgs_set(h, *bad) == n.LBM_E_INVALID, bad[:2]
            assert L.lbm_last_error(h)
        for bad in (nan, inf, -inf, -1.0):
            assert L.lbm_sgs_apply(h, bad, stats) == n.LBM_E_INVALID
        assert b"steps" in L.lbm_last_error(h)
        assert launches() == before and _same(e.store(n_av=0)[0], cells0)
        # the model set before is still there: Smagorinsky 0.1
        _apply_and_check(e, obst, "smagorinsky", float(np.float32(0.1)), 1.0, "kept")
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["sgs"]["launches"] == 2 and prof["sgs"]["total_ms"] > 0        # one launch per part
        e.load_cells(cells0)
        before = launches()
        # steps == 0: LBM_OK, no launch, every bit stays (an added zero would flip the -0.0f)
        assert L.lbm_sgs_apply(h, 0.0, stats) == n.LBM_OK and list(stats) == [0.0, 0.0, 0.0]
        assert L.lbm_sgs_apply(h, -0.0, None) == n.LBM_OK
        assert launches() == before and _same(e.store(n_av=0)[0], cells0)
        # a rate out of range at apply: three steps from 1.85 towards 1.99 overshoot 2; one step does not
        e.sgs_model("omega", 1.99)
        assert L.lbm_sgs_apply(h, 3.0, None) == n.LBM_E_INVALID and b"(0, 2)" in L.lbm_last_error(h)
        assert launches() == before and _same(e.store(n_av=0)[0], cells0)
        _apply_and_check(e, obst, "omega", float(np.float32(1.99)), 1.0, "in range")
        with pytest.raises(ValueError):
            e.sgs_model("wale", 0.1)
        with pytest.raises(ValueError):
            e.sgs_model("smagorinsky", np.zeros((3, 3), np.float32))
        # OFF, then apply: LBM_OK, no launch
        e.sgs_model("off")
        before, kept = launches(), e.store(n_av=0)[0]
        assert e.sgs_apply(1.0, stats=True) == (0, 0.0, 0.0) and not e.eddy_viscosity().any()
        assert launches() == before and _same(e.store(n_av=0)[0], kept)
    p1 = lio.Params(37, 19, 8, 10, 0.1, 0.005, 1.0)
    with n.Engine(p1, obst) as e:                            # omega = 1: nothing to rescale
        e.load_cells(cells0)
        e.sgs_model("smagorinsky", 0.1)
        assert e._L.lbm_sgs_apply(e._h, 1.0, None) == n.LBM_E_INVALID
        assert b"omega = 1" in e._L.lbm_last_error(e._h)
        assert e._L.lbm_sgs_store_nut(e._h, n._ptr(nut)) == n.LBM_E_INVALID
        assert _same(e.store(n_av=0)[0], cells0)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:       # a handle that never sets a model launches nothing new
        e.load_cells(cells0)
        e.run_steps(4, accelerate_first=True)
        assert e.sgs_apply(1.0) is None
        assert not [k for k in e.profile_summary() if "sgs" in k["name"]]


# ------------------------------------------------- run_les is its definition ----

def test_run_les_equals_the_cpu_loop_bitwise(gpu_lib):
    """50 steps at stride 1 on the default kernel in a periodic box with a body force and a porous block, a
    wall-damped Cs, against "lio.forcing_kick, oracle.step, lio.sgs_filter"; stride 3 against its own loop."""
    nx, ny = 48, 24
    p, obst, cells0 = _problem(nx, ny, 21, iters=50)
    zones = [fc.zone(0, (0, 0), (nx, ny), 0.0, None, (1e-5, 0.0)), fc.zone(2, (20, 6), (9, 11), 0.05)]
    cs = _coef((ny, nx), "smagorinsky", "array", 6)
    refs = {}
    for stride in (1, 3):
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            fc.set_zones(e, zones)
            e.sgs_model("smagorinsky", cs)
            av = e.run_les(50, stride, forced=True)
            cells = e.store(n_av=0)[0]
            assert e.kernel_in_use() in ("resident", "step2") and av.size == 50
            with pytest.raises(ValueError):
                e.run_les(5, stride=0)
        want, _ = sc.cpu_les(p, obst, cells0, "smagorinsky", cs, 50, stride, zones)
        cc.assert_same_bits(cells, want, f"run_les(50, {stride})")
        refs[stride] = want
    assert not _same(refs[1], refs[3])
    free, _ = fc.cpu_forced(p, obst, cells0, zones, 50)
    assert not _same(refs[1], free)                          # the model is felt
    with gpu_lib.Engine(p, obst) as e, gpu_lib.Engine(p, obst) as b:
        for h in (e, b):
            h.load_cells(cells0)
            h.sgs_model("smagorinsky", cs)
        hist = e.les_history(13, 5, stride=3)
        assert [s[0] for s in hist] == [5, 10, 13]
        want = []
        for chunk in (5, 5, 3):                              # chunks of 5 in strides of 3: 3 + 2, 3 + 2, 3
            done, st = 0, None
            while done < chunk:
                m = min(3, chunk - done)
                b.run_steps(m)
                st = b.sgs_apply(m, stats=True)
                done += m
            want.append((st[0], st[1] / st[0], st[2]))
        assert [s[1:] for s in hist] == want and all(w[0] > 0 and w[1] > 0 for w in want)
        assert _same(e.store(n_av=0)[0], b.store(n_av=0)[0])


# ------------------------------------------------- physics on the device ----

def test_equivalence_on_the_device(gpu_lib):
    def run(p, obst, cells0, steps):
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            e.sgs_model("omega", sc.WAVE_OMEGA1)
            e.run_les(steps)
            return e.store(n_av=0)[0]
    gap = sc.wave_gap(2, run=run)
    print(f"equivalence on the device: max |filtered omega0 run - plain omega1 run| {gap:.3e}")
    assert gap <= WAVE_BOUND[2]


def test_smagorinsky_slot_on_the_device(gpu_lib):
    p, obst, cells0, zones = sc.slot(2)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        fc.set_zones(e, zones)
        e.sgs_model("smagorinsky", sc.SLOT_CS)
        e.run_les(sc.SLOT_STEPS - 50, forced=True)
        hist = e.les_history(50, 50, forced=True)
        cells = e.store(n_av=0)[0]
        nut = e.eddy_viscosity()
    err, across = sc.slot_profile_error(p, obst, cells, 2)
    print(f"Smagorinsky slot on the device: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= SLOT_BOUND and across <= CROSS_BOUND
    # The eddy viscosity is Cs^2 |u'|, largest beside the walls (xi = 7.5).  On the CPU restatement the last
    # application's largest nu_add is 8.11219e-3 against the exact 8.11123e-3, 1.2e-4 apart; asserted 5e-4.
    step, cells_n, mean, peak = hist[0]
    assert step == 50 and cells_n == int((obst == 0).sum()) and 0 < mean < peak
    want = (-sc.SLOT_NU0 + math.sqrt(sc.SLOT_NU0 ** 2 + 4 * sc.SLOT_CS ** 2 * sc.SLOT_F * 7.5)) / 2
    print(f"largest eddy viscosity {peak:.6e}, Cs^2 |u'| at xi = 7.5 {want:.6e}; nu0 {sc.SLOT_NU0:.4e}")
    assert abs(peak - want) <= 5e-4 * want
    # eddy_viscosity() of a filtered lattice reads the rescaled non-equilibrium part: low by (1 - w_eff) / (1 - w0)
    assert not nut[:, 0].any() and 0.85 * want < float(nut[1, 1]) < 0.95 * want


# ----------------------------------------------------------------- runner ----

def test_runner_sgs_option(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    help_text = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--sgs" in help_text.stdout + help_text.stderr and "--sgs-stride" in help_text.stdout + help_text.stderr
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "23"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file)]
    for spec, stride in (("smagorinsky:0.17", 1), ("omega:1.2", 4)):
        d = tmp_path / f"s{stride}"
        d.mkdir()
        r = subprocess.run(base + ["--sgs", spec, "--sgs-stride", str(stride), "--out-dir", str(d)],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
        final = (d / "final_state.dat").read_text()
        kind, coef = spec.split(":")
        with gpu_lib.Engine(p, obst) as e:                   # the same run through the binding
            e.load_cells(lio.init_cells(p))
            e.sgs_model(kind, float(coef))
            hist = e.les_history(23, stride, stride, accelerate_first=True)
            cells = e.store(n_av=0)[0]
            e.load_cells(lio.init_cells(p))                  # and the free run, which must differ
            e.run_steps(23, accelerate_first=True)
            assert not _same(cells, e.store(n_av=0)[0])
        want = tmp_path / f"want{stride}.dat"
        assert lio.write_results(str(want), p, obst, cells)
        assert final == want.read_text()
        got = (d / "sgs.dat").read_text().split("\n")
        assert [l for l in got if l] == [f"{s} {c} {m:.17g} {x:.17g}" for s, c, m, x in hist]
    r = subprocess.run(base + ["--sgs", "smagorinsky:0.1", "--device", "cpu", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--sgs" in r.stderr
    for bad in ("wale:0.1", "smagorinsky", "omega:abc", "smagorinsky:0.1x"):
        r = subprocess.run(base + ["--sgs", bad, "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--sgs" in r.stderr, bad
    r = subprocess.run(base + ["--sgs", "omega:2.5", "--out-dir", str(tmp_path)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "(0, 2)" in r.stderr
