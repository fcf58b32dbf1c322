"""Host side of the sub-grid model (include/lbm_sgs_hip.h; CPU only).

* The header declares exactly native.EXPORTED_SGS: 8 symbols, all exported by the library and disjoint from
  every other header's list; the other headers' counts and the ABI version stay.
* lbm_sgs_filter_ref / lbm3d_sgs_filter_ref -- the kernels' per-cell function compiled for the host -- equal
  lio.sgs_filter[3d] bit for bit, cells and nut, on random states with about 10 % obstacles, both modes,
  constant and array coefficients, n in (1, 3, 0.37); idle cells keep a planted -0.0f; a NaN planted in one
  fluid cell leaves every other cell's bits alone; bad arguments write nothing.
* Equivalence pins the mechanism.  A 32 x 8 (x 4) periodic shear wave (amplitude 0.02, cross flow 0.01, two
  obstacle cells): 200 times "oracle step at omega0 = 1.7, then the filter OMEGA 1.2, n = 1" against 200
  oracle steps at omega = 1.2.  Measured on this restatement, max |difference| over all populations (the
  largest is 0.44, one ulp 3e-8): 2.4e-7 (2-D), 4.5e-7 (3-D); asserted 1e-6 and 2e-6, 4.2 and 4.5 times the
  measurement.  Planted errors, 2-D / 3-D: q rescaled on the diagonal speeds only 8.0e-4 / 2.4e-4 (800 and
  120 times the bound); d without the 1 / (1 - omega0) is unstable -- 1.1e-2 / 5.7e-3 after 20 steps (more
  than 2800 times the bound) and not finite after 200.
* Smagorinsky profile.  A slot of 18 x 4 (x 4), obstacle columns at x = 0 and 17, density 0.8, omega0 = 1.8,
  a whole-domain forcing zone with f = 2e-5 along the last axis that is not x, Cs = 1.2; 12000 times "kick,
  oracle step, filter n = 1".  The exact steady profile follows from (nu0 + Cs^2 |u'|) |u'| = f |xi|
  (sgs_cases.slot_exact).  Measured on this restatement, error as a share of the peak speed 0.026:
  4.25e-3 (2-D), 4.19e-3 (3-D); asserted 1e-2, 2.4 times the measurement.  Cross flow max |u_x| 6.1e-7 /
  5.0e-7, asserted 2e-6.  The laminar profile lies 0.32 away (32 times the bound: a dead filter fails), and
  18 planted for 18 sqrt 2 gives 5.8e-2 (5.8 times the bound).
* Budget.  One application on a 5 % perturbed lattice changes the mass of a cell by at most 1.4e-7 (2-D) /
  1.7e-7 (3-D) and a momentum component by 2.8e-8 / 2.6e-8 (measured; the populations change by up to 4e-2):
  the rounding of q alone.  Asserted 5e-7 and 1e-7, 3 to 4 times the measurement.  The fp64 sum of nu_add
  obeys the fold bound of forcing_cases.fold_bound.
"""
from __future__ import annotations

import math
import re
import subprocess

import numpy as np
import pytest

import forcing_cases as fc
import sgs_cases as sc
from conftest import ROOT
from lbm_amd import io as lio
from lbm_amd import native

WAVE_BOUND = {2: 1e-6, 3: 2e-6}
SLOT_BOUND, CROSS_BOUND = 1e-2, 2e-6
MASS_BOUND, MOMENTUM_BOUND = 5e-7, 1e-7
MODES = ("smagorinsky", "omega")


# --------------------------------------------------------------- exports ----

def test_library_exports_every_sgs_symbol():
    text = (ROOT / "include" / "lbm_sgs_hip.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", code)))
    assert len(syms) == 8 and sorted(native.EXPORTED_SGS) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    others = {k: v for k, v in vars(native).items() if k.startswith("EXPORTED") and k != "EXPORTED_SGS"}
    assert len(others) >= 14
    for name, other in others.items():
        assert not set(syms) & set(other), name
    assert (len(native.EXPORTED_SCALAR), len(native.EXPORTED_THERMAL), len(native.EXPORTED_TRANSPORT),
            len(native.EXPORTED_WALLS), len(native.EXPORTED_FORCING)) == (16, 4, 4, 10, 10)
    assert L.lbm_abi_version() == native.ABI_VERSION == 5
    for name, value in (("OFF", 0), ("SMAGORINSKY", 1), ("OMEGA", 2)):
        assert getattr(native, "SGS_" + name) == value and f"#define LBM_SGS_{name} {value}" in text


# ----------------------------------------------------------- restatement ----

def _state(dims):
    shape = (19, 37) if dims == 2 else (5, 7, 13)
    return shape, fc.random_state(shape, 0.8, 11 * dims)


def _ref(dims):
    return native.sgs_filter_ref if dims == 2 else native.sgs_filter3d_ref


@pytest.mark.parametrize("fields", [False, True], ids=["constant", "array"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [2, 3])
def test_host_restatement_equals_numpy_bitwise(dims, mode, fields):
    shape, (obst, cells) = _state(dims)
    assert obst.any()
    coef = sc.random_coef(shape, mode, 5 + dims, fields)
    for n in (1.0, 3.0, 0.37):
        want, wnut, idle = sc.filt(dims)(cells, obst, 1.7, mode, coef, n, with_idle=True)
        got, gnut = _ref(dims)(cells, obst, 1.7, mode, coef, n)
        bad = fc.b32(want) != fc.b32(got)
        assert not bad.any(), (n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        assert fc.same(wnut, gnut), n
        assert idle[obst != 0].all() and fc.same(got[idle], cells[idle]) and not gnut[idle].any()
        live = ~idle
        assert live.any() and (fc.b32(got[live]) != fc.b32(cells[live])).any(axis=-1).all()
        if fields:
            off = (coef == 0) if mode == "smagorinsky" else (coef == np.float32(1.7))
            assert off[obst == 0].any() and idle[off].all()
    # n = 0: nothing moves
    got, gnut = _ref(dims)(cells, obst, 1.7, mode, coef, 0.0)
    want, wnut = sc.filt(dims)(cells, obst, 1.7, mode, coef, 0.0)
    assert fc.same(got, cells) and fc.same(want, cells) and not gnut.any() and not wnut.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [2, 3])
def test_idle_cells_keep_every_bit(dims, mode):
    """Obstacles and cells with Cs = 0 / the rate omega0 itself: a planted -0.0f survives (x + 0 would flip it)."""
    shape, (obst, cells) = _state(dims)
    cells = cells.copy()
    cells[..., 2] = np.float32(-0.0)
    off = np.float32(0.0 if mode == "smagorinsky" else 1.7)
    coef = np.full(shape, 0.2 if mode == "smagorinsky" else 1.1, np.float32)
    coef[..., 1::2] = off                                        # every other column is idle
    for f in (sc.filt(dims), _ref(dims)):
        out, nut = f(cells, obst, 1.7, mode, coef, 1.0)
        idle = (obst != 0) | (coef == off)
        assert fc.same(out[idle], cells[idle]) and not nut[idle].any()
        assert (fc.b32(out[idle][:, 2]) == 0x80000000).all()
        assert (fc.b32(out[~idle][:, 2]) != 0x80000000).all() and nut[~idle].all()
        out, nut = f(cells, obst, 1.7, mode, float(off), 2.0)    # the constant that switches the model off
        assert fc.same(out, cells) and not nut.any()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [2, 3])
def test_a_nan_stays_in_its_cell(dims, mode):
    shape, (obst, cells) = _state(dims)
    at = tuple(np.argwhere(obst == 0)[7])
    bad = cells.copy()
    bad[at + (3,)] = np.nan
    coef = sc.random_coef(shape, mode, 9, True)
    for f in (sc.filt(dims), _ref(dims)):
        clean, cnut = f(cells, obst, 1.7, mode, coef, 1.0)
        out, nut = f(bad, obst, 1.7, mode, coef, 1.0)
        other = np.ones(shape, bool)
        other[at] = False
        assert fc.same(out[other], clean[other]) and fc.same(nut[other], cnut[other])
        if coef[at] != (0 if mode == "smagorinsky" else np.float32(1.7)):
            assert np.isnan(out[at]).all()


def test_host_restatement_refuses_bad_arguments():
    L = native.load_library()
    P = native._ptr
    obst, cells = fc.random_state((4, 6), 0.8, 1)
    obst3, cells3 = fc.random_state((2, 4, 6), 0.8, 2)
    keep, keep3 = cells.copy(), cells3.copy()
    nan, inf = float("nan"), float("inf")
    nut, nut3 = np.full((4, 6), 7, np.float32), np.full((2, 4, 6), 7, np.float32)

    def two(nx=6, ny=4, o=P(obst), c=P(cells), w=1.7, mode=1, k=0.2, coef=None, n=1.0):
        return L.lbm_sgs_filter_ref(nx, ny, o, c, w, mode, k, coef, n, P(nut))

    def three(nx=6, ny=4, nz=2, o=P(obst3), c=P(cells3), w=1.7, mode=1, k=0.2, coef=None, n=1.0):
        return L.lbm3d_sgs_filter_ref(nx, ny, nz, o, c, w, mode, k, coef, n, P(nut3))

    arr = np.full((4, 6), 0.2, np.float32)
    arr[2, 3] = np.nan
    high = np.full((4, 6), 1.2, np.float32)
    high[1, 1] = 1.99
    for kw in (dict(nx=0), dict(ny=-1), dict(o=None), dict(c=None), dict(w=1.0), dict(w=0.0), dict(w=2.0), dict(w=nan),
               dict(mode=0), dict(mode=3), dict(mode=-1), dict(k=-0.1), dict(k=nan), dict(k=inf), dict(coef=P(arr)),
               dict(mode=2, k=0.0), dict(mode=2, k=2.0), dict(mode=2, k=-1.0), dict(mode=2, k=nan),
               dict(mode=2, k=1.99, n=3.0),                    # three steps towards 1.99 overshoot 2
               dict(mode=2, coef=P(high), n=3.0), dict(n=nan), dict(n=inf), dict(n=-1.0)):
        assert two(**kw) == native.LBM_E_INVALID, kw
    for kw in (dict(nz=0), dict(o=None), dict(c=None), dict(w=1.0), dict(mode=5), dict(k=-1.0), dict(mode=2, k=2.5),
               dict(mode=2, k=1.99, n=3.0), dict(n=nan), dict(n=-0.5)):
        assert three(**kw) == native.LBM_E_INVALID, kw
    assert fc.same(cells, keep) and fc.same(cells3, keep3) and (nut == 7).all() and (nut3 == 7).all()
    assert two(n=0.0) == native.LBM_OK and three(n=0.0) == native.LBM_OK
    assert fc.same(cells, keep) and fc.same(cells3, keep3) and not nut.any() and not nut3.any()
    assert two() == native.LBM_OK and three() == native.LBM_OK
    assert two(mode=2, k=1.99, n=1.0) == native.LBM_OK           # one step towards 1.99 is in range
    assert not fc.same(cells, keep) and not fc.same(cells3, keep3) and nut.any() and nut3.any()
    with pytest.raises(ValueError):
        native.sgs_filter_ref(keep, obst, 1.7, "wale", 0.1)
    with pytest.raises(ValueError):
        native.sgs_filter_ref(keep, obst, 1.7, "smagorinsky", np.zeros((3, 3), np.float32))
    for bad in (dict(omega=1.0), dict(mode="wale"), dict(coef=-0.1), dict(coef=nan), dict(n=-1.0),
                dict(mode="omega", coef=2.0), dict(mode="omega", coef=1.99, n=3.0)):
        kw = dict(omega=1.7, mode="smagorinsky", coef=0.1, n=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            lio.sgs_filter(keep, obst, kw["omega"], kw["mode"], kw["coef"], kw["n"])


# ----------------------------------------------------- physics: equivalence ----

@pytest.mark.parametrize("dims", [2, 3])
def test_filter_after_every_step_is_a_collision_at_the_other_rate(dims):
    gap = sc.wave_gap(dims)
    print(f"equivalence {dims}-D: max |filtered omega0 run - plain omega1 run| {gap:.3e}")
    assert gap <= WAVE_BOUND[dims]
    # the two rates differ: without the filter the runs are far apart
    p, obst, cells0 = sc.shear_wave(dims)
    plain = sc.step(p, obst, cells0, sc.WAVE_STEPS)
    other = sc.step(sc.shear_wave(dims, sc.WAVE_OMEGA1)[0], obst, cells0, sc.WAVE_STEPS)
    assert np.abs(plain.astype(np.float64) - other).max() > 100 * WAVE_BOUND[dims]


@pytest.mark.parametrize("planted", ["no 1 / (1 - omega0)", "diagonals only"])
@pytest.mark.parametrize("dims", [2, 3])
def test_equivalence_shows_planted_errors(dims, planted, monkeypatch):
    if planted == "diagonals only":
        monkeypatch.setattr(lio, "SGS_RESCALED", (5, 6, 7, 8))
        monkeypatch.setattr(lio, "SGS_RESCALED3D", (5, 6, 7, 8, 10, 11, 12, 13, 15, 16, 17, 18))
        gap = sc.wave_gap(dims)
    else:
        monkeypatch.setattr(lio, "sgs_factor", lambda w0, we, omo: w0 - we)
        gap = sc.wave_gap(dims, steps=20)                        # unstable: not finite after 200 steps
    print(f"equivalence {dims}-D with a planted error ({planted}): {gap:.3e}")
    assert gap > 100 * WAVE_BOUND[dims]


# ------------------------------------------------------- physics: the slot ----

@pytest.mark.parametrize("dims", [2, 3])
def test_smagorinsky_slot_reaches_the_exact_profile(dims):
    err, across = sc.slot_error(dims)
    print(f"Smagorinsky slot {dims}-D: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= SLOT_BOUND and across <= CROSS_BOUND
    assert sc.laminar_distance() > 30 * SLOT_BOUND               # a dead filter is far off
    assert abs(sc.slot_exact().max() - 0.026) < 1e-3


def test_slot_shows_a_planted_constant(monkeypatch):
    monkeypatch.setattr(lio, "SGS_SMAG_K", np.float32(18))       # 18 for 18 sqrt 2
    err = sc.slot_error(2)[0]
    print(f"Smagorinsky slot with 18 planted for 18 sqrt 2: {err:.3e}")
    assert err > 5 * SLOT_BOUND


# ------------------------------------------------------- physics: budget ----

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", [2, 3])
def test_an_application_moves_no_mass_and_no_momentum(dims, mode):
    shape = (19, 37) if dims == 2 else (5, 7, 13)
    obst, cells = fc.random_state(shape, 0.8, 5)
    coef = sc.random_coef(shape, mode, 3, True)
    out, nut, idle = sc.filt(dims)(cells, obst, 1.7, mode, coef, 1.0, with_idle=True)
    e = np.array(lio.E2 if dims == 2 else lio.E3, np.float64)
    change = out.astype(np.float64) - cells.astype(np.float64)
    mass = float(np.abs(change.sum(-1)).max())
    mom = max(float(np.abs((change * e[:, c]).sum(-1)).max()) for c in range(dims))
    print(f"budget {dims}-D {mode}: max mass change of a cell {mass:.3e}, momentum {mom:.3e}, "
          f"largest change of a population {np.abs(change).max():.3e}")
    assert mass <= MASS_BOUND and mom <= MOMENTUM_BOUND
    assert np.abs(change).max() > 1e3 * MASS_BOUND               # the populations do move
    cells_n, total, peak = lio.sgs_stats(nut, idle)
    live = nut[~idle].astype(np.float64)
    assert 0 < cells_n == live.size < int((obst == 0).sum())     # idle fluid cells exist
    exact = math.fsum(live.tolist())
    assert abs(total - exact) <= fc.fold_bound(live) and abs(float(np.sum(live[::-1])) - exact) <= fc.fold_bound(live)
    assert peak == max(float(nut.max()), 0.0)
