"""Host side of the forcing zones (include/lbm_forcing_hip.h; CPU only).

* The header declares exactly native.EXPORTED_FORCING: 10 symbols, all exported by the library and disjoint
  from every other header's list; the other headers' counts and the ABI version stay.
* lbm_forcing_kick_ref / lbm3d_forcing_kick_ref -- the kernels' per-cell function compiled for the host --
  equal lio.forcing_kick[3d] bit for bit, cells and terms, on random states with about 10 % obstacles and on
  every box the GPU tests use; bad arguments write nothing; a planted -0.0f survives in an idle cell.
* Physics pins the restatement.  The CPU loop "kick, oracle step" in the slot of thermal_cases.slot()
  (34 x 4 (x 4), obstacle columns at x = 0 and 33, omega = 1, density 0.8, 6000 steps, f = 1e-5).  Measured
  on this restatement, error as a share of the peak speed (2-D / 3-D), and the bound asserted:
      Poiseuille (lam = 0)              5.87e-4 / 3.39e-4      2e-3
      Darcy-Brinkman, lam = 0.002       7.39e-4 / 7.33e-4      2e-3
      Darcy-Brinkman, lam = 0.01        2.16e-3 / 2.14e-3      5e-3   (the first-order splitting error grows with lam)
      cross flow, max |u_x|             1.9e-7 / 2.0e-7        1e-6
  each bound two to six times the measurement, rounded up.  The planted errors, on the Poiseuille slot
  (the last on lam = 0.01 too): rho dropped from the force term 0.248; 1/9 for 1/12 on the diagonals 0.996;
  the sign of q 0.33; l applied to rho ut only 0.999 (0.990): each more than 60 times its bound.
* Target: one kick with lam = 1 and random |ut| <= 0.05 on a 5 % perturbed lattice leaves lio.macroscopic
  = ut on the fluid cells within 4.9e-8 (2-D) and 5.4e-8 (3-D) measured, 2e-7 asserted; the mass of a cell
  moves by at most 1.5e-8 measured, 1e-7 asserted.
* Impulse budget: the fp64 change of the lattice's momentum equals the summed terms to the rounding of the
  increments -- measured gap 7.5e-8 (2-D), 6.7e-8 (3-D); asserted: (q - 1) half-ulps of the largest population
  per kicked cell, the worst case of that rounding -- and the fp64 sum of the terms obeys the fold bound.
"""
from __future__ import annotations

import ctypes
import math
import re
import subprocess

import numpy as np
import pytest

import forcing_cases as fc
from conftest import ROOT
from lbm_amd import io as lio
from lbm_amd import native

POISEUILLE_BOUND, BRINKMAN_BOUND, CROSS_BOUND = 2e-3, {0.002: 2e-3, 0.01: 5e-3}, 1e-6
TARGET_BOUND, MASS_BOUND = 2e-7, 1e-7


# --------------------------------------------------------------- exports ----

def test_library_exports_every_forcing_symbol():
    text = (ROOT / "include" / "lbm_forcing_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 10 and sorted(native.EXPORTED_FORCING) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    others = {k: v for k, v in vars(native).items() if k.startswith("EXPORTED") and k != "EXPORTED_FORCING"}
    assert len(others) >= 13
    for name, other in others.items():
        assert not set(syms) & set(other), name
    assert (len(native.EXPORTED_SCALAR), len(native.EXPORTED_THERMAL), len(native.EXPORTED_TRANSPORT),
            len(native.EXPORTED_WALLS)) == (16, 4, 4, 10)
    assert L.lbm_abi_version() == native.ABI_VERSION == 5
    assert native.FORCING_MAX_ZONES == 8 and "#define LBM_FORCING_MAX_ZONES 8" in text


# ----------------------------------------------------------- restatement ----

def _state(dims):
    shape = (19, 37) if dims == 2 else (5, 7, 13)
    return shape, fc.random_state(shape, 0.8, 11 * dims)


def _boxes(shape):
    return fc.boxes2d(shape[1], shape[0]) if len(shape) == 2 else fc.boxes3d(shape[2], shape[1], shape[0])


@pytest.mark.parametrize("fields", [False, True], ids=["uniform", "fields"])
@pytest.mark.parametrize("dims", [2, 3])
def test_host_restatement_equals_numpy_bitwise(dims, fields):
    shape, (obst, cells) = _state(dims)
    ref = native.forcing_kick_ref if dims == 2 else native.forcing_kick3d_ref
    kick = lio.forcing_kick if dims == 2 else lio.forcing_kick3d
    boxes = _boxes(shape)
    assert len(boxes) >= (6 if dims == 2 else 12) and obst.any()
    for i, box in enumerate(boxes):
        z = fc.box_zone(0, box, 100 * dims + i, fields, idle=0.3)
        for n in (1.0, 3.0, 0.37):
            want, wterms = kick(cells, obst, box, fc.coef_of(z), n)
            got, gterms = ref(cells, obst, box, z["lam"], z["target"], z["force"], n)
            bad = fc.b32(want) != fc.b32(got)
            assert not bad.any(), (box, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert fc.same(wterms, gterms), (box, n)
            sl = tuple(slice(o, o + e) for o, e in zip(box[:dims][::-1], box[dims:][::-1]))
            outside = np.ones(cells.shape[:-1], bool)
            outside[sl] = False
            assert fc.same(got[outside], cells[outside]) and fc.same(got[..., 0], cells[..., 0])
            assert fc.same(got[obst != 0], cells[obst != 0])
            if (obst[sl] == 0).any() and not fields:
                assert not fc.same(got[sl], cells[sl])


@pytest.mark.parametrize("dims", [2, 3])
def test_idle_cells_keep_every_bit(dims):
    """Obstacles, cells with lam = 0 and f = 0, and steps = 0: a planted -0.0f survives (x + 0 would flip it)."""
    shape, (obst, cells) = _state(dims)
    obst = obst.copy()
    obst[...] = 0
    cells = cells.copy()
    cells[..., 2] = np.float32(-0.0)
    ext = shape[::-1]
    box = (0,) * dims + ext
    lam = np.zeros(shape, np.float32)
    lam[..., ::2] = 0.25                                         # every other column is idle
    for f in (lambda *a: (lio.forcing_kick if dims == 2 else lio.forcing_kick3d)(a[0], a[1], a[2], [a[3]] + a[4] + a[5], a[6]),
              native.forcing_kick_ref if dims == 2 else native.forcing_kick3d_ref):
        out, terms = f(cells, obst, box, lam, [0.01] * dims, [0.0] * dims, 1.0)
        assert fc.same(out[..., 1::2, :], cells[..., 1::2, :]) and not terms[..., 1::2, :].any()
        assert (fc.b32(out[..., 1::2, 2]) == 0x80000000).all()
        assert (fc.b32(out[..., ::2, 2]) != 0x80000000).all() and terms[..., ::2, :].any()
        out, terms = f(cells, obst, box, lam, [0.01] * dims, [0.0] * dims, 0.0)
        assert fc.same(out, cells) and not terms.any()
        out, terms = f(cells, obst, box, 0.0, [0.3] * dims, [-0.0] * dims, 2.0)     # a target without a drag is idle
        assert fc.same(out, cells) and not terms.any()


def test_host_restatement_refuses_bad_arguments():
    L = native.load_library()
    P = native._ptr
    obst, cells = fc.random_state((4, 6), 0.8, 1)
    obst3, cells3 = fc.random_state((2, 4, 6), 0.8, 2)
    keep, keep3 = cells.copy(), cells3.copy()
    nan, inf = float("nan"), float("inf")
    ctypes_f32p = ctypes.POINTER(ctypes.c_float)

    def konst(n, **kw):
        v = [0.1, 0.01, 0.02, 0.03, 1e-4, 2e-4, 3e-4][:n] if n == 7 else [0.1, 0.01, 0.02, 1e-4, 2e-4]
        for i, x in kw.items():
            v[int(i[1:])] = x
        return (ctypes.c_float * n)(*v)

    def two(nx=6, ny=4, o=P(obst), c=P(cells), box=(1, 1, 3, 2), coef=None, k=None, n=1.0):
        return L.lbm_forcing_kick_ref(nx, ny, o, c, *box, coef, konst(5) if k is None else k, n, None)

    def three(nx=6, ny=4, nz=2, o=P(obst3), c=P(cells3), box=(1, 1, 0, 3, 2, 2), coef=None, k=None, n=1.0):
        return L.lbm3d_forcing_kick_ref(nx, ny, nz, o, c, *box, coef, konst(7) if k is None else k, n, None)

    arr = np.full((2, 3), np.nan, np.float32)
    table = (ctypes_f32p * 5)(None, P(arr), None, None, None)
    for kw in (dict(nx=0), dict(ny=-1), dict(o=None), dict(c=None), dict(box=(4, 1, 3, 2)), dict(box=(1, 3, 3, 2)),
               dict(box=(-1, 1, 3, 2)), dict(box=(1, 1, -3, 2)), dict(box=(1, 1, 0, 2)), dict(n=nan), dict(n=inf),
               dict(n=-1.0), dict(k=konst(5, k0=-0.1)), dict(k=konst(5, k0=nan)), dict(k=konst(5, k2=inf)),
               dict(k=konst(5, k4=nan)), dict(coef=table)):
        assert two(**kw) == native.LBM_E_INVALID, kw
    for kw in (dict(nz=0), dict(o=None), dict(c=None), dict(box=(1, 1, 1, 3, 2, 2)), dict(box=(1, 1, 0, 3, 2, -1)),
               dict(n=nan), dict(n=-0.5), dict(k=konst(7, k0=-1.0)), dict(k=konst(7, k6=nan)), dict(k=konst(7, k3=inf))):
        assert three(**kw) == native.LBM_E_INVALID, kw
    assert fc.same(cells, keep) and fc.same(cells3, keep3)
    assert two(n=0.0) == native.LBM_OK and three(n=0.0) == native.LBM_OK
    assert fc.same(cells, keep) and fc.same(cells3, keep3)
    assert two() == native.LBM_OK and three() == native.LBM_OK
    assert not fc.same(cells, keep) and not fc.same(cells3, keep3)
    with pytest.raises(ValueError):
        native.forcing_kick_ref(keep, obst, (0, 0, 6, 4), target=(0.1, 0.1, 0.1))
    with pytest.raises(ValueError):
        native.forcing_kick_ref(keep, obst, (0, 0, 6, 4), lam=np.zeros((3, 3), np.float32))
    for bad in (dict(box=(0, 0, 7, 4)), dict(n=-1.0), dict(coef=[-0.1, 0, 0, 0, 0]), dict(coef=[0.1, nan, 0, 0, 0])):
        kw = dict(box=(0, 0, 6, 4), coef=[0.1, 0, 0, 0, 0], n=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            lio.forcing_kick(keep, obst, kw["box"], kw["coef"], kw["n"])


# -------------------------------------------------------- physics: slot ----

PLANTED = {
    "no rho in the force": lambda l, rho, ut, j, g: (l * ((rho * ut) - j)) + g,
    "l on rho ut only": lambda l, rho, ut, j, g: ((l * (rho * ut)) - j) + (rho * g),
}


@pytest.mark.parametrize("dims", [2, 3])
def test_poiseuille_slot_reaches_the_exact_profile(dims):
    err, across = fc.slot_error(dims, 0.0)
    print(f"Poiseuille {dims}-D: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= POISEUILLE_BOUND and across <= CROSS_BOUND


@pytest.mark.parametrize("lam", [0.002, 0.01])
@pytest.mark.parametrize("dims", [2, 3])
def test_darcy_brinkman_slot_reaches_the_exact_profile(dims, lam):
    err, across = fc.slot_error(dims, lam)
    print(f"Darcy-Brinkman {dims}-D, lam = {lam}: error {err:.3e} of the peak speed, max |u_x| {across:.3e}")
    assert err <= BRINKMAN_BOUND[lam] and across <= CROSS_BOUND
    # the drag is felt: the Poiseuille profile is far off
    assert abs(fc.slot_exact(lam).max() - fc.slot_exact(0.0).max()) > 100 * BRINKMAN_BOUND[lam] * fc.slot_exact(lam).max()


@pytest.mark.parametrize("planted", ["no rho in the force", "l on rho ut only", "diagonal weight", "sign of q"])
def test_slot_shows_planted_errors(planted, monkeypatch):
    if planted in PLANTED:
        monkeypatch.setattr(lio, "forcing_momentum", PLANTED[planted])
    elif planted == "diagonal weight":
        monkeypatch.setattr(lio, "KICK_W", (lio.KICK_W[0], np.float32(3) * (np.float32(1) / np.float32(9))))
    else:
        monkeypatch.setattr(lio, "KICK_PAIRS", lio.KICK_PAIRS[:3] + ((6, 8, ((+1, 0), (-1, 1))),))    # q = bx - by
    # the replacement runs through kick=, as thermal_cases.slot_error takes one
    kick = lambda *a: lio.forcing_kick(*a)                                                  # noqa: E731
    err = fc.slot_error(2, 0.0, kick=kick)[0]
    print(f"Poiseuille with a planted error ({planted}): {err:.4f}")
    assert err > 60 * POISEUILLE_BOUND
    if planted == "l on rho ut only":
        err = fc.slot_error(2, 0.01, kick=kick)[0]
        print(f"Darcy-Brinkman (0.01) with a planted error ({planted}): {err:.4f}")
        assert err > 60 * BRINKMAN_BOUND[0.01]


# ------------------------------------------- physics: target, impulse ----

def _target_state(dims):
    shape = (19, 37) if dims == 2 else (5, 7, 13)
    obst, cells = fc.random_state(shape, 0.8, 5)
    rng = np.random.default_rng(2)
    ut = [(0.05 * (2 * rng.random(shape) - 1)).astype(np.float32) for _ in range(dims)]
    p = (lio.Params(shape[1], shape[0], 0, 10, 0.8, 0.0, 1.0) if dims == 2
         else lio.Params3D(shape[2], shape[1], shape[0], 0, 0.8, 0.0, 1.0))
    return shape, p, obst, cells, ut


@pytest.mark.parametrize("dims", [2, 3])
def test_lam_one_sets_the_target_velocity(dims, monkeypatch):
    shape, p, obst, cells, ut = _target_state(dims)
    kick = lio.forcing_kick if dims == 2 else lio.forcing_kick3d
    mac = lio.macroscopic if dims == 2 else lio.macroscopic3d
    box = (0,) * dims + shape[::-1]
    fluid = obst == 0

    def gap(n=1.0, lam=1.0):
        out, _ = kick(cells, obst, box, [lam] + ut + [0.0] * dims, n)
        u = mac(p, obst, out)
        mass = np.abs(out.astype(np.float64).sum(-1) - cells.astype(np.float64).sum(-1)).max()
        return max(float(np.abs(u[c].astype(np.float64) - ut[c])[fluid].max()) for c in range(dims)), float(mass)

    err, mass = gap()
    print(f"target {dims}-D: max |u - ut| {err:.3e}, max mass change of a cell {mass:.3e}")
    assert err <= TARGET_BOUND and mass <= MASS_BOUND
    assert gap(4.0, 0.5)[0] <= TARGET_BOUND                      # l = min(n lam, 1): clamped, not overshot
    assert gap(1.0, 0.5)[0] > 1e4 * TARGET_BOUND                 # half the gap stays
    monkeypatch.setattr(lio, "forcing_momentum", PLANTED["l on rho ut only"])
    assert gap()[0] <= TARGET_BOUND                              # this error is invisible at l = 1 ...
    monkeypatch.setattr(lio, "forcing_momentum", lambda l, rho, ut, j, g: (l * (ut - j)) + (rho * g))
    assert gap()[0] > 1e4 * TARGET_BOUND                         # ... a missing density in the target is not


@pytest.mark.parametrize("dims", [2, 3])
def test_impulse_budget(dims):
    shape, p, obst, cells, _ = _target_state(dims)
    kick = lio.forcing_kick if dims == 2 else lio.forcing_kick3d
    z = fc.box_zone(0, (0,) * dims + shape[::-1], 3, True, idle=0.3)
    out, terms = kick(cells, obst, fc.box_of(z), fc.coef_of(z), 1.0)
    e = np.array(lio.E2 if dims == 2 else lio.E3, np.float64)
    kicked = int((terms != 0).any(axis=-1).sum())
    assert 0 < kicked < int((obst == 0).sum())                   # idle fluid cells exist
    # every increment is added with one rounding of at most half an ulp of the result
    gap_bound = kicked * (cells.shape[-1] - 1) * 2.0 ** -24 * 2 * float(np.abs(out).max())
    for c in range(dims):
        dj = float(((out.astype(np.float64) - cells.astype(np.float64)) * e[:, c]).sum())
        t = terms[..., c].astype(np.float64).ravel()
        total = math.fsum(t.tolist())
        print(f"budget {dims}-D, component {c}: lattice {dj!r}, terms {total!r}, gap {abs(dj - total):.3e} "
              f"(bound {gap_bound:.3e})")
        assert abs(dj - total) <= gap_bound < 1e-3 * float(np.abs(t).sum())     # a wrong term would show
        assert abs(float(np.sum(t)) - total) <= fc.fold_bound(t)
        assert abs(float(np.sum(t[::-1])) - total) <= fc.fold_bound(t)
