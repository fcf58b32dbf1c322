"""Host side of the scalar transport sums (include/lbm_transport_hip.h; CPU only).

* The header declares exactly native.EXPORTED_TRANSPORT, all exported by the library; the scalar and
  thermal headers' lists are unchanged and the ABI version stays.
* lbm_scalar_terms_ref / lbm3d_scalar_terms_ref -- the kernels' per-cell function compiled for the host
  -- equal lio.scalar_terms[3d] bit for bit (uint64 patterns); bad arguments write nothing.
* The budget: phi(scalar_step(g)) - phi(g) is minus the divergence of the face fluxes within
  32 * 2^-24 * S per cell, everything in fp32; a face from the wrong neighbour and a flipped sign miss
  that bound by more than ten times.
* Physics pins the magnitude: pure conduction carries D nx / 19 through every plane (omega_s = 1), and
  the Rayleigh-Benard set-up at Ra = 3000 carries the same amount through every plane between the fixed
  rows once it is steady, 1.83 times what conduction carries.
"""
from __future__ import annotations

import functools
import re
import subprocess

import numpy as np
import pytest

import thermal_cases as tc
import transport_cases as xc
from conftest import ROOT
from lbm_amd import io as lio
from lbm_amd import native


# --------------------------------------------------------------- exports ----

def _declared(header):
    text = (ROOT / "include" / header).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_transport_symbol():
    syms = _declared("lbm_transport_hip.h")
    assert len(syms) == 4 and sorted(native.EXPORTED_TRANSPORT) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    # the scalar and thermal headers did not grow
    scalar, thermal = _declared("lbm_scalar_hip.h"), _declared("lbm_thermal_hip.h")
    assert len(scalar) == 16 and scalar == sorted(native.EXPORTED_SCALAR)
    assert len(thermal) == 4 and thermal == sorted(native.EXPORTED_THERMAL)
    assert not set(syms) & (set(scalar) | set(thermal) | set(native.EXPORTED_BINNED))
    text = (ROOT / "include" / "lbm_transport_hip.h").read_text()
    assert '#include "lbm_scalar_hip.h"' in text and '#include "lbm_binned_hip.h"' in text
    assert L.lbm_abi_version() == native.ABI_VERSION == 5
    assert lio.SBIN_FIELDS == native.SBIN_FIELDS and lio.SBIN_FIELDS3D == native.SBIN_FIELDS3D
    assert len(native.SBIN_FIELDS) == 6 and len(native.SBIN_FIELDS3D) == 8


# ------------------------------------------------------ host restatement ----

def _state(shape, seed):
    """(obst, g, velocities) of thermal_cases.random_state: 10 % obstacles, -0.0f populations on them."""
    dims = len(shape)
    q, qs = (9, 5) if dims == 2 else (19, 7)
    obst, cells, g = tc.random_state(shape, q, qs, 0.1, seed)
    if dims == 2:
        p = lio.Params(shape[1], shape[0], 0, 10, 0.1, 0.0, 1.0)
        u = lio.macroscopic(p, obst, cells)[:2]
    else:
        p = lio.Params3D(shape[2], shape[1], shape[0], 0, 0.1, 0.0, 1.0)
        u = lio.macroscopic3d(p, obst, cells)[:3]
    return obst, g, u


# extents as (nx, ny[, nz]); numpy's shapes are slowest axis first
SHAPES2 = [(1, 1), (1, 7), (5, 1), (4, 4), (19, 37)]
SHAPES3 = [(1, 1, 1), (1, 3, 2), (3, 1, 5), (5, 7, 13)]


@pytest.mark.parametrize("extent", SHAPES2 + SHAPES3)
def test_host_restatement_equals_numpy_bitwise(extent):
    shape = extent[::-1]
    obst, g, u = _state(shape, 7 + sum(extent))
    if len(shape) == 2:
        want, got = lio.scalar_terms(g, *u, obst), native.scalar_terms_ref(g, *u, obst)
        names = lio.SBIN_FIELDS
    else:
        want, got = lio.scalar_terms3d(g, *u, obst), native.scalar_terms3d_ref(g, *u, obst)
        names = lio.SBIN_FIELDS3D
    assert tuple(want) == tuple(got) == names
    for n in names:
        assert want[n].dtype == np.float64 and want[n].shape == shape
        bad = xc.b64(want[n]) != xc.b64(got[n])
        assert not bad.any(), (extent, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    if np.prod(shape) > 100:
        assert obst.any() and all(np.abs(want[n]).max() > 1e-3 for n in names)
        assert all((want[n][obst != 0] == 0).all() for n in names if n[0] != "f")
        assert all((want[n][obst != 0] != 0).any() for n in names if n[0] == "f")


def test_host_restatement_refuses_bad_arguments():
    L = native.load_library()
    P = native._ptr
    obst, g, (ux, uy) = _state((4, 6), 1)
    obst3, g3, (vx, vy, vz) = _state((2, 4, 6), 2)
    t = np.full((6, 4, 6), 7.0)
    t3 = np.full((8, 2, 4, 6), 7.0)
    two = lambda nx=6, ny=4, a=P(ux), b=P(uy), o=P(obst), gg=P(g), out=P(t): \
        L.lbm_scalar_terms_ref(nx, ny, a, b, o, gg, out)                               # noqa: E731
    three = lambda nx=6, ny=4, nz=2, a=P(vx), b=P(vy), c=P(vz), o=P(obst3), gg=P(g3), out=P(t3): \
        L.lbm3d_scalar_terms_ref(nx, ny, nz, a, b, c, o, gg, out)                      # noqa: E731
    for f in (two, three):
        for kw in (dict(nx=0), dict(ny=-1), dict(a=None), dict(b=None), dict(o=None), dict(gg=None), dict(out=None)):
            assert f(**kw) == native.LBM_E_INVALID, kw
    assert three(nz=0) == native.LBM_E_INVALID and three(c=None) == native.LBM_E_INVALID
    assert (t == 7).all() and (t3 == 7).all()
    assert two() == native.LBM_OK and three() == native.LBM_OK
    assert not (t == 7).any() and not (t3 == 7).any()
    with pytest.raises(ValueError):
        native.scalar_terms_ref(g, ux, uy, obst[:-1])
    with pytest.raises(ValueError):
        native.scalar_terms3d_ref(g, vx, vy, vz, obst3)


def test_binned_restatement_and_nusselt_number():
    obst, g, (ux, uy) = _state((9, 14), 5)
    terms = lio.scalar_terms(g, ux, uy, obst)
    one = lio.scalar_binned_sums(g, ux, uy, obst, 1, 1)
    assert all(np.array_equal(one[n], terms[n] + 0.0) for n in lio.SBIN_FIELDS)
    s = lio.scalar_binned_sums(g, ux, uy, obst, 5, 4)
    assert s["fx"].shape == (3, 3) and s["fluid"].sum() == (obst == 0).sum()
    assert abs(s["phi"].sum() - terms["phi"].sum()) < 1e-12 * np.abs(terms["phi"]).sum()
    fx, fy = lio.scalar_face_flux(g)
    assert fx.dtype == np.float32 and fx[3, 13] == g[1][3, 13] - g[3][3, 0] and fy[8, 2] == g[2][8, 2] - g[4][0, 2]
    assert lio.nusselt_number(2.0, 40, 0.25, 1.0, 20.0) == pytest.approx(4.0)


# ------------------------------------------------------------- the budget ----

def _budget(extent, seed, omega_s, plant=None):
    """(largest residual / bound over the cells, largest residual, largest |change of phi|): the change of
    phi over one step against minus the divergence of the face fluxes, all in fp32, per cell against
    32 * 2^-24 * S with S the largest sum_k |g_k| over the cell and its face neighbours."""
    shape = extent[::-1]
    dims = len(shape)
    obst, g, u = _state(shape, seed)
    if dims == 2:
        new, flux = lio.scalar_step(g, *u, obst, omega_s), list(lio.scalar_face_flux(g))
        axes = (1, 0)
    else:
        new, flux = lio.scalar_step3d(g, *u, obst, omega_s), list(lio.scalar_face_flux3d(g))
        axes = (2, 1, 0)
    if plant == "wrong neighbour":          # g4[y] for g4[y+1] (3-D: g4[y] too)
        flux[1] = g[2] - g[4] if dims == 2 else g[3] - g[4]
    elif plant == "sign":
        flux[1] = -flux[1]
    change = lio.scalar_phi(new) - lio.scalar_phi(g)
    div = None
    for f, ax in zip(flux, axes):
        d = np.roll(f, 1, axis=ax) - f       # F[c - 1] - F[c]
        div = d if div is None else div + d
    assert change.dtype == np.float32 and div.dtype == np.float32
    mass = np.abs(g).sum(axis=0, dtype=np.float32)
    s = mass
    for ax in axes:
        s = np.maximum(s, np.maximum(np.roll(mass, 1, axis=ax), np.roll(mass, -1, axis=ax)))
    res = np.abs(change.astype(np.float64) - div.astype(np.float64))
    bound = 32 * 2.0 ** -24 * s.astype(np.float64)
    return float((res / bound).max()), float(res.max()), float(np.abs(change).max())


@pytest.mark.parametrize("extent,seed", [((14, 9), 3), ((7, 6, 5), 3)])
def test_budget_of_the_face_fluxes(extent, seed):
    """thermal_cases.random_state((9, 14), ..., seed 3) and its 3-D twin on (5, 6, 7), omega_s = 1.3.
    Measured: residual 1.2e-7 where phi changes by up to 0.84 (2-D)."""
    ratio, res, change = _budget(extent, seed, 1.3)
    print(f"{extent}: residual {res:.3e} = {ratio:.4f} of the bound; phi changes by up to {change:.3f}")
    assert ratio <= 1.0 and change > 0.3
    for plant in ("wrong neighbour", "sign"):
        r = _budget(extent, seed, 1.3, plant)[0]
        print(f"{extent} planted {plant}: {r:.3e} of the bound")
        assert r > 10.0


# ------------------------------------------------------- pure conduction ----

def _plane_sums(g):
    """sum_x FY per face row y, float64 (math.fsum-free: 40 fp32 values widened first)."""
    return lio.scalar_face_flux(g)[1].astype(np.float64).sum(axis=1)


@functools.lru_cache(maxsize=None)
def _conduction(omega_s):
    """The plane sums of FY over the faces y = 1 .. 19 after 6000 steps of pure conduction between the fixed
    rows of thermal_cases.rayleigh_benard(0), from the linear profile, over D nx / 19 of that omega_s."""
    p, obst, _, phi0, fixed, _ = tc.rayleigh_benard(0)
    y = np.arange(p.ny, dtype=np.float64)[:, None]
    lin = np.broadcast_to(0.5 - (y - 1) / 19, phi0.shape).astype(np.float32)
    lin[1], lin[p.ny - 2] = np.float32(0.5), np.float32(-0.5)
    g = lio.scalar_apply_fixed(lio.scalar_init(lin), *fixed)
    zero = np.zeros_like(lin)
    for _ in range(6000):
        g = lio.scalar_apply_fixed(lio.scalar_step(g, zero, zero, obst, omega_s), *fixed)
    return _plane_sums(g)[1:20] / (lio.scalar_diffusivity(omega_s, 2) * p.nx / 19.0)


def test_pure_conduction_carries_d_over_h():
    """omega_s = 1: every plane sum of FY between the fixed rows is D nx / 19; measured within 6e-6."""
    r = _conduction(1.0)
    print(f"conduction, omega_s = 1: plane sums / (D nx / 19) in [{r.min():.7f}, {r.max():.7f}]")
    assert r.shape == (19,) and np.abs(r - 1).max() <= 5e-5


# ------------------------------------------------ Rayleigh-Benard transfer ----

@functools.lru_cache(maxsize=None)
def _rb(ra):
    """(plane sums of FY over y = 1 .. 19, sum_x u_y phi of the rows 10 and 11), each over D nx / 19, after
    6000 steps of the CPU loop."""
    p, obst, cells, phi0, fixed, s = tc.rayleigh_benard(ra)
    g = lio.scalar_apply_fixed(lio.scalar_init(phi0), *fixed)
    cells, g = tc.cpu_thermal(p, obst, cells, g, tc.RB_OMEGA, s, 0.0, fixed, xc.RB_STEPS)
    ux, uy = lio.macroscopic(p, obst, cells)[:2]
    conv = lio.scalar_terms(g, ux, uy, obst)["uyphi"].sum(axis=1)
    return _plane_sums(g)[1:20] / xc.rb_unit(), conv[10:12] / xc.rb_unit()


def test_rayleigh_benard_heat_transfer():
    """Ra = 3000: the plane sums over y = 1 .. 19 are 1.88761 to 1.88763 of D nx / 19 (spread 1.4e-5 of the
    mean); conduction at omega_s = 1.4 gives 1.0310 in those units, so Nu = 1.83; the convective part at
    mid-height is 1.672."""
    planes, conv = _rb(3000)
    base = _conduction(tc.RB_OMEGA)
    mean = planes.mean()
    spread = (planes.max() - planes.min()) / mean
    nu = mean / base.mean()
    print(f"Ra 3000: planes [{planes.min():.6f}, {planes.max():.6f}] mean {mean:.6f} spread {spread:.2e}; "
          f"conduction {base.mean():.5f} (spread {np.ptp(base):.1e}); Nu {nu:.4f}; convective {conv.tolist()}")
    assert spread <= xc.RB_FLAT
    assert nu > 1.5
    assert abs(mean - xc.RB_NU_CPU) <= 2e-5           # the figure the device test compares with
    assert (0 < conv).all() and (conv < planes[9:11].min()).all()


MEASURED_BELOW = 9.6e-3


def test_rayleigh_benard_below_onset_conducts():
    """Ra = 1400, below the onset: after 6000 steps the plane sums stay at the conduction value.
    Measured: every plane 0.9596 % BELOW conduction (0.483 % at Ra = 700, the same at step 12000), not the
    1e-5 first expected.  The roll is gone (convective part at mid-height -9e-5 of D nx / 19); what remains
    is the first-order coupling: in hydrostatic balance the stored lattice carries an apparent velocity of
    minus half the kick, u_y = -a (phi - phi_ref) / 2 (2.4e-4 here), which the scalar step advects with.
    It is linear in the acceleration and flat over the planes.  Asserted with a margin of five."""
    planes, conv = _rb(1400)
    base = _conduction(tc.RB_OMEGA)
    off = np.abs(planes / base - 1).max()
    print(f"Ra 1400: largest |plane sum / conduction - 1| = {off:.3e}; convective part {np.abs(conv).max():.3e}")
    assert off <= 5 * MEASURED_BELOW
    assert np.abs(conv).max() < 1e-3
