"""Set-ups and the CPU loops shared by the sub-grid model's tests (tests/test_sgs_host.py,
tests/test_gpu_sgs.py, tests/test_gpu_sgs3d.py); no test lives here.

The CPU loop is the definition of Engine.run_les from pieces pinned elsewhere: per chunk of n steps the
forcing zones (lio.forcing_kick[3d], n), n flow steps of the oracle, then the filter (lio.sgs_filter[3d], n).
"""
from __future__ import annotations

import math

import numpy as np

import forcing_cases as fc
from lbm_amd import io as lio
from oracle import oracle

b32, same = fc.b32, fc.same

W2 = (4 / 9,) + (1 / 9,) * 4 + (1 / 36,) * 4
W3 = tuple(1 / 3 if k == 0 else (1 / 18 if sum(abs(c) for c in e) == 1 else 1 / 36) for k, e in enumerate(lio.E3))


def params(shape, omega, density=1.0):
    """lio.Params / Params3D of a domain of that shape (slowest axis first), no inlet acceleration."""
    if len(shape) == 2:
        return lio.Params(shape[1], shape[0], 0, 10, density, 0.0, omega)
    return lio.Params3D(shape[2], shape[1], shape[0], 0, density, 0.0, omega)


def equilibrium(rho, u):
    """float32 AoS cells of the second-order equilibrium of rho and u = (ux, uy[, uz]) (float64 arrays)."""
    dims = len(u)
    e, w = (lio.E2, W2) if dims == 2 else (lio.E3, W3)
    usq = sum(c * c for c in u)
    out = np.empty(np.shape(rho) + (len(e),), np.float64)
    for k, ek in enumerate(e):
        eu = sum(c * v for c, v in zip(ek, u))
        out[..., k] = w[k] * rho * (1 + 3 * eu + 4.5 * eu * eu - 1.5 * usq)
    return out.astype(np.float32)


def step(p, obst, cells, n=1):
    """n oracle steps."""
    if cells.ndim == 3:
        for _ in range(n):
            cells, _ = oracle.step(p, cells, obst)
        return cells
    return oracle.run3d(p, obst, n, cells)[0]


def filt(dims):
    return lio.sgs_filter if dims == 2 else lio.sgs_filter3d


def random_coef(shape, mode, seed, fields, omega=1.7, idle=0.3):
    """A coefficient for `mode`: a constant, or (fields) an array of which a share `idle` of the cells is
    switched off (Cs = 0, or the rate omega itself)."""
    rng = np.random.default_rng(seed)
    if mode == "smagorinsky":
        if not fields:
            return float(np.float32(0.1 + 0.2 * rng.random()))
        return ((0.05 + 0.3 * rng.random(shape)) * (rng.random(shape) >= idle)).astype(np.float32)
    if not fields:
        return float(np.float32(0.8 + 0.6 * rng.random()))
    w = (0.8 + 0.95 * rng.random(shape)).astype(np.float32)       # up to 1.75: three steps from 1.7 stay below 2
    w[rng.random(shape) < idle] = np.float32(omega)
    return w


def cpu_les(p, obst, cells, mode, coef, steps, stride=1, zones=(), sgs=None):
    """`steps` steps in chunks of n <= stride: every zone (ascending index, n), n oracle steps, the filter (n).
    sgs: a replacement of lio.sgs_filter[3d] (planted errors).  Returns (cells, nut of the last application)."""
    cells = np.ascontiguousarray(cells, np.float32)
    dims = cells.ndim - 1
    sgs = sgs or filt(dims)
    nut, done = np.zeros(cells.shape[:-1], np.float32), 0
    while done < steps:
        n = min(stride, steps - done)
        if zones:
            cells, _ = fc.restate(cells, obst, zones, float(n))
        cells = step(p, obst, cells, n)
        cells, nut = sgs(cells, obst, p.omega, mode, coef, float(n))
        done += n
    return cells, nut


# ----------------------------------------------------- the shear wave ----

WAVE_OMEGA0, WAVE_OMEGA1, WAVE_STEPS = 1.7, 1.2, 200


def shear_wave(dims=2, omega=WAVE_OMEGA0):
    """32 x 8 (x 4), periodic: u_x = 0.02 sin(2 pi y / 8), a cross flow u_y = 0.01, density 1, two obstacle
    cells.  Returns (p, obst, cells0)."""
    shape = (8, 32) if dims == 2 else (4, 8, 32)
    p = params(shape, omega)
    y = np.arange(8, dtype=np.float64).reshape((8, 1) if dims == 2 else (1, 8, 1))
    ux = np.broadcast_to(0.02 * np.sin(2 * math.pi * y / 8), shape)
    u = [ux, np.full(shape, 0.01)] + ([np.zeros(shape)] if dims == 3 else [])
    obst = np.zeros(shape, np.uint8)
    obst[..., 2, 5] = obst[..., 6, 20] = 1
    return p, obst, equilibrium(np.ones(shape), u)


def wave_gap(dims=2, sgs=None, run=None, steps=WAVE_STEPS):
    """max |a - b| over all populations after 200 steps: a from "one step at omega0 = 1.7, then the filter OMEGA
    1.2, n = 1" (the CPU loop, or `run(p, obst, cells0, steps)`, the device's), b from as many oracle steps at
    omega = 1.2."""
    p, obst, cells0 = shear_wave(dims)
    if run is None:
        a, _ = cpu_les(p, obst, cells0, "omega", WAVE_OMEGA1, steps, sgs=sgs)
    else:
        a = run(p, obst, cells0, steps)
    b = step(shear_wave(dims, WAVE_OMEGA1)[0], obst, cells0, steps)
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


# ------------------------------------------------------------ the slot ----

SLOT_F, SLOT_CS, SLOT_OMEGA, SLOT_STEPS, SLOT_DENSITY = 2e-5, 1.2, 1.8, 12000, 0.8
SLOT_NU0 = (1 / SLOT_OMEGA - 0.5) / 3


def slot(dims=2):
    """18 x 4 (x 4), obstacle columns at x = 0 and 17, omega = 1.8, density 0.8, at rest; one whole-domain
    forcing zone with the acceleration 2e-5 along the last axis that is not x.  Returns (p, obst, cells0,
    [zone])."""
    shape = (4, 18) if dims == 2 else (4, 4, 18)
    p = params(shape, SLOT_OMEGA, SLOT_DENSITY)
    obst = np.zeros(shape, np.uint8)
    obst[..., 0] = obst[..., -1] = 1
    cells0 = equilibrium(np.full(shape, SLOT_DENSITY), [np.zeros(shape)] * dims)
    force = [0.0] * dims
    force[-1] = SLOT_F
    return p, obst, cells0, [fc.zone(0, (0,) * dims, shape[::-1], 0.0, None, force)]


def slot_exact(cs=SLOT_CS):
    """u(x) along the force for x = 1 .. 16, xi = x - 8.5, no slip at the half-way walls xi = +-8.  The steady
    balance (nu0 + Cs^2 |u'|) |u'| = f |xi| gives |u'| = (-nu0 + sqrt(nu0^2 + 4 Cs^2 f |xi|)) / (2 Cs^2), whose
    integral from the wall is closed: with g(s) = sqrt(nu0^2 + 4 Cs^2 f s), the primitive of |u'| is
    (-nu0 s + g^3 / (6 Cs^2 f)) / (2 Cs^2).  cs = 0: Poiseuille."""
    xi = np.abs(np.arange(1, 17, dtype=np.float64) - 8.5)
    if cs == 0:
        return SLOT_F / (2 * SLOT_NU0) * (8.0 ** 2 - xi ** 2)
    c2 = cs * cs

    def prim(s):
        return (-SLOT_NU0 * s + (SLOT_NU0 ** 2 + 4 * c2 * SLOT_F * s) ** 1.5 / (6 * c2 * SLOT_F)) / (2 * c2)
    return prim(8.0) - prim(xi)


def slot_profile_error(p, obst, cells, dims):
    """(max |u - exact| / max exact over the fluid cells, max |u across|)."""
    u = (lio.macroscopic if dims == 2 else lio.macroscopic3d)(p, obst, cells)
    along, across = u[dims - 1].astype(np.float64), u[0].astype(np.float64)
    exact = slot_exact()
    return float(np.abs(along[..., 1:17] - exact).max() / exact.max()), float(np.abs(across).max())


def slot_error(dims=2, sgs=None, steps=SLOT_STEPS):
    p, obst, cells, zones = slot(dims)
    cells, _ = cpu_les(p, obst, cells, "smagorinsky", SLOT_CS, steps, zones=zones, sgs=sgs)
    return slot_profile_error(p, obst, cells, dims)


def laminar_distance():
    """max |Poiseuille - exact| / max exact: what a dead filter would show."""
    return float(np.abs(slot_exact(0) - slot_exact()).max() / slot_exact().max())
