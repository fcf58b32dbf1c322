"""Set-ups, boxes and the CPU loop shared by the forcing-zone tests (tests/test_forcing_host.py,
tests/test_gpu_forcing.py, tests/test_gpu_forcing3d.py); no test lives here.

A zone is a dict(index, origin, shape, lam, target, force): origin = (x0, y0[, z0]), shape = (w, h[, d]),
lam and each component of target and force a number or a float32 array of the box's shape, slowest axis
first -- the keywords of Engine.forcing_zone.  The CPU loop is the definition of Engine.run_forced at
stride 1 from pieces pinned elsewhere: the zones applied in index order (lio.forcing_kick[3d]), then one
flow step of the oracle.
"""
from __future__ import annotations

import math

import numpy as np

import thermal_cases as tc
from lbm_amd import io as lio
from oracle import oracle

b32, same = tc.b32, tc.same


def zone(index, origin, shape, lam=0.0, target=None, force=None):
    dims = len(origin)
    return dict(index=index, origin=tuple(origin), shape=tuple(shape), lam=lam,
                target=[0.0] * dims if target is None else list(target),
                force=[0.0] * dims if force is None else list(force))


def coef_of(z):
    """The zone's coefficients in header order (lam, ut.., f..): what lio.forcing_kick takes."""
    return [z["lam"]] + list(z["target"]) + list(z["force"])


def box_of(z):
    return tuple(z["origin"]) + tuple(z["shape"])


def restate(cells, obst, zones, n):
    """(cells after every zone in ascending index order, {index: terms}) of one forcing_apply(n)."""
    dims = cells.ndim - 1
    kick = lio.forcing_kick if dims == 2 else lio.forcing_kick3d
    terms = {}
    for z in sorted(zones, key=lambda z: z["index"]):
        cells, terms[z["index"]] = kick(cells, obst, box_of(z), coef_of(z), n)
    return cells, terms


def set_zones(e, zones):
    for z in zones:
        e.forcing_zone(**z)


def fold_bound(terms):
    """a sum of n terms folded in fp64 lies within 2 (n - 1) 2^-53 sum|term| of the exact sum."""
    t = np.abs(np.asarray(terms, np.float64)).ravel()
    return 2.0 * max(t.size - 1, 0) * 2.0 ** -53 * math.fsum(t.tolist())


def check_impulse(impulse, terms, what=""):
    """impulse float64[8][dims] of one apply against {index: terms}: within the fold bound of fsum, rows of
    unset zones zero."""
    dims = impulse.shape[1]
    for i in range(impulse.shape[0]):
        if i not in terms:
            assert not impulse[i].any(), (what, i)
            continue
        for c in range(dims):
            t = terms[i][..., c].astype(np.float64).ravel()
            want = math.fsum(t.tolist())
            assert abs(impulse[i, c] - want) <= fold_bound(t), (what, i, c, impulse[i, c], want, fold_bound(t))


# ------------------------------------------------------------------ boxes ----

def boxes2d(nx, ny):
    """(x0, y0, w, h): the whole domain, boxes whose x edges cut quads in every way, a single cell."""
    out = [(0, 0, nx, ny), (0, ny // 2, 1, 1)]
    for x0, w in ((1, 5), (4, 4), (3, 2), (nx - 3, 3)):
        if x0 >= 0 and x0 + w <= nx:
            out.append((x0, min(1, ny - 1), w, max(1, ny - 2)))
    return out


def boxes3d(nx, ny, nz):
    out = []
    for x0, y0, w, h in boxes2d(nx, ny):
        for z0, d in ((0, nz), (1, 1), (nz - 1, 1)):
            if 0 <= z0 < nz and (x0, y0, z0, w, h, d) not in out:
                out.append((x0, y0, z0, w, h, d))
    return out


def random_coefs(dims, ext, seed, fields, idle=0.0):
    """(lam, target, force): constants, or (fields) arrays over the box `ext` (slowest axis first) of which a
    share `idle` of the cells has lam = 0 and force = 0."""
    rng = np.random.default_rng(seed)
    if not fields:
        return (float(np.float32(0.3 * rng.random())), [float(np.float32(0.05 * v)) for v in rng.standard_normal(dims)],
                [float(np.float32(1e-3 * v)) for v in rng.standard_normal(dims)])
    live = rng.random(ext) >= idle
    lam = (1.5 * rng.random(ext) * live).astype(np.float32)                  # some cells past the clamp l = 1
    target = [(0.05 * rng.standard_normal(ext)).astype(np.float32) for _ in range(dims)]
    force = [(1e-3 * rng.standard_normal(ext) * live).astype(np.float32) for _ in range(dims)]
    return lam, target, force


def box_zone(index, box, seed, fields, idle=0.0):
    dims = len(box) // 2
    lam, target, force = random_coefs(dims, box[dims:][::-1], seed, fields, idle)
    return zone(index, box[:dims], box[dims:], lam, target, force)


def random_state(shape, density, seed, obstacles=0.1):
    """(obst, cells): about 10 % obstacles, a 5 % perturbed rest equilibrium, -0.0f populations on obstacles."""
    q = 9 if len(shape) == 2 else 19
    obst, cells, _ = tc.random_state(shape, q, 5 if q == 9 else 7, density, seed, obstacles)
    return obst, cells


# --------------------------------------------------------------- the loop ----

def cpu_forced(p, obst, cells, zones, steps, dims=2, kick=None):
    """`steps` times: every zone (ascending index) with n = 1, then one oracle step.  kick: a replacement of
    lio.forcing_kick[3d] (planted errors).  Returns (cells, float64[8][dims] impulse of the last application)."""
    cells = np.ascontiguousarray(cells, np.float32)
    kick = kick or (lio.forcing_kick if dims == 2 else lio.forcing_kick3d)
    zones = sorted(zones, key=lambda z: z["index"])
    imp = np.zeros((8, dims))
    for _ in range(steps):
        for z in zones:
            cells, terms = kick(cells, obst, box_of(z), coef_of(z), 1.0)
            imp[z["index"]] = terms.astype(np.float64).reshape(-1, dims).sum(axis=0)
        if dims == 2:
            cells, _ = oracle.step(p, cells, obst)
        else:
            cells, _ = oracle.run3d(p, obst, 1, cells)
    return cells, imp


# ---------------------------------------------------------------- the slot ----

SLOT_F, SLOT_STEPS, NU = 1e-5, 6000, 1.0 / 6.0


def slot(dims=2, lam=0.0):
    """The geometry of thermal_cases.slot(): 34 x 4 (x 4), obstacle columns at x = 0 and 33, omega = 1,
    density 0.8, at rest; one whole-domain zone with the drag `lam` and the acceleration 1e-5 along the last
    axis that is not x.  Returns (p, obst, cells0, [zone])."""
    p, obst, cells0, *_ = tc.slot(dims)
    force = [0.0] * dims
    force[-1] = SLOT_F
    shape = (p.nx, p.ny) if dims == 2 else (p.nx, p.ny, p.nz)
    return p, obst, cells0, [zone(0, (0,) * dims, shape, lam, None, force)]


def slot_exact(lam=0.0):
    """u(x) along the force for x = 1 .. 32, xi = x - 16.5, no slip at xi = +-16: Poiseuille
    f / (2 nu) (16^2 - xi^2), or with a drag (Darcy-Brinkman) (f / lam) (1 - cosh(r xi) / cosh(16 r)),
    r = sqrt(lam / nu)."""
    xi = np.arange(1, 33, dtype=np.float64) - 16.5
    if lam == 0:
        return SLOT_F / (2 * NU) * (16.0 ** 2 - xi ** 2)
    r = math.sqrt(lam / NU)
    return SLOT_F / lam * (1 - np.cosh(r * xi) / math.cosh(16 * r))


def slot_profile_error(p, obst, cells, lam, dims):
    """(max |u - exact| / max exact over the fluid cells, max |u across|)."""
    u = (lio.macroscopic if dims == 2 else lio.macroscopic3d)(p, obst, cells)
    along, across = u[dims - 1].astype(np.float64), u[0].astype(np.float64)
    exact = slot_exact(lam)
    return float(np.abs(along[..., 1:33] - exact).max() / exact.max()), float(np.abs(across).max())


def slot_error(dims=2, lam=0.0, steps=SLOT_STEPS, kick=None):
    p, obst, cells, zones = slot(dims, lam)
    cells, _ = cpu_forced(p, obst, cells, zones, steps, dims, kick)
    return slot_profile_error(p, obst, cells, lam, dims)
