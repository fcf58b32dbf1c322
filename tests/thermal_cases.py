"""Set-ups and the CPU loop shared by the buoyancy tests (tests/test_thermal_host.py,
tests/test_gpu_thermal.py, tests/test_gpu_thermal3d.py); no test lives here.

The CPU loop is the definition of Engine.run_thermal at stride 1, from pieces that are pinned
elsewhere: the kick (lio.buoyancy_kick[3d]), one flow step of the oracle, the scalar step
(lio.scalar_step[3d]) over lio.macroscopic[3d] of the stepped lattice, then the fixed list.
"""
from __future__ import annotations

import math

import numpy as np

from lbm_amd import io as lio
from oracle import oracle


def b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(b32(a), b32(b))


def random_state(shape, q, qs, density, seed, obstacles=0.1):
    """(obst, cells, g) of a domain of that shape (slowest axis first): about 10 % random obstacles, a 5 %
    perturbed rest equilibrium with a few -0.0f populations on obstacle cells, and a random scalar whose
    populations are perturbed too (phi in about [-1, 1])."""
    rng = np.random.default_rng(seed)
    obst = (rng.random(shape) < obstacles).astype(np.uint8)
    if q == 9:
        eq = lio.init_cells(lio.Params(shape[1], shape[0], 0, 10, density, 0.0, 1.0))
        init = lio.scalar_init
    else:
        eq = oracle.init_cells3d(lio.Params3D(shape[2], shape[1], shape[0], 0, density, 0.0, 1.0))
        init = lio.scalar_init3d
    cells = (eq * (1 + 0.05 * rng.standard_normal(shape + (q,)))).astype(np.float32)
    cells[obst != 0, 1::3] = np.float32(-0.0)
    g = init((2 * rng.random(shape) - 1).astype(np.float32))
    g = (g * (1 + 0.1 * rng.standard_normal((qs,) + shape))).astype(np.float32)
    return obst, cells, g


# ---------------------------------------------------------------- the loop ----

def cpu_thermal(p, obst, cells, g, omega_s, s, phi_ref, fixed, steps, dims=2, kick=None):
    """`steps` times: kick, one oracle step, the scalar step over the stepped lattice's velocity, the
    fixed list.  Returns (cells, g).  kick: a replacement of lio.buoyancy_kick[3d] (planted errors)."""
    cells = np.ascontiguousarray(cells, np.float32)
    if dims == 2:
        kick = kick or lio.buoyancy_kick
        for _ in range(steps):
            cells = kick(cells, g, obst, p.density, s, phi_ref)
            cells, _ = oracle.step(p, cells, obst)
            ux, uy = lio.macroscopic(p, obst, cells)[:2]
            g = lio.scalar_step(g, ux, uy, obst, omega_s)
            if fixed is not None:
                g = lio.scalar_apply_fixed(g, *fixed)
    else:
        kick = kick or lio.buoyancy_kick3d
        for _ in range(steps):
            cells = kick(cells, g, obst, p.density, s, phi_ref)
            cells, _ = oracle.run3d(p, obst, 1, cells)
            ux, uy, uz = lio.macroscopic3d(p, obst, cells)[:3]
            g = lio.scalar_step3d(g, ux, uy, uz, obst, omega_s)
            if fixed is not None:
                g = lio.scalar_apply_fixed3d(g, *fixed)
    return cells, g


# ------------------------------------------------------- heated vertical slot ----

SLOT_NX, SLOT_ACCEL, SLOT_DENSITY = 34, 1e-4, 0.8


def slot(dims=2):
    """The heated slot: 34 x 4 (x 4) cells, obstacle columns (planes) at x = 0 and x = 33, omega = omega_s = 1,
    no body force; phi0 = 0.5 - (x - 1) / 31 with the columns x = 1 and x = 32 fixed at +0.5 and -0.5; gravity
    along the last axis that is not x.  The density is not 1, so that a missing density factor shows.
    Returns (p, obst, cells0, phi0, fixed, s)."""
    nx = SLOT_NX
    x = np.arange(nx, dtype=np.float64)
    line = (0.5 - (x - 1) / 31).astype(np.float32)
    if dims == 2:
        p = lio.Params(nx, 4, 0, 10, SLOT_DENSITY, 0.0, 1.0)
        shape = (4, nx)
        cells0 = lio.init_cells(p)
        s = (0.0, SLOT_ACCEL)
    else:
        p = lio.Params3D(nx, 4, 4, 0, SLOT_DENSITY, 0.0, 1.0)
        shape = (4, 4, nx)
        cells0 = oracle.init_cells3d(p)
        s = (0.0, 0.0, SLOT_ACCEL)
    obst = np.zeros(shape, np.uint8)
    obst[..., 0] = obst[..., -1] = 1
    phi0 = np.broadcast_to(line, shape).copy()
    held = np.zeros(shape, bool)
    held[..., 1] = held[..., 32] = True
    idx = np.argwhere(held)                                                        # columns (z,) y, x
    coords = [idx[:, dims - 1 - k].astype(np.int32) for k in range(dims)]          # x, y[, z]
    value = np.where(coords[0] == 1, 0.5, -0.5).astype(np.float32)
    return p, obst, cells0, phi0, tuple(coords) + (value,), s


def slot_exact():
    """u(x) along gravity for x = 1 .. 32: a / (6 nu L) (xi^3 - (H/2)^2 xi), xi = x - 16.5, L = 31, H = 32,
    nu = 1/6: the steady balance nu u'' = a xi / L with no slip at the half-way walls xi = +-16."""
    xi = np.arange(1, 33, dtype=np.float64) - 16.5
    return SLOT_ACCEL / (6 * (1 / 6) * 31) * (xi ** 3 - 16.0 ** 2 * xi)


def slot_error(dims=2, steps=3000, kick=None):
    """(max |u - exact| / max |exact| over the fluid cells, max |u across| , max |phi - phi0|) after
    `steps` steps of the CPU loop."""
    p, obst, cells, phi0, fixed, s = slot(dims)
    g = (lio.scalar_init if dims == 2 else lio.scalar_init3d)(phi0)
    g = (lio.scalar_apply_fixed if dims == 2 else lio.scalar_apply_fixed3d)(g, *fixed)
    cells, g = cpu_thermal(p, obst, cells, g, 1.0, s, 0.0, fixed, steps, dims, kick)
    u = (lio.macroscopic if dims == 2 else lio.macroscopic3d)(p, obst, cells)
    along, across = u[dims - 1].astype(np.float64), u[0].astype(np.float64)
    exact = slot_exact()
    err = np.abs(along[..., 1:33] - exact).max() / np.abs(exact).max()
    drift = np.abs(lio.scalar_phi(g).astype(np.float64) - phi0)[..., 1:33].max()
    return float(err), float(np.abs(across).max()), float(drift)


# ------------------------------------------------------- Rayleigh-Benard onset ----

RB_NX, RB_NY, RB_OMEGA, RB_HEIGHT = 40, 22, 1.4, 19.5


def rb_accel(ra):
    """a = Ra nu D / 19.5^3 for omega = omega_s = 1.4 and a scalar difference of 1."""
    nu = (1.0 / RB_OMEGA - 0.5) / 3.0
    return ra * nu * lio.scalar_diffusivity(RB_OMEGA, 2) / RB_HEIGHT ** 3


def rayleigh_benard(ra):
    """40 x 22, obstacle rows y = 0 and y = 21, omega = omega_s = 1.4, no body force, density 1; the rows
    y = 1 and y = 20 fixed at +0.5 (hot, below) and -0.5; phi0 the linear profile between them plus
    1e-3 sin(2 pi x / 40) sin(pi (y - 1) / 19); gravity impulse s = (0, a).
    Returns (p, obst, cells0, phi0, fixed, s)."""
    nx, ny = RB_NX, RB_NY
    p = lio.Params(nx, ny, 0, 10, 1.0, 0.0, RB_OMEGA)
    obst = np.zeros((ny, nx), np.uint8)
    obst[0] = obst[-1] = 1
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    phi0 = (0.5 - (y - 1) / 19 + 1e-3 * np.sin(2 * math.pi * x / nx) * np.sin(math.pi * (y - 1) / 19)).astype(np.float32)
    fx = np.concatenate([np.arange(nx), np.arange(nx)]).astype(np.int32)
    fy = np.concatenate([np.full(nx, 1), np.full(nx, ny - 2)]).astype(np.int32)
    value = np.where(fy == 1, 0.5, -0.5).astype(np.float32)
    phi0[1], phi0[ny - 2] = np.float32(0.5), np.float32(-0.5)
    return p, obst, lio.init_cells(p), phi0, (fx, fy, value), (0.0, rb_accel(ra))


def rb_growth_cpu(ra, kick=None):
    """(max |u_x| at step 4000 / max |u_x| at step 2000, min rho, max rho over the fluid at step 4000)."""
    p, obst, cells, phi0, fixed, s = rayleigh_benard(ra)
    g = lio.scalar_apply_fixed(lio.scalar_init(phi0), *fixed)
    cells, g = cpu_thermal(p, obst, cells, g, RB_OMEGA, s, 0.0, fixed, 2000, 2, kick)
    u2000 = np.abs(lio.macroscopic(p, obst, cells)[0]).max()
    cells, g = cpu_thermal(p, obst, cells, g, RB_OMEGA, s, 0.0, fixed, 2000, 2, kick)
    u4000 = np.abs(lio.macroscopic(p, obst, cells)[0]).max()
    rho = cells.astype(np.float64).sum(axis=-1)[obst == 0]
    return float(u4000) / float(u2000), float(rho.min()), float(rho.max())
