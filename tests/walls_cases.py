"""Shared set-ups of the scalar wall tests (tests/test_scalar_walls_host.py, tests/test_gpu_scalar_walls.py,
tests/test_gpu_scalar_walls3d.py): bit comparisons, random bodies, and the conduction slot -- two obstacle
rows (2-D) or planes (3-D) GAP fluid cells apart, WIDTH cells wide, each a body of its own -- advanced by the
numpy restatement of include/lbm_scalar_walls_hip.h."""
from __future__ import annotations

import functools
import math

import numpy as np

from lbm_amd import io as lio

GAP, WIDTH = 10, 4


def b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(b32(a), b32(b))


def fold_bound(terms):
    """a sum of n terms folded in fp64 lies within 2 (n - 1) 2^-53 sum|term| of the exact sum."""
    t = np.asarray(terms, np.float64).ravel()
    return 2.0 * max(t.size - 1, 0) * 2.0 ** -53 * math.fsum(np.abs(t).tolist())


def random_bodies(obst, seed, nb=7):
    """(labels, kinds, values): every blocked cell in one of the bodies 0 .. nb - 2 or in none (-1, -2) at
    random, so bodies are scattered cells; body nb - 1 has no cell; labels on fluid cells are noise, some
    >= nb (they are ignored); kinds cycle through adiabatic, value, flux, values have both signs."""
    rng = np.random.default_rng(seed)
    blocked = np.asarray(obst) != 0
    labels = rng.integers(-3, nb + 5, size=blocked.shape)
    labels[blocked] = rng.integers(-2, nb - 1, size=int(blocked.sum()))
    kinds = ((np.arange(nb) + int(rng.integers(3))) % 3).astype(np.int32)
    values = np.where(kinds == lio.WALL_FLUX, 0.02, 1.5) * rng.normal(size=nb)
    return labels.astype(np.int32), kinds, values.astype(np.float32)


def slot(dims, kinds=(lio.WALL_VALUE, lio.WALL_VALUE), values=(1.0, 0.0)):
    """(obst, labels, kinds, values, phi0) of the conduction slot: body 0 the low wall, body 1 the high one;
    the scalar starts at 0.5 everywhere."""
    shape = (GAP + 2,) + (WIDTH,) * (dims - 1)
    obst = np.zeros(shape, np.uint8)
    obst[0], obst[-1] = 1, 1
    labels = np.full(shape, -1, np.int32)
    labels[0], labels[-1] = 0, 1
    return (obst, labels, np.asarray(kinds, np.int32), np.asarray(values, np.float32),
            np.full(shape, 0.5, np.float32))


def advance(g, obst, labels, kinds, values, omega_s, steps, u=None, apply=None):
    """`steps` times lio.scalar_step[3d] (u: the frozen velocity components; None: at rest) and the wall pass
    (`apply`: a stand-in for lio.scalar_apply_walls[3d], for planted errors)."""
    d3 = g.ndim == 4
    zero = np.zeros(g.shape[1:], np.float32)
    u = (zero,) * (3 if d3 else 2) if u is None else u
    step = lio.scalar_step3d if d3 else lio.scalar_step
    apply = apply or (lio.scalar_apply_walls3d if d3 else lio.scalar_apply_walls)
    for _ in range(steps):
        g = apply(step(g, *u, obst, omega_s), obst, labels, kinds, values)
    return g


@functools.lru_cache(maxsize=None)
def conduction(dims, omega_s, steps, kinds=(lio.WALL_VALUE, lio.WALL_VALUE), values=(1.0, 0.0)):
    """The slot after `steps` steps from phi = 0.5: (g, phi along the gap through the first column)."""
    obst, labels, kinds, values, phi0 = slot(dims, kinds, values)
    g = advance((lio.scalar_init3d if dims == 3 else lio.scalar_init)(phi0), obst, labels, kinds, values, omega_s,
                steps)
    g.setflags(write=False)
    phi = lio.scalar_phi(g)
    return g, (phi[:, 0, 0] if dims == 3 else phi[:, 0]).astype(np.float64)


def linear_profile(hot=1.0, cold=0.0):
    """phi of the GAP fluid cells with the walls halfway between the wall cells and their fluid neighbours."""
    y = np.arange(1, GAP + 1) - 0.5
    return hot + (cold - hot) * y / GAP
