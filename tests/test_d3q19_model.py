"""An independent D3Q19-BGK model against the D3Q19 restatement (CPU only).

oracle/lbm_oracle3d.c is written from the kernel's own tables (speed order,
OPP, the ten body-force lines), so an error the two share -- a wrong weight on
a z speed, a swapped opposite pair, a force sign -- passes every bitwise GPU
test.  Here the same step is built in float64 numpy from the definition of the
lattice alone:

  * the velocity set is every c in {-1, 0, 1}^3 with |c|^2 <= 2, the weights
    are 1/3, 1/18, 1/36 by |c|^2, and the opposite of a speed is found by
    searching for -c;
  * pull streaming is np.roll along c, periodic in x, y and z;
  * fluid cells relax to f_eq = w rho (1 + 3 c.u + 4.5 (c.u)^2 - 1.5 u^2) and
    gain c_x rho0 a / 18 (|c|^2 = 1) or / 36 (|c|^2 = 2); obstacle cells
    return every population to where it came from (out_k = s_opp(k)).

Only the place of a velocity in the population array is taken from
include/lbm3d_hip.h (its documented speed order, parsed from the header).

Measure: max |oracle - model| / (rho0 w_k) over all cells and speeds, on an
11 x 7 x 5 periodic box without walls, 8 % random obstacles, rho0 = 0.1, 2 %
population noise.

Measured (CPU, this test's own printout):
  clean, omega 1.7, a 0.002, 1 / 5 / 20 steps      5.9e-7 / 1.32e-6 / 1.324e-6
  clean, 20 steps, omega 0.6 / 1.0 / 1.95          3.5e-7 / 4.7e-7 / 3.3e-6
  clean, 20 steps, omega 1.7, a 0                  1.32e-6
BOUND = 8 x the clean 20-step figure of the base case = 8 x 1.324e-6 =
1.06e-5: the deviation is the rounding noise of an fp32 run (a few ulp of a
population of size rho0 w_k per step, no longer growing once the noise has
mixed), so a small multiple is enough; the other omegas and a = 0 are held to
the same bound (their largest figure, omega 1.95, is 0.31 of it).
Planted model errors, smallest deviation over 1 / 5 / 20 steps and its ratio to
BOUND (each must exceed 100):
  weight of speed 9 set to 1/36            1.75     1.6e5
  opposites of speeds 5 and 7 swapped      0.0445   4.2e3
  force sign on speed 15 flipped           4.0e-3   378
"""
from __future__ import annotations

import re

import numpy as np
import pytest

from conftest import ROOT
from lbm_amd import io as lio
from oracle import oracle

CLEAN_MEASURED = 1.324e-6       # base case, 20 steps (see the module docstring)
BOUND = 8 * CLEAN_MEASURED

NX, NY, NZ = 11, 7, 5
RHO0 = 0.1


def abi_speed_order():
    """[(cx, cy, cz)] by ABI speed index, from the speed table of include/lbm3d_hip.h."""
    text = (ROOT / "include" / "lbm3d_hip.h").read_text()
    table = text[text.index("Speed order"):text.index("opposite:")]
    rows = re.findall(r"(\d+) \(\s*([+-]?\d),\s*([+-]?\d),\s*([+-]?\d)\)", table)
    assert [int(r[0]) for r in rows] == list(range(19))
    return [(int(r[1]), int(r[2]), int(r[3])) for r in rows]


class Model:
    """D3Q19-BGK from its definition; populations float64[nz][ny][nx][19] in ABI order."""

    def __init__(self):
        vel = [(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1) if x * x + y * y + z * z <= 2]
        order = abi_speed_order()
        assert sorted(order) == sorted(vel) and len(vel) == 19   # the header lists exactly the D3Q19 set
        self.c = np.array(order, np.int64)                       # c[k] = (cx, cy, cz)
        n2 = (self.c ** 2).sum(1)
        self.w = np.array([{0: 1 / 3, 1: 1 / 18, 2: 1 / 36}[int(n)] for n in n2])
        self.opp = np.array([next(j for j in range(19) if tuple(self.c[j]) == tuple(-self.c[k])) for k in range(19)])
        # body force along +x per unit rho0 a
        self.g = self.c[:, 0] * np.where(n2 == 1, 1 / 18, 1 / 36)

    def step(self, f, obst, omega, accel):
        s = np.stack([np.roll(f[..., k], (self.c[k, 2], self.c[k, 1], self.c[k, 0]), axis=(0, 1, 2))
                      for k in range(19)], axis=-1)
        rho = s.sum(-1)
        with np.errstate(all="ignore"):
            u = (s @ self.c.astype(np.float64)) / rho[..., None]
        cu = u @ self.c.T.astype(np.float64)
        feq = self.w * rho[..., None] * (1 + 3 * cu + 4.5 * cu * cu - 1.5 * (u * u).sum(-1)[..., None])
        fluid = s + omega * (feq - s) + RHO0 * accel * self.g
        return np.where(obst[..., None] != 0, s[..., self.opp], fluid)

    def run(self, f, obst, omega, accel, steps):
        f = f.astype(np.float64)
        for _ in range(steps):
            f = self.step(f, obst, omega, accel)
        return f


def _wrong_weight():
    m = Model()
    m.w = m.w.copy()
    m.w[9] = 1 / 36
    return m


def _swapped_opposites():
    m = Model()
    m.opp = m.opp.copy()
    m.opp[[5, 7]] = m.opp[[7, 5]]
    return m


def _flipped_force():
    m = Model()
    m.g = m.g.copy()
    m.g[15] = -m.g[15]
    return m


def _state(omega, accel):
    p = lio.Params3D(NX, NY, NZ, 0, RHO0, accel, omega)
    rng = np.random.default_rng(1907)
    obst = (rng.random((NZ, NY, NX)) < 0.08).astype(np.uint8)
    c0 = (oracle.init_cells3d(p) * (1 + 0.02 * rng.standard_normal((NZ, NY, NX, 19)))).astype(np.float32)
    return p, obst, c0


def _deviation(model, p, obst, c0, steps):
    ref, _ = oracle.run3d(p, obst, steps, c0)
    got = model.run(c0, obst, float(np.float32(p.omega)), float(np.float32(p.accel)), steps)
    return float(np.max(np.abs(ref.astype(np.float64) - got) / (RHO0 * model.w)))


def test_model_is_d3q19():
    """The generated set has the lattice's isotropy: sum w = 1, sum w c = 0,
    sum w c_i c_j = delta_ij / 3 -- and the model conserves mass without a force."""
    m = Model()
    c = m.c.astype(np.float64)
    assert m.w.sum() == pytest.approx(1, abs=1e-15)
    assert np.allclose(m.w @ c, 0, atol=1e-15)
    assert np.allclose((m.w[:, None, None] * c[:, :, None] * c[:, None, :]).sum(0), np.eye(3) / 3, atol=1e-15)
    assert sorted(m.opp) == list(range(19)) and np.array_equal(m.opp[m.opp], np.arange(19))
    p, obst, c0 = _state(1.7, 0.0)
    out = m.run(c0, obst, 1.7, 0.0, 7)
    assert out.sum() == pytest.approx(c0.sum(dtype=np.float64), rel=1e-13)


@pytest.mark.parametrize("omega,accel", [(1.7, 0.002), (0.6, 0.002), (1.0, 0.002), (1.95, 0.002), (1.7, 0.0)])
def test_oracle3d_matches_independent_model(omega, accel):
    """The restatement stays within BOUND of the float64 model after 1, 5 and
    20 steps, at every omega and with and without the body force.  Measured
    clean deviation 1.324e-6 (base case, 20 steps), BOUND = 8 x that = 1.06e-5;
    planted errors reach 1.6e5, 4.2e3 and 378 x BOUND (module docstring)."""
    p, obst, c0 = _state(omega, accel)
    m = Model()
    for steps in (1, 5, 20):
        dev = _deviation(m, p, obst, c0, steps)
        print(f"D3Q19 oracle vs model: omega {omega} accel {accel} steps {steps}: {dev:.3e} (bound {BOUND:.3e})")
        assert dev < BOUND, (omega, accel, steps, dev)


@pytest.mark.parametrize("variant,make", [("weight of speed 9 = 1/36", _wrong_weight),
                                          ("opposites of speeds 5 and 7 swapped", _swapped_opposites),
                                          ("force sign on speed 15 flipped", _flipped_force)])
def test_planted_model_errors_are_seen(variant, make):
    """Each physics error the restatement could share with the kernel, planted
    in the model, moves the measure beyond 100 x BOUND at every step count:
    the comparison above would catch it in the restatement."""
    p, obst, c0 = _state(1.7, 0.002)
    m = make()
    for steps in (1, 5, 20):
        dev = _deviation(m, p, obst, c0, steps)
        print(f"D3Q19 planted error ({variant}) steps {steps}: {dev:.3e} = {dev / BOUND:.3g} x bound")
        assert dev > 100 * BOUND, (variant, steps, dev)


@pytest.mark.parametrize("z0,n", [(1, 3), (2, 1), (3, 4), (0, 5)])
def test_oracle3d_slab_step_equals_full_step(z0, n):
    """oracle.step3d_slab on planes [z0, z0 + n) (periodic in z) with one ghost
    plane each side gives the full step's planes bit for bit, and the slabs'
    |u| sums are those of their planes."""
    p, obst, c0 = _state(1.7, 0.002)
    full, _ = oracle.run3d(p, obst, 1, c0)
    zs = np.arange(z0 - 1, z0 + n + 1) % NZ
    out, tot = oracle.step3d_slab(p, c0[zs], obst[zs[1:-1]])
    assert np.array_equal(out.view(np.uint32), full[zs[1:-1]].view(np.uint32))
    assert np.isfinite(tot) and tot > 0
