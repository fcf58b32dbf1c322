"""Host side of the passive scalar (include/lbm_scalar_hip.h; CPU only).

* The header declares exactly native.EXPORTED_SCALAR, all exported by the
  library and disjoint from the other headers' lists; the ABI version stays 5.
* The numpy restatement the GPU tests compare against (lio.scalar_init /
  scalar_step / scalar_phi / scalar_apply_fixed / scalar_stats and their 3-D
  twins) is pinned by physics, not against itself: a sine wave on a uniform
  flow decays as exp(-D k^2 t) and travels u t cells (amplitude within 2 %,
  shift within 0.1 cell), and the total is conserved among random obstacles
  (5e-5 relative over 200 steps); nothing leaves a closed shell of obstacle
  cells (exactly 0: any permutation of the opposites conserves the total, only
  the reversal keeps the wall tight).  A planted wrong weight or wrong opposite
  breaks one of those pins.
* lbm_scalar_step_ref and its 3-D twin -- the C++ per-cell function of the
  kernels, compiled for the host -- equal the restatement bit for bit (uint32
  patterns) on random states with obstacles.
* The contract that needs no GPU: NULL handles, the arguments of the _ref
  functions.  (The fixed-list checks of a live handle -- out of range,
  duplicates, n = 0 -- need a handle and are in tests/test_gpu_scalar.py; the
  list semantics of the restatement are pinned here.)
"""
from __future__ import annotations

import math
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lbm_amd import io as lio
from lbm_amd import native


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------- exports ----

def test_library_exports_every_scalar_symbol():
    text = (ROOT / "include" / "lbm_scalar_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 16 and sorted(native.EXPORTED_SCALAR) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    assert L.lbm_abi_version() == 5
    others = (set(native.EXPORTED) | set(native.EXPORTED3D) | set(native.EXPORTED3D_FIELDS)
              | set(native.EXPORTED_FORCES) | set(native.EXPORTED_AVERAGES) | set(native.EXPORTED_GRADIENTS)
              | set(native.EXPORTED_STRESS) | set(native.EXPORTED_BINNED) | set(native.EXPORTED_TRACERS))
    assert not set(syms) & others
    assert re.search(rf"\bLBM_SCALAR_MAX_PARTS = {native.SCALAR_MAX_PARTS}\b", text)
    assert (native.SCALAR_Q, native.SCALAR_Q3D) == (len(lio.SCALAR_OPP), len(lio.SCALAR_OPP3D)) == (5, 7)


def test_null_handle_is_invalid():
    L = native.load_library()
    for pre, extra in (("lbm_", ()), ("lbm3d_", (None,))):
        assert getattr(L, pre + "scalar_begin")(None, 1.0, None) == native.LBM_E_INVALID
        assert getattr(L, pre + "scalar_set_fixed")(None, 0, None, None, *extra, None) == native.LBM_E_INVALID
        assert getattr(L, pre + "scalar_advance")(None, 1) == native.LBM_E_INVALID
        assert getattr(L, pre + "scalar_steps")(None, None) == native.LBM_E_INVALID
        assert getattr(L, pre + "scalar_store")(None, None, None) == native.LBM_E_INVALID
        assert getattr(L, pre + "scalar_stats")(None, None, None, None) == native.LBM_E_INVALID
        assert getattr(L, pre + "scalar_end")(None) == native.LBM_E_INVALID


# ---------------------------------------------------------- physics pins ----

# (nx, ny, axis of the wave: 0 = x, 1 = y, omega_s, u along the wave, steps)
WAVES2 = [(32, 8, 0, 1.0, 0.0, 200), (32, 8, 0, 1.6, 0.0, 200), (8, 32, 1, 1.2, 0.0, 200),
          (32, 8, 0, 1.0, 0.05, 320), (64, 8, 0, 1.5, 0.1, 320), (8, 32, 1, 1.5, -0.1, 160)]
# 32 cells along the wave's axis (0 = x, 1 = y, 2 = z), 4 along the others
WAVES3 = [(0, 1.0, 0.0, 200), (1, 1.6, 0.0, 200), (2, 1.2, 0.0, 200),
          (0, 1.0, 0.05, 320), (1, 1.5, 0.1, 320), (2, 1.5, 0.1, 160), (2, 1.2, 0.05, 160)]
AMP_TOL, SHIFT_TOL = 0.02, 0.1


def _fundamental(phi, array_axis):
    """(amplitude, phase) of the fundamental along array_axis, averaged over the other axes."""
    line = phi.astype(np.float64)
    for ax in reversed(range(phi.ndim)):
        if ax != array_axis:
            line = line.mean(axis=ax)
    n = line.size
    c = np.fft.rfft(line)[1]
    return 2.0 * abs(c) / n, math.atan2(c.imag, c.real)


def _wave_errors(shape, array_axis, omega_s, u, steps):
    """Relative amplitude error and shift error (cells) of a sine on a uniform flow along array_axis."""
    dims = len(shape)
    n = shape[array_axis]
    idx = np.arange(n, dtype=np.float64).reshape([-1 if a == array_axis else 1 for a in range(dims)])
    phi0 = np.broadcast_to(1.0 + 0.5 * np.sin(2.0 * np.pi * idx / n), shape).astype(np.float32)
    comp = dims - 1 - array_axis                      # velocity component moving along that array axis
    vel = [np.full(shape, u if c == comp else 0.0, np.float32) for c in range(dims)]
    obst = np.zeros(shape, np.uint8)
    init, step = (lio.scalar_init, lio.scalar_step) if dims == 2 else (lio.scalar_init3d, lio.scalar_step3d)
    g = init(phi0)
    a0, ph0 = _fundamental(lio.scalar_phi(g), array_axis)
    for _ in range(steps):
        g = step(g, *vel, obst, omega_s)
    a1, ph1 = _fundamental(lio.scalar_phi(g), array_axis)
    k = 2.0 * np.pi / n
    want = a0 * math.exp(-lio.scalar_diffusivity(omega_s, dims) * k * k * steps)
    shift = -(ph1 - ph0) / k                          # cells moved, modulo n
    err = (shift - u * steps + n / 2) % n - n / 2
    return abs(a1 / want - 1.0), abs(err), lio.scalar_phi(g)


def _pins_hold():
    """Every physics pin and the conservation pin, as one predicate (the planted-error tests reuse it)."""
    for nx, ny, axis, om, u, steps in WAVES2:
        ea, es, _ = _wave_errors((ny, nx), 1 - axis, om, u, steps)
        if not (ea < AMP_TOL and es < SHIFT_TOL):
            return False
    axis, om, u, steps = WAVES3[3]
    ea, es, _ = _wave_errors(tuple(32 if a == 2 - axis else 4 for a in range(3)), 2 - axis, om, u, steps)
    if not (ea < AMP_TOL and es < SHIFT_TOL):
        return False
    if not (_conservation_drift() < CONS_TOL and _conservation_drift3d() < CONS_TOL):
        return False
    return _enclosure_leak(2)[0] == 0.0 and _enclosure_leak(3)[0] == 0.0


@pytest.mark.parametrize("nx,ny,axis,omega_s,u,steps", WAVES2)
def test_wave_decays_and_travels_2d(nx, ny, axis, omega_s, u, steps):
    ea, es, phi = _wave_errors((ny, nx), 1 - axis, omega_s, u, steps)
    print(f"2-D {nx}x{ny} axis {axis} omega_s {omega_s} u {u} steps {steps}: amplitude error {ea:.4f}, "
          f"shift error {es:.4f} cells")
    assert phi.dtype == np.float32 and phi.shape == (ny, nx)
    assert ea < AMP_TOL and es < SHIFT_TOL


@pytest.mark.parametrize("axis,omega_s,u,steps", WAVES3)
def test_wave_decays_and_travels_3d(axis, omega_s, u, steps):
    shape = tuple(32 if a == 2 - axis else 4 for a in range(3))     # [nz][ny][nx]
    ea, es, phi = _wave_errors(shape, 2 - axis, omega_s, u, steps)
    print(f"3-D axis {axis} omega_s {omega_s} u {u} steps {steps}: amplitude error {ea:.4f}, shift error {es:.4f}")
    assert phi.dtype == np.float32 and phi.shape == shape
    assert ea < AMP_TOL and es < SHIFT_TOL


def test_diffusivity_of_a_relaxation_rate():
    for dims, c in ((2, 3.0), (3, 4.0)):
        for om in (0.6, 1.0, 1.5, 1.9):
            assert lio.scalar_diffusivity(om, dims) == (1.0 / om - 0.5) / c


# ---------------------------------------------------------- conservation ----

CONS_TOL = 5e-5


def _random_flow(shape, seed, obstacles=0.1, scale=0.05):
    rng = np.random.default_rng(seed)
    vel = [(scale * rng.standard_normal(shape)).astype(np.float32) for _ in shape]
    obst = (rng.random(shape) < obstacles).astype(np.uint8)
    for v in vel:
        v[obst != 0] = 0                              # what fields() gives at an obstacle
    phi0 = (1.0 + rng.random(shape)).astype(np.float32)
    return vel, obst, phi0


def _total(g):
    return math.fsum(lio.scalar_phi(g).astype(np.float64).ravel().tolist())


def _conservation_drift(steps=200):
    vel, obst, phi0 = _random_flow((19, 37), 11)
    g = lio.scalar_init(phi0)
    t0 = _total(g)
    for _ in range(steps):
        g = lio.scalar_step(g, *vel, obst, 1.3)
    return abs(_total(g) / t0 - 1.0)


def _conservation_drift3d(steps=50):
    vel, obst, phi0 = _random_flow((5, 7, 13), 12)
    g = lio.scalar_init3d(phi0)
    t0 = _total(g)
    for _ in range(steps):
        g = lio.scalar_step3d(g, *vel, obst, 1.3)
    return abs(_total(g) / t0 - 1.0)


def test_total_is_conserved_among_obstacles():
    d2, d3 = _conservation_drift(), _conservation_drift3d()
    print(f"relative drift of the total: 2-D 37x19, 200 steps: {d2:.2e}; 3-D 13x7x5, 50 steps: {d3:.2e}")
    assert d2 < CONS_TOL and d3 < CONS_TOL


def _enclosure_leak(dims, steps=40):
    """A closed shell of obstacle cells, one cell thick, around a chamber that holds phi = 1 in a
    random flow; phi = 0 outside.  What arrives at a shell cell along k leaves it along opp(k) and
    streams back to the cell it came from, so no population ever leaves the shell outwards: the sum of
    |phi| over the fluid cells outside is exactly 0 after any number of steps (zero is exact in fp32,
    so no tolerance), while any table that is not the reversal lets the scalar through the wall.  The
    total stays conserved for every permutation, so this is the pin of the opposites."""
    shape = (12, 16) if dims == 2 else (9, 10, 12)
    lo, hi = (2, 3), (8, 10)
    if dims == 3:
        lo, hi = (2, 2, 3), (6, 7, 9)
    box = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
    inner = tuple(slice(a + 1, b) for a, b in zip(lo, hi))
    obst = np.zeros(shape, np.uint8)
    obst[box] = 1
    obst[inner] = 0
    outside = np.ones(shape, bool)
    outside[box] = False
    phi0 = np.zeros(shape, np.float32)
    phi0[inner] = 1
    vel, _, _ = _random_flow(shape, 5, obstacles=0.0)
    for v in vel:
        v[obst != 0] = 0
    init, step = (lio.scalar_init, lio.scalar_step) if dims == 2 else (lio.scalar_init3d, lio.scalar_step3d)
    g = init(phi0)
    for _ in range(steps):
        g = step(g, *vel, obst, 1.4)
    phi = lio.scalar_phi(g)
    return float(np.abs(phi[outside]).sum()), float(phi[inner].mean())


def test_nothing_leaves_a_closed_shell():
    for dims in (2, 3):
        leak, held = _enclosure_leak(dims)
        assert leak == 0.0 and held > 0.5                # the chamber still holds the scalar


# -------------------------------------------------------- planted errors ----

def test_the_pins_hold_as_one_predicate():
    assert _pins_hold()


@pytest.mark.parametrize("name,value", [
    ("SCALAR_W", (np.float32(1) / np.float32(3), np.float32(0.16))),                 # a wrong moving weight
    ("SCALAR_W", (np.float32(0.5), np.float32(0.125))),                              # the D3Q7 weights in 2-D
    ("SCALAR_OPP", (0, 3, 4, 1, 1)),                   # S returns what E brought: the total is not conserved
    ("SCALAR_OPP", (0, 3, 2, 1, 4)),                   # N and S not reversed: the wall lets the scalar through
    ("SCALAR_OPP", (0, 1, 4, 3, 2)),                   # E and W not reversed
    ("SCALAR_W3D", (np.float32(0.25), np.float32(1) / np.float32(6))),
    ("SCALAR_OPP3D", (0, 2, 1, 4, 3, 5, 6)),           # +z and -z not reversed
    ("SCALAR_OPP3D", (0, 2, 1, 4, 3, 6, 6)),
])
def test_a_planted_error_breaks_a_pin(monkeypatch, name, value):
    monkeypatch.setattr(lio, name, value)
    assert not _pins_hold()


# ---------------------------------------------------- reference function ----

@pytest.mark.parametrize("nx,ny", [(37, 19), (64, 32), (1, 7), (7, 1), (4, 1)])
def test_step_ref_equals_the_restatement_2d(nx, ny):
    (ux, uy), obst, phi0 = _random_flow((ny, nx), 100 * nx + ny)
    rng = np.random.default_rng(nx + ny)
    g = (lio.scalar_init(phi0) * (1 + 0.2 * rng.standard_normal((5, ny, nx)))).astype(np.float32)
    for om in (0.7, 1.0, 1.85):
        for _ in range(3):
            want = lio.scalar_step(g, ux, uy, obst, om)
            got = native.scalar_step_ref(g, ux, uy, obst, om)
            assert got.dtype == np.float32 and np.array_equal(_b32(got), _b32(want)), (nx, ny, om)
            g = want
    assert obst.any() or nx * ny < 8


@pytest.mark.parametrize("nx,ny,nz", [(13, 7, 5), (16, 8, 8), (5, 4, 1)])
def test_step_ref_equals_the_restatement_3d(nx, ny, nz):
    (ux, uy, uz), obst, phi0 = _random_flow((nz, ny, nx), 100 * nx + 10 * ny + nz)
    rng = np.random.default_rng(nx + ny + nz)
    g = (lio.scalar_init3d(phi0) * (1 + 0.2 * rng.standard_normal((7, nz, ny, nx)))).astype(np.float32)
    for om in (0.7, 1.0, 1.85):
        for _ in range(3):
            want = lio.scalar_step3d(g, ux, uy, uz, obst, om)
            got = native.scalar_step3d_ref(g, ux, uy, uz, obst, om)
            assert np.array_equal(_b32(got), _b32(want)), (nx, ny, nz, om)
            g = want
    assert obst.any()


def test_step_ref_refuses_bad_arguments():
    L = native.load_library()
    f32p = native.ctypes.POINTER(native.ctypes.c_float)
    u8p = native.ctypes.POINTER(native.ctypes.c_uint8)
    g = np.ones((5, 3, 4), np.float32)
    out = np.full_like(g, 7)
    u = np.zeros((3, 4), np.float32)
    ob = np.zeros((3, 4), np.uint8)
    P = lambda a: a.ctypes.data_as(f32p)
    O = ob.ctypes.data_as(u8p)
    assert L.lbm_scalar_step_ref(4, 3, 1.0, P(u), P(u), O, P(g), P(out)) == native.LBM_OK
    out[...] = 7
    for om in (0.0, 2.0, -1.0, float("nan"), float("inf")):
        assert L.lbm_scalar_step_ref(4, 3, om, P(u), P(u), O, P(g), P(out)) == native.LBM_E_INVALID, om
    assert L.lbm_scalar_step_ref(0, 3, 1.0, P(u), P(u), O, P(g), P(out)) == native.LBM_E_INVALID
    assert L.lbm_scalar_step_ref(4, 3, 1.0, None, P(u), O, P(g), P(out)) == native.LBM_E_INVALID
    assert L.lbm_scalar_step_ref(4, 3, 1.0, P(u), P(u), None, P(g), P(out)) == native.LBM_E_INVALID
    assert L.lbm_scalar_step_ref(4, 3, 1.0, P(u), P(u), O, P(g), None) == native.LBM_E_INVALID
    assert L.lbm3d_scalar_step_ref(4, 3, 0, 1.0, P(u), P(u), P(u), O, P(g), P(out)) == native.LBM_E_INVALID
    assert L.lbm3d_scalar_step_ref(4, 3, 1, 1.0, P(u), P(u), None, O, P(g), P(out)) == native.LBM_E_INVALID
    assert (out == 7).all()
    with pytest.raises(ValueError):
        native.scalar_step_ref(g[:4], u, u, ob, 1.0)


# ------------------------------------------ begin state, fixed list, stats ----

def test_begin_state_fixed_list_and_stats_of_the_restatement():
    rng = np.random.default_rng(4)
    phi0 = rng.random((6, 9)).astype(np.float32)
    g = lio.scalar_init(phi0)
    third, sixth = np.float32(1) / np.float32(3), np.float32(1) / np.float32(6)
    assert g.shape == (5, 6, 9) and g.dtype == np.float32
    assert np.array_equal(_b32(g[0]), _b32(phi0 * third)) and all(np.array_equal(_b32(g[k]), _b32(phi0 * sixth))
                                                                   for k in range(1, 5))
    g3 = lio.scalar_init3d(np.broadcast_to(phi0, (2, 6, 9)))
    assert g3.shape == (7, 2, 6, 9) and np.array_equal(_b32(g3[0][1]), _b32(phi0 * np.float32(0.25)))
    assert np.array_equal(_b32(g3[6][0]), _b32(phi0 * np.float32(0.125)))
    # the fixed list overwrites exactly the listed cells with the begin state of the value
    x, y, v = np.array([0, 8, 3]), np.array([5, 0, 2]), np.array([2.0, -1.0, 0.5], np.float32)
    f = lio.scalar_apply_fixed(g, x, y, v)
    want = g.copy()
    for xi, yi, vi in zip(x, y, v):
        want[:, yi, xi] = lio.scalar_init(np.full((1, 1), vi, np.float32))[:, 0, 0]
    assert np.array_equal(_b32(f), _b32(want)) and not np.array_equal(f, g)
    f3 = lio.scalar_apply_fixed3d(g3, x, y, np.array([1, 0, 1]), v)
    assert np.array_equal(_b32(f3[:, 1, 5, 0]), _b32(lio.scalar_init3d(np.full((1, 1, 1), 2.0))[:, 0, 0, 0]))
    assert (f3 != g3).any(axis=0).sum() == 3
    # stats: the exact sum, the extremes over fluid cells, the identities without one
    obst = np.zeros((6, 9), np.uint8)
    obst[5, 0] = 1
    total, lo, hi = lio.scalar_stats(f, obst)
    phi = lio.scalar_phi(f)
    assert total == math.fsum(phi.astype(np.float64).ravel().tolist())
    assert lo == phi[obst == 0].min() and hi == phi[obst == 0].max() and hi < phi.max()      # (0, 5) holds 2
    _, lo, hi = lio.scalar_stats(f, np.ones((6, 9), np.uint8))
    assert lo == np.inf and hi == -np.inf
