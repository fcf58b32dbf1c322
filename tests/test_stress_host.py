"""Host side of the non-equilibrium strain rate (include/lbm_stress_hip.h; CPU only).

* The header declares exactly native.EXPORTED_STRESS, all exported by the
  library and disjoint from the other headers' lists; the ABI version stays 5;
  the enum values are the positions in STRESS_FIELDS / STRESS_FIELDS3D.
* Every entry point answers a NULL handle with LBM_E_INVALID.
* The numpy restatement the GPU tests compare against (lio.neq_strain /
  neq_strain3d / near_wall / strain_stats) is pinned by arithmetic, not against
  itself: populations built in fp64 from a chosen density, velocity and strain
  rate (equilibrium plus the first-order Chapman-Enskog non-equilibrium part,
  scaled by 1 - omega as the stored post-collision lattice carries it) must
  give that strain rate back within 2^-20 |coef| -- the rounding of sums of at
  most ten terms of size <= rho / 3, divided by rho, with a factor 2 over the
  derived 2^-21.  That pins the sign, the factor and the (1 - omega).  The
  expression order is pinned by the x <-> y swap and the periodic wrap of
  near_wall by hand-written maps, bit for bit.
* On the oracle's D3Q19 Poiseuille lattice s_xy equals the analytic 1/2 du/dy
  at every fluid cell, the wall-adjacent ones included, where the finite
  difference of lio.velocity_gradients3d is more than a quarter low.
* lbm_runner --device cpu --stress (lbmhost::neqStrain, a second
  implementation) writes what the restatement derives from the same run's cells.
"""
from __future__ import annotations

import math
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG, ROOT
from lbm_amd import io as lio
from lbm_amd import native
from oracle import oracle

EXE = PKG / "build" / "lbm_runner"
F2 = ("sxx", "sxy", "syy", "strain")
F3 = ("sxx", "syy", "szz", "sxy", "sxz", "syz", "strain")
OMEGAS = (0.6, 0.8, 1.25, 1.7, 1.85, 1.95)
W2 = np.array([4 / 9] + [1 / 9] * 4 + [1 / 36] * 4)
W3 = np.array([(1 / 3, 1 / 18, 1 / 36)[sum(c * c for c in e)] for e in lio.E3])   # by |e|^2: the order mixes them


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _coef(omega):
    omega = np.float32(omega)
    return float((np.float32(-1.5) * omega) / (np.float32(1) - omega))


# --------------------------------------------------------------- exports ----

def test_library_exports_every_stress_symbol():
    text = (ROOT / "include" / "lbm_stress_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 6 and sorted(native.EXPORTED_STRESS) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    assert L.lbm_abi_version() == 5
    others = (set(native.EXPORTED) | set(native.EXPORTED3D) | set(native.EXPORTED3D_FIELDS)
              | set(native.EXPORTED_FORCES) | set(native.EXPORTED_AVERAGES) | set(native.EXPORTED_GRADIENTS))
    assert not set(syms) & others


def test_field_name_lists_follow_the_header_enums():
    text = (ROOT / "include" / "lbm_stress_hip.h").read_text()
    assert native.STRESS_FIELDS == F2 and native.STRESS_FIELDS3D == F3
    for prefix, names in (("LBM_STRESS_", native.STRESS_FIELDS), ("LBM3D_STRESS_", native.STRESS_FIELDS3D)):
        for i, n in enumerate(names):
            assert re.search(rf"\b{prefix}{n.upper()} = {i}\b", text), (prefix, n)
        assert re.search(rf"\b{prefix}FIELDS = {len(names)}\b", text)
    # the work units the GPU tests place their sizes around
    hpp = (PKG / "csrc" / "lbm_stress.hpp").read_text()
    num = {k: int(v) for k, v in re.findall(r"\b(ST_BLOCK|ST_ITER|S3X|S3Y|S3Z) = (\d+)", hpp)}
    assert native.STRESS_QUAD == 4
    assert native.STRESS_BLOCK_QUADS == num["ST_BLOCK"] * num["ST_ITER"]
    assert native.STRESS3D_BLOCK == (4 * num["S3X"], num["S3Y"], num["S3Z"])


def test_null_handle_is_invalid():
    L = native.load_library()
    assert L.lbm_store_stress(None, None) == native.LBM_E_INVALID
    assert L.lbm_store_stress_local(None, None) == native.LBM_E_INVALID
    assert L.lbm_stress_stats(None, None, None, None, None, None) == native.LBM_E_INVALID
    assert L.lbm3d_store_stress(None, None) == native.LBM_E_INVALID
    assert L.lbm3d_store_stress_box(None, None, None) == native.LBM_E_INVALID
    assert L.lbm3d_stress_stats(None, None, None, None, None, None) == native.LBM_E_INVALID


# ------------------------------------------- constructed populations ----

def _constructed(e, w, rho, u, S, omega):
    """fp64 populations [n][q]: f_eq(rho, u) + (1 - omega) (-3 w rho / omega) (e e - I / 3) : S."""
    e = np.asarray(e, np.float64)                            # [q][d]
    d = e.shape[1]
    eu = u @ e.T                                             # [n][q]
    uu = (u * u).sum(-1)[:, None]
    feq = w[None, :] * rho[:, None] * (1 + 3 * eu + 4.5 * eu * eu - 1.5 * uu)
    qt = e[:, :, None] * e[:, None, :] - np.eye(d)[None] / 3  # [q][d][d]
    qs = np.einsum("qab,nab->nq", qt, S)
    return feq + (1 - omega) * (-3 * w[None, :] * rho[:, None] / omega) * qs


def _cases(d, n, seed):
    rng = np.random.default_rng(seed)
    rho = rng.choice([0.1, 1.0, 2.5], n)
    u = rng.uniform(-1, 1, (n, d))
    u *= (0.1 * rng.random(n) / np.sqrt((u * u).sum(-1)))[:, None]     # |u| <= 0.1
    S = rng.uniform(-1e-2, 1e-2, (n, d, d))
    S = np.triu(S) + np.triu(S, 1).transpose(0, 2, 1)                  # symmetric, |S_ab| <= 1e-2
    return rho, u, S


@pytest.mark.parametrize("omega", OMEGAS)
def test_constructed_populations_give_their_strain_rate_2d(omega):
    n = 700
    rho, u, S = _cases(2, n, int(omega * 100))
    om = float(np.float32(omega))
    cells = _constructed(lio.E2, W2, rho, u, S, om).astype(np.float32).reshape(1, n, 9)
    g = lio.neq_strain(cells, np.zeros((1, n), np.uint8), omega)
    assert all(g[k].dtype == np.float32 and g[k].shape == (1, n) for k in F2 + ("s2",))
    bound = 2.0 ** -20 * abs(_coef(omega))
    worst = 0.0
    for name, (a, b) in (("sxx", (0, 0)), ("syy", (1, 1)), ("sxy", (0, 1))):
        err = np.abs(g[name][0].astype(np.float64) - S[:, a, b]).max()
        worst = max(worst, err)
        assert err <= bound, (name, err, bound)
    print(f"omega {omega}: worst {worst / abs(_coef(omega)):.3e} |coef| (bound {2.0 ** -20:.3e})")
    s2 = (g["sxx"] * g["sxx"] + g["syy"] * g["syy"]) + (g["sxy"] * g["sxy"]) * np.float32(2)
    assert np.array_equal(_b32(g["s2"]), _b32(s2))
    assert np.array_equal(_b32(g["strain"]), _b32(np.sqrt(g["s2"], dtype=np.float32)))


@pytest.mark.parametrize("omega", OMEGAS)
def test_constructed_populations_give_their_strain_rate_3d(omega):
    n = 700
    rho, u, S = _cases(3, n, 1000 + int(omega * 100))
    om = float(np.float32(omega))
    cells = _constructed(lio.E3, W3, rho, u, S, om).astype(np.float32).reshape(1, 1, n, 19)
    g = lio.neq_strain3d(cells, np.zeros((1, 1, n), np.uint8), omega)
    assert all(g[k].dtype == np.float32 and g[k].shape == (1, 1, n) for k in F3 + ("s2",))
    bound = 2.0 ** -20 * abs(_coef(omega))
    for name, (a, b) in (("sxx", (0, 0)), ("syy", (1, 1)), ("szz", (2, 2)), ("sxy", (0, 1)), ("sxz", (0, 2)),
                         ("syz", (1, 2))):
        err = np.abs(g[name][0, 0].astype(np.float64) - S[:, a, b]).max()
        assert err <= bound, (name, err, bound)
    diag = (g["sxx"] * g["sxx"] + g["syy"] * g["syy"]) + g["szz"] * g["szz"]
    off = (g["sxy"] * g["sxy"] + g["sxz"] * g["sxz"]) + g["syz"] * g["syz"]
    assert np.array_equal(_b32(g["s2"]), _b32(diag + off * np.float32(2)))


@pytest.mark.parametrize("omega", OMEGAS)
def test_equilibrium_lattice_has_no_strain(omega):
    n = 500
    bound = 2.0 ** -20 * abs(_coef(omega))
    rho, u, S = _cases(2, n, 7)
    g = lio.neq_strain(_constructed(lio.E2, W2, rho, u, 0 * S, 1.5).astype(np.float32).reshape(1, n, 9),
                       np.zeros((1, n), np.uint8), omega)
    assert max(np.abs(g[k]).max() for k in ("sxx", "sxy", "syy")) <= bound
    rho, u, S = _cases(3, n, 8)
    g = lio.neq_strain3d(_constructed(lio.E3, W3, rho, u, 0 * S, 1.5).astype(np.float32).reshape(1, 1, n, 19),
                         np.zeros((1, 1, n), np.uint8), omega)
    assert max(np.abs(g[k]).max() for k in F3[:6]) <= bound


def test_omega_one_is_refused():
    with pytest.raises(ValueError, match="omega"):
        lio.neq_strain(np.ones((2, 2, 9), np.float32), np.zeros((2, 2), np.uint8), 1.0)


# ------------------------------------------------------- symmetries ----

def _random2(seed, ny=9, nx=11):
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, 0, 1, 0.1, 0.0, 1.85)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    return cells, (rng.random((ny, nx)) < 0.15).astype(np.uint8)


def _random3(seed, nz=5, ny=6, nx=7):
    rng = np.random.default_rng(seed)
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.0, 1.85)
    cells = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    return cells, (rng.random((nz, ny, nx)) < 0.15).astype(np.uint8)


def test_obstacle_cells_are_plus_zero():
    cells, ob = _random2(1)
    g = lio.neq_strain(cells, ob, 1.85)
    assert ob.any() and g["strain"][ob == 0].min() > 0
    for k in F2 + ("s2",):
        assert not _b32(g[k])[ob != 0].any(), k
    cells, ob = _random3(2)
    g = lio.neq_strain3d(cells, ob, 1.85)
    for k in F3 + ("s2",):
        assert not _b32(g[k])[ob != 0].any(), k


def test_axis_swap_symmetry_2d():
    """Speeds 1 <-> 2, 3 <-> 4, 6 <-> 8 swap x and y: sxx and syy change places and sxy
    stays.  Bit for bit where no sum rounds -- populations that are multiples of 2^-12
    with density exactly 1, so that rho, the moments and rho * u are exact and only
    commutative products differ; the swap reorders the sequential sums of rho, pxx and pyy,
    so general populations agree to the rounding bound of the construction tests."""
    swap = [0, 2, 1, 4, 3, 5, 8, 7, 6]
    rng = np.random.default_rng(3)
    n = rng.integers(100, 400, (9, 11, 9))
    n[..., 0] += 4096 - n.sum(-1)
    cells = (n / 4096).astype(np.float32)
    assert (cells.astype(np.float64).sum(-1) == 1).all() and (cells > 0).all()
    ob = (rng.random((9, 11)) < 0.15).astype(np.uint8)
    g = lio.neq_strain(cells, ob, 1.85)
    s = lio.neq_strain(np.ascontiguousarray(cells[..., swap]), ob, 1.85)
    assert np.abs(g["sxy"]).max() > 0 and not np.array_equal(g["sxx"], g["syy"])
    assert np.array_equal(_b32(s["sxy"]), _b32(g["sxy"]))
    assert np.array_equal(_b32(s["sxx"]), _b32(g["syy"])) and np.array_equal(_b32(s["syy"]), _b32(g["sxx"]))
    assert np.array_equal(_b32(s["strain"]), _b32(g["strain"]))
    cells, ob = _random2(3)
    g = lio.neq_strain(cells, ob, 1.85)
    s = lio.neq_strain(np.ascontiguousarray(cells[..., swap]), ob, 1.85)
    bound = 2.0 ** -20 * abs(_coef(1.85))
    for a, b in (("sxy", "sxy"), ("sxx", "syy"), ("syy", "sxx")):
        assert np.abs(s[a].astype(np.float64) - g[b]).max() <= bound, (a, b)


@pytest.mark.parametrize("shift", [(1, 0), (0, 1), (-3, 4)])
def test_roll_equivariance(shift):
    cells, ob = _random2(4)
    g = lio.neq_strain(cells, ob, 1.85)
    r = lio.neq_strain(np.roll(cells, shift, (0, 1)), np.roll(ob, shift, (0, 1)), 1.85)
    for k in F2 + ("s2",):
        assert np.array_equal(_b32(r[k]), _b32(np.roll(g[k], shift, (0, 1)))), k
    assert np.array_equal(lio.near_wall(np.roll(ob, shift, (0, 1))), np.roll(lio.near_wall(ob), shift, (0, 1)))
    cells, ob = _random3(5)
    sh = shift + (2,)
    g = lio.neq_strain3d(cells, ob, 1.85)
    r = lio.neq_strain3d(np.roll(cells, sh, (0, 1, 2)), np.roll(ob, sh, (0, 1, 2)), 1.85)
    for k in F3 + ("s2",):
        assert np.array_equal(_b32(r[k]), _b32(np.roll(g[k], sh, (0, 1, 2)))), k
    assert np.array_equal(lio.near_wall3d(np.roll(ob, sh, (0, 1, 2))), np.roll(lio.near_wall3d(ob), sh, (0, 1, 2)))


def test_near_wall_by_hand():
    ob = np.zeros((5, 5), np.uint8)
    ob[0, 0] = 1          # a corner: its 8 neighbours wrap to rows 4, 1 and columns 4, 1
    ob[2, 3] = 1
    want = np.array([[0, 1, 0, 0, 1],
                     [1, 1, 1, 1, 1],
                     [0, 0, 1, 0, 1],
                     [0, 0, 1, 1, 1],
                     [1, 1, 0, 0, 1]], bool)
    assert np.array_equal(lio.near_wall(ob), want)
    assert not lio.near_wall(np.zeros((3, 4), np.uint8)).any()
    assert not lio.near_wall(np.ones((3, 4), np.uint8)).any()
    ob3 = np.zeros((3, 3, 3), np.uint8)
    ob3[0, 0, 0] = 1      # with extent 3 every other cell is a periodic neighbour: only the 8 corner
    want3 = np.ones((3, 3, 3), bool)      # offsets (+-1, +-1, +-1) are not lattice neighbours
    want3[0, 0, 0] = False
    for z in (1, 2):
        for y in (1, 2):
            for x in (1, 2):
                want3[z, y, x] = False
    assert np.array_equal(lio.near_wall3d(ob3), want3)


def test_strain_stats_restatement():
    cells, ob = _random2(6)
    g = lio.neq_strain(cells, ob, 1.85)
    near = lio.near_wall(ob)
    s2, ms, nw, sw, mw = lio.strain_stats(g, ob, near)
    fluid = ob == 0
    assert s2 == math.fsum(g["s2"][fluid].astype(np.float64).tolist())
    assert ms == g["strain"].max() and isinstance(ms, np.float32)
    assert nw == int(near.sum()) and 0 < nw < fluid.sum()
    assert sw == math.fsum(g["strain"][near].astype(np.float64).tolist())
    assert mw == g["strain"][near].max() and isinstance(mw, np.float32)
    none = np.zeros_like(ob)
    assert lio.strain_stats(g, none, lio.near_wall(none))[2:] == (0, 0.0, 0)


# ------------------------------------------------- physics: Poiseuille ----

NXP, NYP, NZP = 4, 18, 4


@pytest.fixture(scope="module", params=[(1.25, 1.0, 1e-5), (1.7, 0.1, 1e-4)], ids=["w1.25", "w1.7"])
def poiseuille(request):
    omega, density, accel = request.param
    p = lio.Params3D(NXP, NYP, NZP, 0, density, accel, omega)
    obst = lio.channel_obstacles3d(NXP, NYP, NZP)
    cells, _ = oracle.run3d(p, obst, 12000)
    return p, obst, cells


def poiseuille_sxy(p):
    """The analytic 1/2 du_x/dy at the cell centres y = 0 .. ny-1 of the channel."""
    nu = (1 / float(np.float32(p.omega)) - 0.5) / 3
    return 0.5 * (float(np.float32(p.accel)) / 3) / (2 * nu) * (p.ny - 1 - 2 * np.arange(p.ny))


def test_poiseuille_wall_accurate_strain(poiseuille):
    """s_xy of the oracle's steady channel against the analytic 1/2 du_x/dy, relative to
    its value at the wall-adjacent cell.  Measured deviation: 1.3e-3 (omega 1.25) and
    4.3e-5 (omega 1.7); the finite difference of lio.velocity_gradients3d at the
    wall-adjacent cell is 28 % low (9.04e-5 against 1.25e-4; 3.05e-3 against 4.25e-3).
    The other components vanish in the channel: asserted below 1e-4 absolute (the scale
    of the smaller wall value, 1.25e-4; 2^-21 |coef| = 3.6e-6 is the rounding floor
    there).  Measured maximum: 4.5e-7 at omega 1.25, 7.9e-6 at omega 1.7."""
    p, obst, cells = poiseuille
    g = lio.neq_strain3d(cells, obst, p.omega)
    ana = poiseuille_sxy(p)
    wall = ana[1]
    fluid = slice(1, NYP - 1)
    dev = np.abs(g["sxy"][:, fluid, :].astype(np.float64) - ana[None, fluid, None]).max() / wall
    others = max(np.abs(g[k][:, fluid, :]).max() for k in ("sxx", "syy", "szz", "sxz", "syz"))
    print(f"omega {p.omega}: sxy deviation {dev:.3e}, wall cell {g['sxy'][0, 1, 0]:.4e} (analytic {wall:.4e}), "
          f"other components {others:.3e}")
    assert dev < 1e-2
    assert others < 1e-4
    ux, uy, uz, _, _ = lio.macroscopic3d(p, obst, cells)
    fd = lio.velocity_gradients3d(ux, uy, uz, obst)
    # gxy alone (gyx = 0 in the channel): strain = sqrt(2 sxy^2), sxy = gxy / 2
    fd_sxy = fd["strain"][:, 1, :].astype(np.float64) / math.sqrt(2)
    assert (np.abs(fd_sxy - wall) / wall > 0.2).all()
    assert np.abs(g["sxy"][:, 1, :] - wall).max() / wall < 1e-2


# ---------------------------------------------------------------- runner ----

def test_cpu_runner_writes_stress_state(tmp_path):
    """The golden 128 x 128 problem, 50 steps, on the host backend: stress_state.dat
    (lbmhost::neqStrain of the stored cells) parsed back equals the restatement over the
    same run's cells -- the oracle's, whose final_state.dat the run reproduces byte for
    byte.  %.12E is exact for fp32."""
    steps = 50
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = str(steps)
    params = tmp_path / "short.params"
    params.write_text("\n".join(lines))
    p = lio.Params.from_file(str(params))
    assert p.max_iters == steps
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    r = subprocess.run([str(EXE), "--device", "cpu", "--stress", "--params", str(params), "--obstacles",
                        str(obst_file), "--runs", "0", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    cells, _ = oracle.run(p, obst, steps, lio.init_cells(p))
    lio.write_results(str(tmp_path / "ref_final_state.dat"), p, obst, cells)
    assert (tmp_path / "final_state.dat").read_bytes() == (tmp_path / "ref_final_state.dat").read_bytes()
    got = lio.read_stress_state(str(tmp_path / "stress_state.dat"), p.nx, p.ny)
    ob = np.asarray(obst).reshape(p.ny, p.nx)
    assert np.array_equal(got["obstacle"], (ob != 0).astype(np.uint8))
    assert np.array_equal(got["near_wall"], lio.near_wall(ob).astype(np.uint8)) and got["near_wall"].any()
    want = lio.neq_strain(cells.reshape(p.ny, p.nx, 9), ob, p.omega)
    for k in F2:
        assert np.array_equal(_b32(got[k]), _b32(want[k])), k
    assert want["strain"].max() > 0
