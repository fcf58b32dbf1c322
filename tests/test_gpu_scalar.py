"""The passive scalar on the device, D2Q9 + D2Q5 (lbm_scalar_*;
include/lbm_scalar_hip.h, csrc/lbm_scalar.hip, csrc/lbm_scalar.hpp).

Bar: after every scalar_advance the populations and phi are BITWISE (uint32
patterns) lio.scalar_step applied to the same handle's fields() at that moment
(and lio.scalar_apply_fixed after every step) -- the numpy restatement of the
header's definition, pinned by physics in tests/test_scalar_host.py -- for
every step kernel of the flow, both numerics, both sides of the flow pair,
advance(1 | 2 | 3), decomposed handles (whose bits are the single-domain
handle's) and degenerate shapes.  The statistics' extremes are exact and the
sum lies within the fold bound DESIGN 4.14 states for fp64 sums,
2 (n - 1) 2^-53 sum|phi|, of the exact sum.  No other tolerance anywhere.
"""
from __future__ import annotations

import ctypes
import math
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)      # flow steps before each advance: both lattices of the pair get read
ADVANCES = (1, 2, 3, 1, 2)    # scalar steps of each advance
GRIDS = [(37, 19), (64, 32)]
OMEGA_S = 1.3


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_b32(a), _b32(b))


def _problem(nx, ny, seed, iters=8, obstacles=0.1):
    """About 10 % random obstacles on a 5 % perturbed equilibrium, and a random phi0 in [1, 2)."""
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx)) < obstacles).astype(np.uint8)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    phi0 = (1 + rng.random((ny, nx))).astype(np.float32)
    return p, obst, cells, phi0


def _fixed(p, obst, seed=3, n=9):
    """n distinct cells: corners, the cells next to the middle (the borders of the decompositions), an
    obstacle cell and a fluid cell among them."""
    rng = np.random.default_rng(seed)
    cells = {(0, 0), (p.nx - 1, p.ny - 1), (p.nx // 2, p.ny // 2), (max(p.nx // 2 - 1, 0), p.ny // 2)}
    ob, fl = np.argwhere(obst != 0), np.argwhere(obst == 0)
    if len(ob):
        cells.add((int(ob[0][1]), int(ob[0][0])))
    if len(fl):
        cells.add((int(fl[-1][1]), int(fl[-1][0])))
    while len(cells) < min(n, p.nx * p.ny):
        cells.add((int(rng.integers(p.nx)), int(rng.integers(p.ny))))
    x, y = np.array(sorted(cells), np.int32).T
    return x, y, (3 + rng.random(x.size)).astype(np.float32)


def _advance_and_check(e, obst, g, n, fixed=None, what=""):
    """One advance of n steps: the handle against n steps of the restatement over its fields()."""
    f = e.fields(("ux", "uy"))
    for _ in range(n):
        g = lio.scalar_step(g, f["ux"], f["uy"], obst, OMEGA_S)
        if fixed is not None:
            g = lio.scalar_apply_fixed(g, *fixed)
    before = e.scalar_steps
    e.scalar_advance(n)
    assert e.scalar_steps == before + n
    phi, got = e.scalar(populations=True)
    assert got.dtype == np.float32 and got.shape == g.shape
    bad = _b32(got) != _b32(g)
    assert not bad.any(), (what, n, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert _same(phi, lio.scalar_phi(g)) and _same(e.scalar(), phi), (what, n)
    return g


def _sequence(e, p, obst, cells0, phi0, fixed=None, what="", chunks=CHUNKS):
    e.load_cells(cells0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    g = lio.scalar_init(phi0)
    assert _same(e.scalar(populations=True)[1], g) and e.scalar_steps == 0
    if fixed is not None:
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed(g, *fixed)
        assert _same(e.scalar(populations=True)[1], g)
    for i, (steps, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(steps, accelerate_first=i == 0)
        g = _advance_and_check(e, obst, g, n, fixed, what)
    return g


# ------------------------------------------------------------ 1. parity ----

@pytest.mark.parametrize("with_fixed", [False, True])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_advance_sequences_bitwise(gpu_lib, nx, ny, with_fixed):
    p, obst, cells0, phi0 = _problem(nx, ny, 100 * nx + ny)
    fixed = _fixed(p, obst) if with_fixed else None
    with gpu_lib.Engine(p, obst) as e:
        g = _sequence(e, p, obst, cells0, phi0, fixed, (nx, ny, with_fixed))
    assert obst.any() and np.abs(lio.scalar_phi(g) - phi0).max() > 1e-3          # the scalar moved


@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_advance_every_kernel_bitwise(gpu_lib, mode):
    n = gpu_lib
    kw, want = {
        "auto": (dict(), ("resident", "step2")),
        "stream": (dict(kernel=n.KERNEL_STREAM), ("stream",)),
        "stream_tolerance": (dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE), ("stream",)),
        "step2": (dict(kernel=n.KERNEL_STEP2), ("step2",)),
        "scalar": (dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP), ("scalar",)),
        "pipeline": (dict(kernel=n.KERNEL_PIPELINE), ("pipeline",)),
    }[mode]
    p, obst, cells0, phi0 = _problem(132, 70, 7)
    with n.Engine(p, obst, **kw) as e:
        _sequence(e, p, obst, cells0, phi0, _fixed(p, obst), mode)
        assert e.kernel_in_use() in want
        assert e.numerics() == ("tolerance" if mode == "stream_tolerance" else "bitwise")


# ------------------------------------------------------ 2. decomposed ----

@pytest.fixture(scope="module")
def single(gpu_lib):
    """{grid: (p, obst, cells0, phi0, fixed, g)} of the single-domain handles after the sequence: the
    reference of the decomposed cases, computed once and left unchanged."""
    out = {}
    for nx, ny in GRIDS:
        p, obst, cells0, phi0 = _problem(nx, ny, 31 + nx)
        fixed = _fixed(p, obst)
        with gpu_lib.Engine(p, obst, parts=1) as e:
            assert len(e.local_rects()) == 1
            g = _sequence(e, p, obst, cells0, phi0, fixed, "single")
            stats = e.scalar_stats()
        for a in (obst, cells0, phi0, g) + fixed:
            a.setflags(write=False)
        out[(nx, ny)] = (p, obst, cells0, phi0, fixed, g, stats)
    return out


@pytest.mark.parametrize("grid", [(1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_bits_do_not_depend_on_the_decomposition(gpu_lib, single, nx, ny, grid):
    p, obst, cells0, phi0, fixed, ref, ref_stats = single[(nx, ny)]
    with gpu_lib.Engine(p, obst, parts=grid[0] * grid[1], grid=grid, devices=[0]) as e:
        rects = e.local_rects()
        assert len(rects) == grid[0] * grid[1]
        g = _sequence(e, p, obst, cells0, phi0, fixed, (nx, ny, grid))
        total, lo, hi = e.scalar_stats()
    assert _same(g, ref)
    if grid[1] == 2 and nx == 37:
        assert any(r[0] % 4 for r in rects)              # a sub-domain off the 16-B alignment
    assert (lo, hi) == ref_stats[1:] and abs(total - ref_stats[0]) <= _fold_bound(lio.scalar_phi(ref))


# ------------------------------------------------- 3. degenerate shapes ----

@pytest.mark.parametrize("nx,ny", [(1, 8), (8, 1), (1, 1), (2, 1), (4, 1), (5, 3), (8, 2)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny):
    p, obst, cells0, phi0 = _problem(nx, ny, 5 + nx + 10 * ny, obstacles=0.2 if nx * ny > 4 else 0.0)
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, _fixed(p, obst, n=2), (nx, ny))


def test_all_obstacle_grid(gpu_lib):
    p, _, cells0, phi0 = _problem(13, 6, 2)
    obst = np.ones((6, 13), np.uint8)
    with gpu_lib.Engine(p, obst) as e:
        g = _sequence(e, p, obst, cells0, phi0, None, "all obstacles", chunks=(1, 2))
        total, lo, hi = e.scalar_stats()
    assert lo == np.inf and hi == -np.inf
    assert abs(total - lio.scalar_stats(g, obst)[0]) <= _fold_bound(lio.scalar_phi(g))
    # every step reverses the populations in place: two steps are the identity on the moving ones
    g2 = lio.scalar_step(lio.scalar_step(g, phi0 * 0, phi0 * 0, obst, OMEGA_S), phi0 * 0, phi0 * 0, obst, OMEGA_S)
    assert _same(g2, g)


# -------------------------------------------------------- 4. fixed cells ----

def test_fixed_cells_fluid_and_obstacle(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 77)
    fy, fx = [int(v) for v in np.argwhere(obst == 0)[5]]
    oy, ox = [int(v) for v in np.argwhere(obst != 0)[2]]
    i32p, f32p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    with n.Engine(p, obst) as e:
        L, h = e._L, e._h
        e.load_cells(cells0)
        e.run_steps(3, accelerate_first=True)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        g = lio.scalar_init(phi0)
        fixed = (np.array([fx, ox], np.int32), np.array([fy, oy], np.int32), np.array([5.0, -2.0], np.float32))
        e.scalar_fix(*fixed)
        g = lio.scalar_apply_fixed(g, *fixed)
        assert _same(e.scalar(populations=True)[1], g)
        g = _advance_and_check(e, obst, g, 3, fixed, "fixed")
        phi = lio.scalar_phi(g)
        held = lio.scalar_phi(lio.scalar_init(fixed[2].reshape(1, 2)))[0]     # 5 / 3 + 4 (5 / 6) in fp32: 5 + 1 ulp
        assert phi[fy, fx] == held[0] and phi[oy, ox] == held[1] and abs(held[0] - 5) < 1e-6
        # refused lists: the old list stays
        P = lambda a, t: a.ctypes.data_as(t)
        val = np.array([1.0, 1.0], np.float32)
        for bx, by in (([0, p.nx], [0, 0]), ([0, 0], [0, p.ny]), ([-1, 0], [0, 0]), ([0, 1], [-1, 1]),
                       ([3, 3], [4, 4])):
            xb, yb = np.array(bx, np.int32), np.array(by, np.int32)
            assert L.lbm_scalar_set_fixed(h, 2, P(xb, i32p), P(yb, i32p), P(val, f32p)) == n.LBM_E_INVALID, (bx, by)
        assert b"twice" in L.lbm_last_error(h)
        assert L.lbm_scalar_set_fixed(h, -1, None, None, None) == n.LBM_E_INVALID
        assert L.lbm_scalar_set_fixed(h, 1, None, P(yb, i32p), P(val, f32p)) == n.LBM_E_INVALID
        assert _same(e.scalar(populations=True)[1], g)
        g = _advance_and_check(e, obst, g, 1, fixed, "old list kept")
        # n = 0 clears the list; a fresh begin clears it too
        assert L.lbm_scalar_set_fixed(h, 0, None, None, None) == n.LBM_OK
        g = _advance_and_check(e, obst, g, 2, None, "cleared")
        e.scalar_fix(*fixed)
        e.scalar_begin(phi0, diffusivity=lio.scalar_diffusivity(np.float32(OMEGA_S)))
        g = _advance_and_check(e, obst, lio.scalar_init(phi0), 1, None, "begin clears")
        with pytest.raises(ValueError):
            e.scalar_fix(fixed[0], fixed[1], fixed[2][:1])
        with pytest.raises(ValueError):
            e.scalar_fix(fixed[0], fixed[1])


# -------------------------------------------------------------- 5. stats ----

def _fold_bound(phi):
    """a sum of n terms folded in fp64 lies within 2 (n - 1) 2^-53 sum|term| of the exact sum."""
    return 2.0 * (phi.size - 1) * 2.0 ** -53 * math.fsum(np.abs(phi.astype(np.float64)).ravel().tolist())


@pytest.mark.parametrize("nx,ny", GRIDS + [(300, 70)])
def test_stats_equal_the_restatement(gpu_lib, nx, ny):
    p, obst, cells0, phi0 = _problem(nx, ny, 9 * nx + ny)
    phi0 = (phi0 - np.float32(1.5)).astype(np.float32)           # both signs
    obst[np.unravel_index(np.argmax(phi0), phi0.shape)] = 1      # the extremes of all cells lie on obstacles
    obst[np.unravel_index(np.argmin(phi0), phi0.shape)] = 1
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        for steps in (0, 2):
            e.run_steps(steps)
            e.scalar_advance(steps)
            g = e.scalar(populations=True)[1]
            total, lo, hi = e.scalar_stats()
            want, wlo, whi = lio.scalar_stats(g, obst)
            phi = lio.scalar_phi(g)
            print(f"{nx}x{ny} after {steps}: total {total!r} exact {want!r} bound {_fold_bound(phi):.3e}")
            assert abs(total - want) <= _fold_bound(phi)
            assert np.float32(lo) == wlo and np.float32(hi) == whi
            if steps == 0:
                assert lo > phi.min() and hi < phi.max()
            again = e.scalar_stats()
            assert np.array_equal(np.array(again[:1]).view(np.uint64), np.array([total]).view(np.uint64))
            assert again[1:] == (lo, hi)


# -------------------------------------------- 6. no engine state touched ----

def test_scalar_touches_no_engine_state(gpu_lib):
    p, obst, cells0, phi0 = _problem(64, 32, 21, iters=13)
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        e.scalar_fix(*_fixed(p, obst))
        e.run_steps(7, accelerate_first=True)
        av7 = e.store(cells=False, n_av=7)[1].copy()
        e.scalar_advance(3)
        e.scalar(populations=True)
        e.scalar_stats()
        e.run_steps(6)
        cells_a, av6 = e.store(n_av=6)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        cells, av = e.store(n_av=13)
    assert np.array_equal(_b32(cells_a), _b32(cells)) and np.array_equal(_b32(np.concatenate([av7, av6])), _b32(av))


# ------------------------------------ 7. run_scalar / scalar_history ----

def test_run_scalar_and_history(gpu_lib):
    p, obst, cells0, phi0 = _problem(64, 32, 3, iters=13)
    with gpu_lib.Engine(p, obst) as e:                      # by hand: stride 1 and stride 5
        refs = {}
        for stride in (1, 5):
            e.load_cells(cells0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            g, done = lio.scalar_init(phi0), 0
            while done < 13:
                n = min(stride, 13 - done)
                e.run_steps(n, accelerate_first=done == 0)
                g = _advance_and_check(e, obst, g, n, None, ("by hand", stride))
                done += n
            refs[stride] = (g, e.store(n_av=0)[0])
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        cells13, av13 = e.store(n_av=13)
    assert np.array_equal(_b32(refs[1][1]), _b32(cells13)) and not _same(refs[1][0], refs[5][0])
    for stride in (1, 5):
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            av = e.run_scalar(13, stride, accelerate_first=True)
            assert e.scalar_steps == 13
            assert _same(e.scalar(populations=True)[1], refs[stride][0])
            assert np.array_equal(_b32(e.store(n_av=0)[0]), _b32(cells13)) and np.array_equal(_b32(av), _b32(av13))
            with pytest.raises(ValueError):
                e.run_scalar(5, 0)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        hist = e.scalar_history(13, 5, accelerate_first=True)
        assert [s[0] for s in hist] == [5, 10, 13] and hist[-1][1:] == e.scalar_stats()
        assert _same(e.scalar(populations=True)[1], refs[1][0])
        assert all(len(s) == 4 and s[2] <= s[3] for s in hist)


# ---------------------------------------------------------- 8. contract ----

def test_scalar_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 9)
    f32p = ctypes.POINTER(ctypes.c_float)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        L, h = e._L, e._h
        phi = np.full((p.ny, p.nx), 7, np.float32)
        cnt = ctypes.c_int64(-1)
        tot = ctypes.c_double(-1)
        # before begin
        assert L.lbm_scalar_advance(h, 1) == n.LBM_E_STATE
        assert L.lbm_scalar_steps(h, ctypes.byref(cnt)) == n.LBM_E_STATE
        assert L.lbm_scalar_steps(h, None) == n.LBM_E_INVALID
        assert L.lbm_scalar_store(h, phi.ctypes.data_as(f32p), None) == n.LBM_E_STATE
        assert L.lbm_scalar_stats(h, ctypes.byref(tot), None, None) == n.LBM_E_STATE
        assert L.lbm_scalar_set_fixed(h, 0, None, None, None) == n.LBM_E_STATE
        assert L.lbm_scalar_end(h) == n.LBM_OK
        assert (phi == 7).all() and cnt.value == -1 and tot.value == -1
        # omega_s
        for om in (0.0, 2.0, -0.5, 2.5, float("nan"), float("inf")):
            assert L.lbm_scalar_begin(h, om, None) == n.LBM_E_INVALID, om
        assert L.lbm_scalar_steps(h, ctypes.byref(cnt)) == n.LBM_E_STATE
        with pytest.raises(ValueError):
            e.scalar_begin(phi0)
        with pytest.raises(ValueError):
            e.scalar_begin(phi0, omega_s=1.0, diffusivity=0.1)
        with pytest.raises(ValueError):
            e.scalar_begin(phi0[:-1], omega_s=1.0)
        # begun, no lattice yet: everything but advance works; NULL phi0 is zeros
        e.scalar_begin(None, omega_s=OMEGA_S)
        assert L.lbm_scalar_advance(h, 1) == n.LBM_E_STATE and L.lbm_scalar_advance(h, -1) == n.LBM_E_INVALID
        ph, g = e.scalar(populations=True)
        assert not _b32(ph).any() and not _b32(g).any() and e.scalar_stats() == (0.0, 0.0, 0.0)
        e.load_cells(cells0)
        e.run_steps(3, accelerate_first=True)
        e.scalar_begin(phi0, omega_s=OMEGA_S)                  # a second begin replaces the state
        # steps: negative refused, zero launches nothing
        launches = lambda: sum(k["launches"] for k in e.profile_summary())
        before = launches()
        assert L.lbm_scalar_advance(h, -1) == n.LBM_E_INVALID
        assert L.lbm_scalar_advance(h, 0) == n.LBM_OK and launches() == before and e.scalar_steps == 0
        assert L.lbm_scalar_store(h, None, None) == n.LBM_OK
        assert L.lbm_scalar_stats(h, None, None, None) == n.LBM_OK and launches() == before
        # a refused begin keeps the state
        g = _advance_and_check(e, obst, lio.scalar_init(phi0), 2, None, "contract")
        assert L.lbm_scalar_begin(h, 2.0, None) == n.LBM_E_INVALID
        assert e.scalar_steps == 2 and _same(e.scalar(populations=True)[1], g)
        # profile classes
        e.scalar_fix(*_fixed(p, obst))
        e.scalar_advance(2)
        e.scalar_stats()
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["scalar_step"]["launches"] == 4 and prof["scalar_fixed"]["launches"] == 3
        assert prof["scalar_stats"]["launches"] == 2 and prof["scalar_step"]["total_ms"] > 0
        # end
        e.scalar_end()
        assert L.lbm_scalar_advance(h, 1) == n.LBM_E_STATE and L.lbm_scalar_end(h) == n.LBM_OK
        e.scalar_begin(phi0, omega_s=OMEGA_S)     # the handle is destroyed with a scalar: lbm_destroy frees it
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:       # a handle that never begins launches nothing
        e.load_cells(cells0)
        e.run_steps(4, accelerate_first=True)
        assert not [k for k in e.profile_summary() if "scalar_" in k["name"]]


def test_restrictions_are_refused_with_a_message(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(64, 64, 4)
    with n.Engine(p, obst, parts=18, grid=(3, 6), devices=[0]) as e:
        assert len(e.local_rects()) == 18 > n.SCALAR_MAX_PARTS
        with pytest.raises(n.LbmError, match="more than 16 local sub-domains") as err:
            e.scalar_begin(phi0, omega_s=1.0)
        assert err.value.code == n.LBM_E_INVALID
        assert e._L.lbm_scalar_advance(e._h, 1) == n.LBM_E_STATE
    with n.Engine(p, obst, parts=16, devices=[0]) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=1.0)
        e.scalar_advance(1)
        assert e.scalar_steps == 1


# ------------------------------------------------------------ 9. runner ----

def test_runner_scalar_option(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    help_text = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--scalar" in help_text.stdout + help_text.stderr
    assert "--scalar-omega" in help_text.stdout + help_text.stderr
    assert "--scalar-stride" in help_text.stdout + help_text.stderr
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "23"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    # a blob of dye, one fixed inlet cell, the rest 0
    src = [(10, 64, 2.0, 1), (40, 40, 1.0, 0), (41, 40, 0.5, 0), (127, 127, 0.25, 0)]
    (tmp_path / "dye.txt").write_text("".join(f"{x} {y} {v!r}" + (" 1\n" if f else "\n") for x, y, v, f in src))
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file), "--scalar",
            str(tmp_path / "dye.txt"), "--scalar-omega", "1.3"]
    out = {}
    for stride in (1, 4):
        d = tmp_path / f"s{stride}"
        d.mkdir()
        r = subprocess.run(base + ["--scalar-stride", str(stride), "--out-dir", str(d)], capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
        text = (d / "scalar_state.dat").read_text().splitlines()
        assert len(text) == p.nx * p.ny and text[0].split()[:2] == ["0", "0"] and text[1].split()[:2] == ["1", "0"]
        assert all(len(t.split()) == 3 for t in text[:300])
        out[stride] = lio.read_scalar_state(str(d / "scalar_state.dat"), p.nx, p.ny)
    # the same coupled run through the binding
    phi0 = np.zeros((p.ny, p.nx), np.float32)
    for x, y, v, _ in src:
        phi0[y, x] = v
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(lio.init_cells(p))
        e.scalar_begin(phi0, omega_s=1.3)
        e.scalar_fix(np.array([10]), np.array([64]), np.array([2.0], np.float32))
        e.run_scalar(23, 1, accelerate_first=True)
        phi = e.scalar()
    assert _same(out[1], phi) and not _same(out[4], phi)
    assert phi[64, 10] == lio.scalar_phi(lio.scalar_init(np.full((1, 1), 2, np.float32)))[0, 0]
    r = subprocess.run(base + ["--device", "cpu", "--out-dir", str(tmp_path)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--scalar" in r.stderr
