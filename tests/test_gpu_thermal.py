"""Boussinesq buoyancy on the device, D2Q9 (lbm_scalar_buoyancy; include/lbm_thermal_hip.h,
csrc/lbm_scalar.hip, csrc/lbm_scalar.hpp).

Bar: after every scalar_buoyancy the stored lattice is BITWISE (uint32 patterns) lio.buoyancy_kick
of what the same handle stored just before -- the numpy restatement of the header's definition,
pinned by physics in tests/test_thermal_host.py -- on both sides of the flow pair, for every step
kernel, both numerics and decomposed handles; a run afterwards continues bit for bit, av_vels
included, as a second handle does that loaded the kicked cells (the ghost rebuild); run_thermal is
its definition and, at stride 1 on the default kernel, the CPU loop (oracle step + lio) bit for bit;
the Rayleigh-Benard roll decays at Ra = 1400 and grows at Ra = 2200 on the device as it does on the
CPU (tests/test_thermal_host.py states the measured ratios).  No tolerance anywhere.
"""
from __future__ import annotations

import subprocess

import numpy as np
import pytest

import thermal_cases as tc
from conftest import GOLD, PKG
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)      # flow steps before each kick: both lattices of the pair get kicked
ADVANCES = (1, 2, 3, 1, 2)    # scalar steps before each kick
GRIDS = [(37, 19), (64, 32)]
OMEGA_S = 1.3
IMPULSES = [(0.004, -0.003), (0.0, 0.005)]
PHI_REF = 1.4
MODES = ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"]

_b32, _same = tc.b32, tc.same


def _mode(n, mode):
    return {
        "auto": (dict(), ("resident", "step2")),
        "stream": (dict(kernel=n.KERNEL_STREAM), ("stream",)),
        "stream_tolerance": (dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE), ("stream",)),
        "step2": (dict(kernel=n.KERNEL_STEP2), ("step2",)),
        "scalar": (dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP), ("scalar",)),
        "pipeline": (dict(kernel=n.KERNEL_PIPELINE), ("pipeline",)),
    }[mode]


def _problem(nx, ny, seed, iters=8, obstacles=0.1):
    """About 10 % random obstacles on a 5 % perturbed equilibrium, and a random phi0 in [1, 2)."""
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx)) < obstacles).astype(np.uint8)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    phi0 = (1 + rng.random((ny, nx))).astype(np.float32)
    return p, obst, cells, phi0


def _fixed(p, obst, n=5, seed=3):
    rng = np.random.default_rng(seed)
    cells = {(0, 0), (p.nx - 1, p.ny - 1), (p.nx // 2, p.ny // 2)}
    while len(cells) < min(n, p.nx * p.ny):
        cells.add((int(rng.integers(p.nx)), int(rng.integers(p.ny))))
    x, y = np.array(sorted(cells), np.int32).T
    return x, y, (3 + rng.random(x.size)).astype(np.float32)


def _kick_and_check(e, p, obst, s, what=""):
    """One kick: the handle's store() against the restatement of what it stored just before; the scalar
    is untouched.  Returns the kicked cells."""
    before = e.store(n_av=0)[0]
    phi, g = e.scalar(populations=True)
    steps = e.scalar_steps
    e.scalar_buoyancy(s, PHI_REF)
    got = e.store(n_av=0)[0]
    want = lio.buoyancy_kick(before, g, obst, p.density, s, PHI_REF)
    bad = _b32(got) != _b32(want)
    assert not bad.any(), (what, s, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert _same(got[obst != 0], before[obst != 0]) and (obst.all() or not _same(got, before)), what
    phi2, g2 = e.scalar(populations=True)
    assert _same(g2, g) and _same(phi2, phi) and e.scalar_steps == steps, what
    return got


def _sequence(e, p, obst, cells0, phi0, s, what="", chunks=CHUNKS):
    e.load_cells(cells0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    fixed = _fixed(p, obst)
    e.scalar_fix(*fixed)
    cells = None
    for i, (c, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(c, accelerate_first=i == 0)
        e.scalar_advance(n)
        cells = _kick_and_check(e, p, obst, s, (what, i))
        held = lio.scalar_phi(lio.scalar_init(fixed[2].reshape(1, -1)))[0]
        assert _same(e.scalar()[fixed[1], fixed[0]], held)
    return cells


# ------------------------------------------------------- 5. kick, bitwise ----

@pytest.mark.parametrize("s", IMPULSES)
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_kick_sequences_bitwise(gpu_lib, nx, ny, s):
    p, obst, cells0, phi0 = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, s, (nx, ny, s))
    assert obst.any()


@pytest.mark.parametrize("mode", MODES)
def test_kick_every_kernel_bitwise(gpu_lib, mode):
    kw, want = _mode(gpu_lib, mode)
    p, obst, cells0, phi0 = _problem(132, 70, 7)
    with gpu_lib.Engine(p, obst, **kw) as e:
        for s in IMPULSES:
            _sequence(e, p, obst, cells0, phi0, s, (mode, s))
        assert e.kernel_in_use() in want
        assert e.numerics() == ("tolerance" if mode == "stream_tolerance" else "bitwise")


# ------------------------------------------------ 6. continuation, bitwise ----

def _continuation(n, p, obst, cells0, phi0, kw, what):
    """Kick, then run k steps -- on the kicked handle and on a second one that loaded the kicked cells --
    for k = 1, 2, 5 and the fused depth + 1.  Returns the lattice after k = 5 (the depth is the handle's own)."""
    with n.Engine(p, obst, **kw) as a, n.Engine(p, obst, **kw) as b:
        a.load_cells(cells0)
        a.scalar_begin(phi0, omega_s=OMEGA_S)
        a.run_steps(3, accelerate_first=True)
        a.scalar_advance(2)
        after5 = None
        for i, k in enumerate((1, 2, 5, a.steps_per_launch() + 1)):
            kicked = _kick_and_check(a, p, obst, IMPULSES[i % 2], (what, k))
            b.load_cells(kicked)
            a.run_steps(k)
            b.run_steps(k)
            cells, av = a.store(n_av=k)
            cells_b, av_b = b.store(n_av=k)
            bad = _b32(cells) != _b32(cells_b)
            assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert np.array_equal(_b32(av), _b32(av_b)) and av.size == k, (what, k)
            a.scalar_advance(1)
            if i == 2:
                after5 = cells
        return after5


@pytest.mark.parametrize("mode", MODES)
def test_a_run_continues_from_the_kicked_lattice(gpu_lib, mode):
    kw, want = _mode(gpu_lib, mode)
    p, obst, cells0, phi0 = _problem(132, 70, 17, iters=40)
    _continuation(gpu_lib, p, obst, cells0, phi0, kw, mode)


@pytest.fixture(scope="module")
def single(gpu_lib):
    """{grid: (p, obst, cells0, phi0, last lattice)} of the single-domain handles: the reference of the
    decomposed cases, computed once and left unchanged."""
    out = {}
    for nx, ny in GRIDS:
        p, obst, cells0, phi0 = _problem(nx, ny, 31 + nx, iters=40)
        cells = _continuation(gpu_lib, p, obst, cells0, phi0, dict(parts=1), "single")
        for a in (obst, cells0, phi0, cells):
            a.setflags(write=False)
        out[(nx, ny)] = (p, obst, cells0, phi0, cells)
    return out


@pytest.mark.parametrize("grid", [(1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_decomposed_handles_kick_and_continue_bitwise(gpu_lib, single, nx, ny, grid):
    p, obst, cells0, phi0, ref = single[(nx, ny)]
    kw = dict(parts=grid[0] * grid[1], grid=grid, devices=[0])
    with gpu_lib.Engine(p, obst, **kw) as e:
        rects = e.local_rects()
        assert len(rects) == grid[0] * grid[1]
        if grid[1] == 2 and nx == 37:
            assert any(r[0] % 4 for r in rects)              # a sub-domain off the 16-B alignment
    cells = _continuation(gpu_lib, p, obst, cells0, phi0, kw, (nx, ny, grid))
    assert _same(cells, ref)                                 # a decomposed handle's bits are the single-domain handle's


# ------------------------------------- 7. degenerate shapes, the contract ----

@pytest.mark.parametrize("nx,ny", [(1, 1), (3, 1), (1, 5), (4, 1), (5, 3), (8, 2)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny):
    p, obst, cells0, phi0 = _problem(nx, ny, 5 + nx + 10 * ny, obstacles=0.2 if nx * ny > 4 else 0.0)
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, IMPULSES[0], (nx, ny), chunks=(3, 2, 1))


def test_all_obstacle_grid_keeps_every_bit(gpu_lib):
    p, _, cells0, phi0 = _problem(13, 6, 2)
    cells0[..., 3] = np.float32(-0.0)
    obst = np.ones((6, 13), np.uint8)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert _same(_kick_and_check(e, p, obst, IMPULSES[0], "all obstacles"), cells0)


def test_buoyancy_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 9)
    nan, inf = float("nan"), float("inf")
    with n.Engine(p, obst, flags=n.FLAG_PROFILE, parts=2, grid=(1, 2), devices=[0]) as e:
        L, h = e._L, e._h
        assert L.lbm_scalar_buoyancy(None, 0.1, 0.1, 0.0) == n.LBM_E_INVALID
        assert L.lbm_scalar_buoyancy(h, 0.1, 0.1, 0.0) == n.LBM_E_STATE             # before begin
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert L.lbm_scalar_buoyancy(h, 0.1, 0.1, 0.0) == n.LBM_E_STATE             # before the lattice is loaded
        cells0[..., 4] = np.float32(-0.0)
        e.load_cells(cells0)
        launches = lambda: sum(k["launches"] for k in e.profile_summary())          # noqa: E731
        before = launches()
        for bad in ((nan, 0.1, 0.0), (0.1, inf, 0.0), (0.1, 0.1, nan), (-inf, 0.1, 0.0)):
            assert L.lbm_scalar_buoyancy(h, *bad) == n.LBM_E_INVALID, bad
        assert b"finite" in L.lbm_last_error(h)
        # every component zero: LBM_OK, no launch, every bit stays (an added zero would flip the -0.0f)
        assert L.lbm_scalar_buoyancy(h, 0.0, 0.0, 5.0) == n.LBM_OK and L.lbm_scalar_buoyancy(h, -0.0, 0.0, 5.0) == n.LBM_OK
        assert launches() == before and _same(e.store(n_av=0)[0], cells0)
        assert not [k for k in e.profile_summary() if k["name"] == "scalar_buoyancy"]
        with pytest.raises(ValueError):
            e.scalar_buoyancy((0.1, 0.1, 0.1))
        # one launch per sub-domain
        _kick_and_check(e, p, obst, IMPULSES[1], "profile")
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["scalar_buoyancy"]["launches"] == 2 and prof["scalar_buoyancy"]["total_ms"] > 0
        e.scalar_end()
        assert L.lbm_scalar_buoyancy(h, 0.1, 0.1, 0.0) == n.LBM_E_STATE
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:       # a handle that never begins launches nothing new
        e.load_cells(cells0)
        e.run_steps(4, accelerate_first=True)
        assert not [k for k in e.profile_summary() if "scalar_" in k["name"]]


# ------------------------------------------- 8. run_thermal is its definition ----

def test_run_thermal_equals_the_loop_over_the_three_calls(gpu_lib):
    p, obst, cells0, phi0 = _problem(64, 32, 3, iters=13)
    accel = (0.0007, -0.0011)
    refs = {}
    for stride in (1, 3):
        with gpu_lib.Engine(p, obst) as e:                  # by hand
            e.load_cells(cells0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            av, done = [], 0
            while done < 13:
                n = min(stride, 13 - done)
                e.scalar_buoyancy([n * c for c in accel], PHI_REF)
                e.run_steps(n, accelerate_first=done == 0)
                av.append(e.store(cells=False, n_av=n)[1].copy())
                e.scalar_advance(n)
                done += n
            want = (e.store(n_av=0)[0], e.scalar(populations=True)[1], np.concatenate(av))
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            av = e.run_thermal(13, accel, PHI_REF, stride, accelerate_first=True)
            assert e.scalar_steps == 13
            got = (e.store(n_av=0)[0], e.scalar(populations=True)[1], av)
            with pytest.raises(ValueError):
                e.run_thermal(5, accel, stride=0)
        assert all(_same(a, b) for a, b in zip(got, want)), stride
        refs[stride] = want
        with gpu_lib.Engine(p, obst) as e:                  # the kick is felt: the uncoupled run differs
            e.load_cells(cells0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            e.run_scalar(13, stride, accelerate_first=True)
            assert not _same(e.store(n_av=0)[0], want[0])
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        hist = e.thermal_history(13, 5, accel, PHI_REF, accelerate_first=True)
        assert [s[0] for s in hist] == [5, 10, 13] and hist[-1][1:] == e.scalar_stats()
        assert _same(e.store(n_av=0)[0], refs[1][0]) and _same(e.scalar(populations=True)[1], refs[1][1])
    assert not _same(refs[1][0], refs[3][0])


def _rb_engine(n, ra):
    p, obst, cells0, phi0, fixed, s = tc.rayleigh_benard(ra)
    e = n.Engine(p, obst)
    e.load_cells(cells0)
    e.scalar_begin(phi0, omega_s=tc.RB_OMEGA)
    e.scalar_fix(*fixed)
    return e, p, obst, cells0, phi0, fixed, s


def test_run_thermal_equals_the_cpu_loop_bitwise(gpu_lib):
    """The first 50 steps of the Rayleigh-Benard set-up at Ra = 2200 on the default kernel."""
    e, p, obst, cells0, phi0, fixed, s = _rb_engine(gpu_lib, 2200)
    with e:
        e.run_thermal(50, s)
        cells, g = e.store(n_av=0)[0], e.scalar(populations=True)[1]
        assert e.kernel_in_use() in ("resident", "step2")
    g0 = lio.scalar_apply_fixed(lio.scalar_init(phi0), *fixed)
    want_cells, want_g = tc.cpu_thermal(p, obst, cells0, g0, tc.RB_OMEGA, s, 0.0, fixed, 50)
    assert _same(cells, want_cells) and _same(g, want_g)
    assert np.abs(lio.macroscopic(p, obst, cells)[0]).max() > 0                      # the roll turns


@pytest.mark.parametrize("ra", [1400, 2200])
def test_rayleigh_benard_onset_on_the_device(gpu_lib, ra):
    e, p, obst, *_, s = _rb_engine(gpu_lib, ra)
    with e:
        e.run_thermal(2000, s)
        u2000 = float(np.abs(e.fields(("ux",))["ux"]).max())
        e.run_thermal(2000, s)
        u4000 = float(np.abs(e.fields(("ux",))["ux"]).max())
        assert e.scalar_steps == 4000
    r = u4000 / u2000
    print(f"Ra {ra}: max |u_x| {u2000:.4e} at 2000, {u4000:.4e} at 4000, r = {r:.4f}")
    if ra < 1708:
        assert r < 1 and r < 0.8
    else:
        assert r > 1 and r > 2


# ------------------------------------------------------------ 9. runner ----

def test_runner_buoyancy_option(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    help_text = subprocess.run([str(exe), "--help"], capture_output=True, text=True, timeout=60)
    assert "--buoyancy" in help_text.stdout + help_text.stderr
    assert "--scalar-ref" in help_text.stdout + help_text.stderr
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "23"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    src = [(10, 64, 2.0, 1), (40, 40, 1.0, 0), (41, 40, 0.5, 0), (127, 127, 0.25, 0)]
    (tmp_path / "heat.txt").write_text("".join(f"{x} {y} {v!r}" + (" 1\n" if f else "\n") for x, y, v, f in src))
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles", str(obst_file)]
    scalar = ["--scalar", str(tmp_path / "heat.txt"), "--scalar-omega", "1.3"]
    phi0 = np.zeros((p.ny, p.nx), np.float32)
    for x, y, v, _ in src:
        phi0[y, x] = v
    for stride, ref in ((1, 0.0), (4, 0.125)):
        d = tmp_path / f"s{stride}"
        d.mkdir()
        r = subprocess.run(base + scalar + ["--buoyancy", "0,1e-4", "--scalar-ref", repr(ref), "--scalar-stride",
                                            str(stride), "--out-dir", str(d)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
        phi = lio.read_scalar_state(str(d / "scalar_state.dat"), p.nx, p.ny)
        final = (d / "final_state.dat").read_text()
        with gpu_lib.Engine(p, obst) as e:                   # the same thermal run through the binding
            e.load_cells(lio.init_cells(p))
            e.scalar_begin(phi0, omega_s=1.3)
            e.scalar_fix(np.array([10]), np.array([64]), np.array([2.0], np.float32))
            e.run_thermal(23, (0.0, 1e-4), ref, stride, accelerate_first=True)
            assert _same(phi, e.scalar())
            cells = e.store(n_av=0)[0]
            e.scalar_begin(phi0, omega_s=1.3)                # and the passive run, which must differ
            e.load_cells(lio.init_cells(p))
            e.run_scalar(23, stride, accelerate_first=True)
            assert not _same(cells, e.store(n_av=0)[0])
        want = tmp_path / f"want{stride}.dat"
        assert lio.write_results(str(want), p, obst, cells)
        assert final == want.read_text()
    r = subprocess.run(base + ["--buoyancy", "0,1e-4", "--out-dir", str(tmp_path)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "--scalar" in r.stderr and "--buoyancy" in r.stderr
    r = subprocess.run(base + scalar + ["--buoyancy", "0,1e-4", "--device", "cpu", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--buoyancy" in r.stderr
    r = subprocess.run(base + scalar + ["--buoyancy", "1e-4", "--out-dir", str(tmp_path)], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0
