"""D3Q19 on hard states and degenerate lattices (the 3-D counterpart of
tests/test_gpu_edge.py and of the adversarial-division tests of
tests/test_gpu_parity.py), each against the CPU restatement
(oracle/lbm_oracle3d.c):

  1. densities from 2^-126 to 2^100 -- the short division sequences of cell3d
     (rho/3, rho/18, rho/36 by multiply and two FMA corrections) and the
     wave-wide fallback to IEEE division for rho < 2^-120, with whole waves
     tiny (scale by row) and with tiny and normal lanes in one wave (scale by
     blocks of 8 columns), subnormal populations, exactly zero momentum;
  2. signed zeros: -0.0 populations that the body-force lines must turn into
     +0.0 on some speeds and keep on others;
  3. degenerate lattices: every cell an obstacle, one-cell / one-row / one-plane
     lattices (ny of 1 and 2), a periodic box without wall planes, zero steps,
     refused sizes;
  4. the tolerance collision (cell3dt) across binades: it is homogeneous in f
     without a force, so scaling the state by a power of two must scale the
     result exactly.

Every case names the pass form it is about and asserts through
Engine3D.run_stats() / .numerics() that this form ran:

    cell    LBM3D_PAIR=0 LBM3D_TWO=0     one step per launch, one cell per lane (step3d)
    pair    LBM3D_PAIR=1 LBM3D_TWO=0     one step per launch, column pairs (step3d_pair; even nx)
    two     LBM3D_TWO=1 LBM3D_THREE=0    two steps per pass (step3d_two)
    three   LBM3D_THREE=1                three steps per pass (step3d_three)

A shape excludes a form only when nx is odd (no pair kernel) or its z slabs
are thinner than 2n planes (no n-step pass); `permitted` computes that from the
shape, and no case catches a failure.  Items 1-3 are bitwise (bit patterns
compared, NaN positions equal, NaN payloads not compared).
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.usefixtures("debug_knobs")  # the pass forms are selected by knob

FORMS = {
    "cell": {"LBM3D_PAIR": "0", "LBM3D_TWO": "0"},
    "pair": {"LBM3D_PAIR": "1", "LBM3D_TWO": "0"},
    "two": {"LBM3D_TWO": "1", "LBM3D_THREE": "0"},
    "three": {"LBM3D_THREE": "1"},
}
PASS_DEPTH = {"cell": 1, "pair": 1, "two": 2, "three": 3}
# step counts at which the form under test does all or most of the work
FORM_STEPS = {"cell": (1, 3), "pair": (1, 3), "two": (2, 3), "three": (3, 4)}
# |c|^2 = 0, 1, 2 -> 1/3, 1/18, 1/36 in the ABI's speed order (include/lbm3d_hip.h)
W = np.array([1 / 3] + [1 / 18] * 4 + [1 / 36] * 4 + ([1 / 18] + [1 / 36] * 4) * 2)


def permitted(form, nx, nz, parts=1):
    """Whether a lattice of this shape, cut into `parts` z slabs, can run `form`."""
    if form == "pair":
        return nx % 2 == 0
    n = PASS_DEPTH[form]
    return n == 1 or parts == 1 or nz // parts >= 2 * n   # the thinnest slab has floor(nz / parts) planes


def forms_for(nx, nz, parts=1):
    return [f for f in FORMS if permitted(f, nx, nz, parts)]


def expected_stats(form, steps, nx):
    """run_stats() of `steps` steps in `form`: (three-step passes, two-step passes,
    one-step launches, pair kernel)."""
    n3 = steps // 3 if form == "three" else 0
    n2 = (steps - 3 * n3) // 2 if form in ("two", "three") else 0
    return n3, n2, steps - 3 * n3 - 2 * n2, int(form != "cell" and nx % 2 == 0)


def run_form(native, monkeypatch, form, p, obst, c0, steps, parts=1, flags=0):
    """`steps` steps in `form` on device 0; asserts that the form ran."""
    assert permitted(form, p.nx, p.nz, parts)
    for k in ("LBM3D_PAIR", "LBM3D_TWO", "LBM3D_THREE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    with native.Engine3D(p, obst, parts=parts, devices=[0], flags=flags) as e:
        e.load_cells(c0)
        e.run_steps(steps)
        cells, av = e.store(n_av=steps)
        assert e.run_stats() == expected_stats(form, steps, p.nx), (form, steps, e.run_stats())
        tol = bool(flags & native.FLAG_TOLERANCE) and PASS_DEPTH[form] > 1
        assert e.numerics() == ("tolerance" if tol else "bitwise")
    return cells, av


def assert_bitwise(cells, ref, what):
    nan_r = np.isnan(ref)
    assert np.array_equal(np.isnan(cells), nan_r), f"{what}: NaN positions differ"
    same = (cells.view(np.uint32) == ref.view(np.uint32)) | nan_r
    if not same.all():
        bad = np.argwhere(~same)
        z, y, x, k = bad[0]
        pytest.fail(f"{what}: {len(bad)} values differ, first at z={z} y={y} x={x} k={k}: "
                    f"gpu {cells[z, y, x, k]!r} oracle {ref[z, y, x, k]!r}")


def assert_av(av, ref_av):
    both = np.isfinite(ref_av)
    assert np.array_equal(np.isfinite(av), both), (av, ref_av)
    np.testing.assert_allclose(av[both], ref_av[both], rtol=1e-5)


def form_parts(nx, nz, parts_list):
    """[(form, parts)] of every form the shape permits, per slab count."""
    return [(f, parts) for parts in parts_list for f in forms_for(nx, nz, parts)]


# ------------------------------------------------ 1. adversarial densities ----

ANX, ANY, ANZ = 128, 22, 12
SCALES = 2.0 ** np.array([0, -20, -60, -100, -110, -118, -120, -121, -122, -124, -126, 20, 40, 100], np.float64)


@functools.lru_cache(maxsize=None)
def adversarial_state(layout):
    """Populations 0.1 scale w_k with the scale set per group -- a row y ("rows": whole
    waves tiny) or a block of 8 columns ("cols": every wave mixes scales 2^-126 .. 2^100,
    and the pair kernel's DPP neighbours lie 2^40 apart); every third group unperturbed
    (momentum exactly 0), the others times 1 + 1e-3 N(0, 1)."""
    rng = np.random.default_rng(5)
    g = np.arange(ANY)[None, :, None] if layout == "rows" else (np.arange(ANX) // 8)[None, None, :]
    g = g * np.ones((ANZ, ANY, ANX), np.int64)
    base = 0.1 * SCALES[g % len(SCALES)][..., None] * W
    pert = np.where((g % 3 == 0)[..., None], 1.0, 1 + 1e-3 * rng.standard_normal((ANZ, ANY, ANX, 19)))
    c0 = (base * pert).astype(np.float32)
    c0.setflags(write=False)
    return c0


def adversarial_problem():
    return lio.Params3D(ANX, ANY, ANZ, 0, 0.1, 0.0, 1.85), np.zeros((ANZ, ANY, ANX), np.uint8)


@functools.lru_cache(maxsize=None)
def adversarial_ref(layout, steps):
    p, obst = adversarial_problem()
    ref, _ = oracle.run3d(p, obst, steps, adversarial_state(layout))
    ref.setflags(write=False)
    return ref


@pytest.mark.parametrize("layout", ["rows", "cols"])
def test_adversarial_states_reach_the_hard_paths(layout):
    """CPU: what the GPU test below relies on -- through 3 steps the restatement
    stays finite, holds cells below the fallback threshold 2^-120 at every step and
    subnormal populations at steps 1 and 2; the column layout reaches negative
    densities at step 3; unperturbed groups start with exactly zero momentum."""
    c0 = adversarial_state(layout)
    tiny = np.float32(2.0 ** -126)
    for steps in (0, 1, 2, 3):
        c = adversarial_ref(layout, steps) if steps else c0
        rho = c.sum(-1, dtype=np.float32)
        assert np.isfinite(c).all(), steps
        assert (rho < 2.0 ** -120).any(), steps
        if steps in (1, 2):
            assert ((np.abs(c) < tiny) & (c != 0)).any(), steps
    if layout == "cols":
        assert (adversarial_ref(layout, 3).sum(-1, dtype=np.float32) < 0).any()
    zero_mom = (c0[..., 1] == c0[..., 2]) & (c0[..., 3] == c0[..., 4]) & (c0[..., 9] == c0[..., 14])
    assert zero_mom.any() and not zero_mom.all()


@pytest.mark.gpu
@pytest.mark.parametrize("form,parts", form_parts(ANX, ANZ, [1, 2]))
@pytest.mark.parametrize("layout", ["rows", "cols"])
def test_division_adversarial_states_bitwise(gpu_lib, layout, form, parts, monkeypatch):
    """cell3d's short divisions and its IEEE fallback (pair kernel and both passes)
    and step3d's plain '/' against the restatement's correctly rounded '/', bit for
    bit, on the states above; no obstacles and no force, omega 1.85."""
    p, obst = adversarial_problem()
    c0 = adversarial_state(layout)
    for steps in FORM_STEPS[form]:
        ref = adversarial_ref(layout, steps)
        assert np.isfinite(ref).all()
        cells, _ = run_form(gpu_lib, monkeypatch, form, p, obst, c0, steps, parts=parts)
        assert_bitwise(cells, ref, f"{layout} {form} parts={parts} {steps} steps")


# ------------------------------------------------------- 2. signed zeros ----

@functools.lru_cache(maxsize=None)
def signed_zero_state():
    c0 = np.zeros((ANZ, ANY, ANX, 19), np.float32)
    c0[..., 0] = np.float32(1e-45)
    c0[..., 3] = np.float32(1e-40)
    c0[..., 4] = np.float32(-1e-40)
    c0.setflags(write=False)
    return c0


@functools.lru_cache(maxsize=None)
def signed_zero_ref(accel, steps):
    p = lio.Params3D(ANX, ANY, ANZ, 0, 0.1, accel, 1.85)
    ref, _ = oracle.run3d(p, np.zeros((ANZ, ANY, ANX), np.uint8), steps, signed_zero_state())
    ref.setflags(write=False)
    return ref


def negative_zero_speeds(c):
    nz = np.signbit(c) & (c == 0)
    return {k for k in range(19) if nz[..., k].any()}


# speeds that hold -0.0 in the restatement: without a force after steps 1 and 3 / step 2;
# with a force (1 step) the "+ w" and "- w" lines leave it only where no line acts
NEG_ZERO_ODD, NEG_ZERO_EVEN, NEG_ZERO_FORCED = {2, 9, 11, 14, 15}, {6, 8, 12, 13, 17, 18}, {9, 14}


def test_signed_zero_reference_holds_negative_zeros():
    """CPU: the state (a density that underflows rho w omega to +0 under a huge
    |u|^2) gives -0.0 on exactly the speeds the GPU test expects, and with a force
    the restatement is NaN from step 2 on."""
    assert negative_zero_speeds(signed_zero_ref(0.0, 1)) == NEG_ZERO_ODD
    assert negative_zero_speeds(signed_zero_ref(0.0, 2)) == NEG_ZERO_EVEN
    assert negative_zero_speeds(signed_zero_ref(0.0, 3)) == NEG_ZERO_ODD
    assert negative_zero_speeds(signed_zero_ref(0.005, 1)) == NEG_ZERO_FORCED
    assert not np.isnan(signed_zero_ref(0.005, 1)).any() and np.isnan(signed_zero_ref(0.005, 2)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("form,parts", form_parts(ANX, ANZ, [1, 2]))
def test_signed_zero_states_bitwise(gpu_lib, form, parts, monkeypatch):
    """-0.0 populations: `o + w` turns -0 into +0 even for w = 0, `o - w` and the
    six force-free pairs keep it -- a kernel that dropped the force lines at a = 0,
    or added the force to another speed, differs in the sign bit."""
    obst = np.zeros((ANZ, ANY, ANX), np.uint8)
    c0 = signed_zero_state()
    for accel, step_counts in ((0.0, (1, 2, 3)), (0.005, (1,))):
        p = lio.Params3D(ANX, ANY, ANZ, 0, 0.1, accel, 1.85)
        for steps in step_counts:
            ref = signed_zero_ref(accel, steps)
            assert negative_zero_speeds(ref)  # the reference really contains -0.0
            cells, _ = run_form(gpu_lib, monkeypatch, form, p, obst, c0, steps, parts=parts)
            assert_bitwise(cells, ref, f"{form} parts={parts} accel={accel} {steps} steps")


# ------------------------------------------------ 3. degenerate lattices ----

def perturbed(p, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    return (oracle.init_cells3d(p) * (1 + noise * rng.standard_normal((p.nz, p.ny, p.nx, 19)))).astype(np.float32)


def shape_cases(shapes, parts_of):
    """[(nx, ny, nz, form, parts)] of every permitted form of every shape and slab count."""
    return [(nx, ny, nz, f, parts) for nx, ny, nz in shapes for parts in parts_of(nz)
            for f in forms_for(nx, nz, parts)]


@pytest.mark.gpu
@pytest.mark.parametrize("tolerance", [False, True])
@pytest.mark.parametrize("nx,ny,nz,form,parts", shape_cases([(12, 5, 6), (128, 6, 12)], lambda nz: [1, 2]))
def test_all_obstacles_bitwise(gpu_lib, nx, ny, nz, form, parts, tolerance, monkeypatch):
    """Every cell an obstacle: 7 steps of pure bounce-back equal the restatement's,
    av_vels is 0 / 0 fluid cells = NaN in both -- in tolerance mode too (rebound
    does no arithmetic, so that lattice is bitwise as well)."""
    steps = 7
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.7)
    obst = np.ones((nz, ny, nx), np.uint8)
    c0 = perturbed(p, 5)
    ref, ref_av = oracle.run3d(p, obst, steps, c0)
    cells, av = run_form(gpu_lib, monkeypatch, form, p, obst, c0, steps, parts=parts,
                         flags=gpu_lib.FLAG_TOLERANCE if tolerance else 0)
    assert_bitwise(cells, ref, f"{form} parts={parts}")
    assert np.isnan(ref_av).all() and np.isnan(av).all(), av


TINY_SHAPES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (5, 1, 1), (1, 1, 5), (64, 1, 3), (2, 2, 2), (3, 2, 4),
               (130, 2, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("walls", [False, True])
@pytest.mark.parametrize("nx,ny,nz,form,parts", shape_cases(TINY_SHAPES, lambda nz: [1, 2] if nz >= 2 else [1]))
def test_tiny_lattices_bitwise(gpu_lib, nx, ny, nz, form, parts, walls, monkeypatch):
    """One cell, one row, one column, one plane, ny of 1 and 2: every periodic wrap
    lands on the cell's own row, column or plane.  No obstacle, and every other cell
    an obstacle; 9 steps."""
    steps = 9
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.005, 1.85)
    obst = np.zeros((nz, ny, nx), np.uint8)
    if walls:
        obst.reshape(-1)[::2] = 1
    c0 = perturbed(p, 11 + 7 * nx + 3 * ny + nz)
    ref, ref_av = oracle.run3d(p, obst, steps, c0)
    cells, av = run_form(gpu_lib, monkeypatch, form, p, obst, c0, steps, parts=parts)
    assert_bitwise(cells, ref, f"{nx}x{ny}x{nz} {form} parts={parts} walls={walls}")
    assert_av(av, ref_av)


@functools.lru_cache(maxsize=None)
def periodic_box(nx, ny, nz):
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.02, 1.7)
    rng = np.random.default_rng(nx + ny + nz)
    obst = (rng.random((nz, ny, nx)) < 0.05).astype(np.uint8)  # no wall planes: fluid crosses the y seam
    c0 = perturbed(p, nx * ny + nz)
    ref, ref_av = oracle.run3d(p, obst, 9, c0)
    return p, obst, c0, ref, ref_av


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,nz,form,parts", shape_cases([(70, 31, 24), (61, 17, 5)], lambda nz: [1, 3]))
def test_wall_free_periodic_box_bitwise(gpu_lib, nx, ny, nz, form, parts, monkeypatch):
    """A periodic box with 5 % random obstacles and no wall planes (every other
    D3Q19 GPU lattice has solid planes at y = 0 and ny - 1), driven hard (a = 0.02),
    9 steps, one slab and three."""
    p, obst, c0, ref, ref_av = periodic_box(nx, ny, nz)
    assert not obst[:, 0, :].all() and not obst[:, -1, :].all()
    cells, av = run_form(gpu_lib, monkeypatch, form, p, obst, c0, 9, parts=parts)
    assert_bitwise(cells, ref, f"{nx}x{ny}x{nz} {form} parts={parts}")
    assert_av(av, ref_av)


@pytest.mark.gpu
@pytest.mark.parametrize("parts", [1, 2])
def test_zero_steps(gpu_lib, parts):
    """run_steps(0) leaves the lattice as loaded (and as a run left it), reports no
    pass and no launch, and store() has no av_vels to give: zeros, never stale ones."""
    p = lio.Params3D(22, 9, 12, 0, 0.1, 0.002, 1.7)
    obst = lio.channel_obstacles3d(p.nx, p.ny, p.nz)
    c0 = perturbed(p, 3)
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        e.load_cells(c0)
        assert e.run_stats()[:3] == (0, 0, 0)
        e.run_steps(0)
        cells, av = e.store(n_av=0)
        assert len(av) == 0 and e.run_stats()[:3] == (0, 0, 0)
        assert np.array_equal(cells.view(np.uint32), c0.view(np.uint32))
        e.run_steps(4)
        assert sum(n * k for n, k in zip(e.run_stats()[:3], (3, 2, 1))) == 4
        after4, av4 = e.store(n_av=4)
        assert (av4 > 0).all()
        e.run_steps(0)
        cells, av = e.store(n_av=4)
        assert e.run_stats()[:3] == (0, 0, 0)
        assert np.array_equal(cells.view(np.uint32), after4.view(np.uint32))
        assert np.array_equal(av, np.zeros(4, np.float32))
    ref, _ = oracle.run3d(p, obst, 4, c0)
    assert_bitwise(after4, ref, "4 steps between two empty runs")


@pytest.mark.gpu
@pytest.mark.parametrize("nx,ny,nz,iters,parts", [(0, 4, 4, 2, 1), (4, 0, 4, 2, 1), (4, 4, 0, 2, 1), (4, 4, 4, -1, 1),
                                                  (4, 4, 4, 2, 5)])
def test_invalid_sizes_refused(gpu_lib, nx, ny, nz, iters, parts):
    """An empty extent, max_iters < 0 and more slabs than planes: LBM_E_INVALID at create."""
    p = lio.Params3D(nx, ny, nz, iters, 0.1, 0.002, 1.7)
    with pytest.raises(gpu_lib.LbmError) as ei:
        gpu_lib.Engine3D(p, np.zeros((nz, ny, nx), np.uint8), parts=parts, devices=[0])
    assert ei.value.code == gpu_lib.LBM_E_INVALID


@pytest.mark.gpu
def test_negative_steps_refused(gpu_lib):
    """run_steps(-1): LBM_E_INVALID, the lattice and the last run's counts untouched."""
    p = lio.Params3D(22, 9, 6, 0, 0.1, 0.002, 1.7)
    obst = lio.channel_obstacles3d(p.nx, p.ny, p.nz)
    c0 = perturbed(p, 4)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(5)
        stats = e.run_stats()
        before, _ = e.store()
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.run_steps(-1)
        assert ei.value.code == gpu_lib.LBM_E_INVALID
        assert e.run_stats() == stats
        after, _ = e.store()
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))


# ------------------------------- 4. tolerance collision across binades ----

SCALE_EXPONENTS = (-100, -60, 40, 100)
SCALE_STEPS = 6


@functools.lru_cache(maxsize=None)
def scale_problem():
    """A benign state (walls, 5 % obstacles, 2 % noise, no force) and the restatement's
    lattices of it and of its power-of-two multiples, which must be exact multiples of
    each other: power-of-two scaling commutes with every IEEE operation of a step that
    is homogeneous in f, away from the exponent limits."""
    nx, ny, nz = 70, 31, 24
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.0, 1.7)
    rng = np.random.default_rng(77)
    obst = lio.channel_obstacles3d(nx, ny, nz)
    obst[rng.random((nz, ny, nx)) < 0.05] = 1
    c0 = perturbed(p, 78, noise=0.02)
    ref0, _ = oracle.run3d(p, obst, SCALE_STEPS, c0)
    refs = {}
    for k in SCALE_EXPONENTS:
        s = np.float32(2.0 ** k)
        refs[k], _ = oracle.run3d(p, obst, SCALE_STEPS, c0 * s)
        assert np.isfinite(refs[k]).all() and (refs[k] != 0).all()
        assert np.array_equal(refs[k].view(np.uint32), (ref0 * s).view(np.uint32)), k
    return p, obst, c0, ref0, refs


def test_oracle3d_is_scale_covariant():
    """CPU: the restatement of c0 2^k is 2^k times that of c0, bit for bit."""
    scale_problem()


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["two", "three"])
def test_tolerance_collision_scale_covariant(gpu_lib, form, monkeypatch):
    """cell3dt on c0 2^k, k = -100, -60, 40, 100 (6 steps: three two-step or two
    three-step passes): finite, every population within the header's 2e-5
    (relative, per population: this state stays far from cancellation) of the
    restatement on the scaled state, and 2^k times the tolerance lattice of c0 bit
    for bit -- v_rcp_f32 and the FMA chain see the same significands.  Measured on
    an MI355X: 0 ulp from 2^k x base at every k, both forms; largest relative
    deviation from the restatement 2.0e-6 (the same figure at every k, as it must be)."""
    p, obst, c0, ref0, refs = scale_problem()
    tol = gpu_lib.FLAG_TOLERANCE
    base, _ = run_form(gpu_lib, monkeypatch, form, p, obst, c0, SCALE_STEPS, flags=tol)
    assert not np.array_equal(base, ref0)  # the flag selects the other collision
    for k in SCALE_EXPONENTS:
        s = np.float32(2.0 ** k)
        cells, _ = run_form(gpu_lib, monkeypatch, form, p, obst, c0 * s, SCALE_STEPS, flags=tol)
        assert np.isfinite(cells).all(), k
        dev = float(np.max(np.abs(cells.astype(np.float64) - refs[k]) / np.abs(refs[k].astype(np.float64))))
        print(f"D3Q19 tolerance {form} 2^{k}: max relative deviation {dev:.3e}")
        assert dev < 2e-5, (k, dev)
        want = base * s
        ulp = np.abs(cells.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
        print(f"D3Q19 tolerance {form} 2^{k}: max ulp distance to 2^k x base {int(ulp)}")
        assert_bitwise(cells, want, f"tolerance {form} scaled by 2^{k} vs 2^{k} x base")
