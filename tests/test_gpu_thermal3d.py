"""Boussinesq buoyancy on the device, D3Q19 (lbm3d_scalar_buoyancy; include/lbm_thermal_hip.h,
csrc/lbm3d_scalar.hip, csrc/lbm_scalar.hpp).

Bar: after every scalar_buoyancy the stored lattice is BITWISE (uint32 patterns) lio.buoyancy_kick3d
of what the same handle stored just before, on both sides of the flow pair, for both numerics, 1, 2
and 3 z slabs and degenerate shapes; a run of 1, 2, 3 or 5 steps afterwards -- every pass form reads
kicked ghost planes -- continues bit for bit as a second handle does that loaded the kicked cells;
run_thermal is its definition and, at stride 1, the CPU loop (oracle step + lio) bit for bit.  No
tolerance anywhere.
"""
from __future__ import annotations

import numpy as np
import pytest

import thermal_cases as tc
from lbm_amd import io as lio
from oracle import oracle

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2, 5)      # flow steps before each kick: both lattices of the pair get kicked
ADVANCES = (1, 2, 3, 1, 2)
GRIDS = [(13, 7, 5), (16, 8, 8)]
OMEGA_S = 1.3
IMPULSES = [(0.004, -0.003, 0.002), (0.0, 0.0, 0.005)]
PHI_REF = 1.4

_b32, _same = tc.b32, tc.same


def _problem(nx, ny, nz, seed, obstacles=0.1, walls=True):
    """The channel walls plus about 10 % random obstacles; populations perturbed by 5 %; phi0 in [1, 2)."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    rng = np.random.default_rng(seed)
    obst = (rng.random((nz, ny, nx)) < obstacles).astype(np.uint8)
    if walls:
        obst |= lio.channel_obstacles3d(nx, ny, nz)
        obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    c0[obst != 0, 2::5] = np.float32(-0.0)
    phi0 = (1 + rng.random((nz, ny, nx))).astype(np.float32)
    for a in (obst, c0, phi0):
        a.setflags(write=False)
    return p, obst, c0, phi0


def _fixed(p, n=4, seed=3):
    rng = np.random.default_rng(seed)
    cells = {(0, 0, 0), (p.nx - 1, p.ny - 1, p.nz - 1)}
    while len(cells) < min(n, p.nx * p.ny * p.nz):
        cells.add((int(rng.integers(p.nx)), int(rng.integers(p.ny)), int(rng.integers(p.nz))))
    x, y, z = np.array(sorted(cells), np.int32).T
    return x, y, z, (3 + rng.random(x.size)).astype(np.float32)


def _kick_and_check(e, p, obst, s, what=""):
    before = e.store()[0]
    phi, g = e.scalar(populations=True)
    steps = e.scalar_steps
    e.scalar_buoyancy(s, PHI_REF)
    got = e.store()[0]
    want = lio.buoyancy_kick3d(before, g, obst, p.density, s, PHI_REF)
    bad = _b32(got) != _b32(want)
    assert not bad.any(), (what, s, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert _same(got[obst != 0], before[obst != 0]) and (obst.all() or not _same(got, before)), what
    phi2, g2 = e.scalar(populations=True)
    assert _same(g2, g) and _same(phi2, phi) and e.scalar_steps == steps, what
    return got


def _sequence(e, p, obst, c0, phi0, s, what="", chunks=CHUNKS):
    e.load_cells(c0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    fixed = _fixed(p)
    e.scalar_fix(*fixed)
    cells = None
    for i, (c, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(c)
        e.scalar_advance(n)
        cells = _kick_and_check(e, p, obst, s, (what, i))
        held = lio.scalar_phi(lio.scalar_init3d(fixed[3].reshape(1, 1, -1)))[0, 0]
        assert _same(e.scalar()[fixed[2], fixed[1], fixed[0]], held)
    return cells


# ------------------------------------------------------- 5. kick, bitwise ----

@pytest.mark.parametrize("s", IMPULSES)
@pytest.mark.parametrize("form", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_kick_sequences_bitwise(gpu_lib, nx, ny, nz, form, s):
    p, obst, c0, phi0 = _problem(nx, ny, nz, 7)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        _sequence(e, p, obst, c0, phi0, s, (nx, ny, nz, form, s))


def test_wide_rows_cross_waves_and_blocks(gpu_lib):
    """nx = 300: more than one wave of quads per row and a ragged tail; nx = 258: a tail of two cells."""
    for nx in (300, 258):
        p, obst, c0, phi0 = _problem(nx, 5, 3, nx)
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            _sequence(e, p, obst, c0, phi0, IMPULSES[0], nx, chunks=(2, 1))


# ------------------------------------------------ 6. continuation, bitwise ----

def _continuation(n, p, obst, c0, phi0, kw, what):
    """Kick, then run k steps -- on the kicked handle and on a second one that loaded the kicked cells --
    for k = 1, 2, 3, 5: one-, two- and three-step passes all start from kicked ghost planes.  Returns the
    last lattice and the (three-step, two-step, one-step) counts of each run."""
    with n.Engine3D(p, obst, **kw) as a, n.Engine3D(p, obst, **kw) as b:
        a.load_cells(c0)
        a.scalar_begin(phi0, omega_s=OMEGA_S)
        a.run_steps(3)
        a.scalar_advance(2)
        cells, forms = None, []
        for i, k in enumerate((1, 2, 3, 5)):
            kicked = _kick_and_check(a, p, obst, IMPULSES[i % 2], (what, k))
            b.load_cells(kicked)
            a.run_steps(k)
            forms.append(a.run_stats()[:3])
            b.run_steps(k)
            cells, cells_b = a.store()[0], b.store()[0]
            bad = _b32(cells) != _b32(cells_b)
            assert not bad.any(), (what, k, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            a.scalar_advance(1)
        return cells, forms


@pytest.fixture(scope="module")
def single(gpu_lib):
    out = {}
    for grid in GRIDS:
        p, obst, c0, phi0 = _problem(*grid, 11)
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            assert len(e.local_slabs()) == 1
        cells, _ = _continuation(gpu_lib, p, obst, c0, phi0, dict(devices=[0]), "single")
        cells.setflags(write=False)
        out[grid] = (p, obst, c0, phi0, cells)
    return out


@pytest.mark.parametrize("form", ["bitwise", "tolerance"])
def test_a_run_continues_from_the_kicked_lattice(gpu_lib, form):
    p, obst, c0, phi0 = _problem(16, 8, 8, 19)
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    _, forms = _continuation(gpu_lib, p, obst, c0, phi0, kw, form)
    print(f"{form}: (three, two, one) per run of 1, 2, 3, 5 steps: {forms}")
    assert forms[0] == (0, 0, 1) and forms[1] == (0, 1, 0)                # a one-step launch, a two-step pass
    assert forms[2] in ((1, 0, 0), (0, 1, 1)) and sum(f[0] for f in forms) > 0     # and three-step passes


@pytest.mark.parametrize("parts", [2, 3])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_slabs_kick_and_continue_bitwise(gpu_lib, single, nx, ny, nz, parts):
    p, obst, c0, phi0, ref = single[(nx, ny, nz)]
    with gpu_lib.Engine3D(p, obst, parts=parts, devices=[0]) as e:
        assert len(e.local_slabs()) == parts
    cells, _ = _continuation(gpu_lib, p, obst, c0, phi0, dict(parts=parts, devices=[0]), (nx, ny, nz, parts))
    assert _same(cells, ref)                                 # the slabs' bits are the single slab's


# ------------------------------------- 7. degenerate shapes, the contract ----

@pytest.mark.parametrize("nx,ny,nz", [(2, 2, 1), (1, 1, 1), (1, 5, 4), (3, 2, 2), (6, 1, 4), (4, 1, 1), (5, 4, 1)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny, nz):
    """Among them nx < 4: one cell per lane."""
    p, obst, c0, phi0 = _problem(nx, ny, nz, 5, 0.2 if nx * ny * nz > 8 else 0.0, False)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        _sequence(e, p, obst, c0, phi0, IMPULSES[0], (nx, ny, nz), chunks=(3, 2, 1))


def test_buoyancy_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0, phi0 = _problem(13, 7, 5, 9)
    nan, inf = float("nan"), float("inf")
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        assert L.lbm3d_scalar_buoyancy(None, 0.1, 0.1, 0.1, 0.0) == n.LBM_E_INVALID
        assert L.lbm3d_scalar_buoyancy(h, 0.1, 0.1, 0.1, 0.0) == n.LBM_E_STATE          # before begin
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert L.lbm3d_scalar_buoyancy(h, 0.1, 0.1, 0.1, 0.0) == n.LBM_E_STATE          # before the lattice is loaded
        e.load_cells(c0)
        for bad in ((nan, 0.1, 0.1, 0.0), (0.1, inf, 0.1, 0.0), (0.1, 0.1, -inf, 0.0), (0.1, 0.1, 0.1, nan)):
            assert L.lbm3d_scalar_buoyancy(h, *bad) == n.LBM_E_INVALID, bad
        assert b"finite" in L.lbm3d_last_error(h)
        assert L.lbm3d_scalar_buoyancy(h, 0.0, -0.0, 0.0, 5.0) == n.LBM_OK
        assert _same(e.store()[0], c0) and (_b32(c0) == 0x80000000).any()                # every bit, -0.0f included
        with pytest.raises(ValueError):
            e.scalar_buoyancy((0.1, 0.1))
        _kick_and_check(e, p, obst, IMPULSES[1], "contract")
        e.scalar_end()
        assert L.lbm3d_scalar_buoyancy(h, 0.1, 0.1, 0.1, 0.0) == n.LBM_E_STATE


# ------------------------------------------- 8. run_thermal is its definition ----

def test_run_thermal_equals_the_loop_over_the_three_calls(gpu_lib):
    p, obst, c0, phi0 = _problem(16, 8, 8, 21)
    accel = (0.0007, -0.0011, 0.0005)
    refs = {}
    for stride in (1, 3):
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:                  # by hand
            e.load_cells(c0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            done = 0
            while done < 13:
                n = min(stride, 13 - done)
                e.scalar_buoyancy([n * c for c in accel], PHI_REF)
                e.run_steps(n)
                e.scalar_advance(n)
                done += n
            refs[stride] = (e.store()[0], e.scalar(populations=True)[1])
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            e.load_cells(c0)
            e.scalar_begin(phi0, omega_s=OMEGA_S)
            av = e.run_thermal(13, accel, PHI_REF, stride)
            assert av.size == 0 and e.scalar_steps == 13
            assert _same(e.store()[0], refs[stride][0]) and _same(e.scalar(populations=True)[1], refs[stride][1])
            with pytest.raises(ValueError):
                e.run_thermal(5, accel, accelerate_first=True)
    assert not _same(refs[1][0], refs[3][0])
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        hist = e.thermal_history(13, 5, accel, PHI_REF)
        assert [s[0] for s in hist] == [5, 10, 13] and hist[-1][1:] == e.scalar_stats()
        assert _same(e.store()[0], refs[1][0])
        e.load_cells(c0)                                                    # the kick is felt
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        e.run_scalar(13, 1)
        assert not _same(e.store()[0], refs[1][0])


def test_run_thermal_equals_the_cpu_loop_bitwise(gpu_lib):
    """30 steps of the 3-D heated slot (34 x 4 x 4, gravity along z) at stride 1."""
    p, obst, c0, phi0, fixed, s = tc.slot(3)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(c0)
        e.scalar_begin(phi0, omega_s=1.0)
        e.scalar_fix(*fixed)
        e.run_thermal(30, s)
        cells, g = e.store()[0], e.scalar(populations=True)[1]
    g0 = lio.scalar_apply_fixed3d(lio.scalar_init3d(phi0), *fixed)
    want_cells, want_g = tc.cpu_thermal(p, obst, c0, g0, 1.0, s, 0.0, fixed, 30, dims=3)
    assert _same(cells, want_cells) and _same(g, want_g)
    assert np.abs(lio.macroscopic3d(p, obst, cells)[2]).max() > 1e-5               # the slot flows along z
