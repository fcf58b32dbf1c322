"""The scalar transport sums on the device, D2Q9 + D2Q5 (lbm_scalar_store_binned;
include/lbm_transport_hip.h, csrc/lbm_transport.hip, csrc/lbm_transport.hpp).

Bar: after every chunk of flow and scalar steps the sums are lio.scalar_binned_sums of the same
handle's fields() and scalar(populations=True) -- the numpy restatement of the header's definition,
pinned by physics in tests/test_transport_host.py: BITWISE (uint64 patterns) at one-cell bins,
within the fold bound 2 (n - 1) 2^-53 sum|term| of the math.fsum value at larger bins -- for every
flow kernel, both numerics, both sides of both ping-pong pairs, decomposed handles, degenerate
shapes and subsets of the fields (the no-flow form of the kernel).  A call changes nothing on the
handle.  The Rayleigh-Benard heat flux on the device is flat over the planes and is the CPU loop's.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import thermal_cases as tc
import transport_cases as xc
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

CHUNKS = (3, 1, 4, 2)         # flow steps of each chunk: both lattices of the flow pair get read
ADVANCES = (1, 2, 3, 1)       # scalar steps of each chunk: both sets of the scalar pair get read
GRIDS = [(37, 19), (64, 32)]
OMEGA_S = 1.3
FACES = ("fx", "fy")

_b32, _same = tc.b32, tc.same


def _problem(nx, ny, seed, obstacles=0.1):
    """About 10 % random obstacles on a 5 % perturbed equilibrium, and a random phi0 in [-1, 1)."""
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, 8, 10, 0.1, 0.005, 1.85)
    obst = (rng.random((ny, nx)) < obstacles).astype(np.uint8)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    phi0 = (2 * rng.random((ny, nx)) - 1).astype(np.float32)
    return p, obst, cells, phi0


def _fixed(p, obst):
    """The first and the last cell, an obstacle cell and a fluid cell when there are any."""
    cells = {(0, 0), (p.nx - 1, p.ny - 1)}
    for a in (np.argwhere(obst != 0), np.argwhere(obst == 0)):
        if len(a):
            cells.add((int(a[len(a) // 2][1]), int(a[len(a) // 2][0])))
    x, y = np.array(sorted(cells), np.int32).T
    return x, y, np.linspace(2, 3, x.size).astype(np.float32)


def _begin(e, p, obst, cells0, phi0):
    e.load_cells(cells0)
    e.scalar_begin(phi0, omega_s=OMEGA_S)
    e.scalar_fix(*_fixed(p, obst))


def _terms(e, obst):
    """The restatement's per-cell terms of the handle's own state."""
    f = e.fields(("ux", "uy"))
    return lio.scalar_terms(e.scalar(populations=True)[1], f["ux"], f["uy"], obst)


def _sequence(e, p, obst, cells0, phi0, bins_list, what="", chunks=CHUNKS):
    """The call sequence of every parity test; returns the one-cell sums after the last chunk."""
    _begin(e, p, obst, cells0, phi0)
    last = None
    for i, (steps, n) in enumerate(zip(chunks, ADVANCES)):
        e.run_steps(steps, accelerate_first=i == 0)
        e.scalar_advance(n)
        terms = _terms(e, obst)
        for bins in bins_list:
            got = e.scalar_binned(*bins)
            assert set(got) == set(lio.SBIN_FIELDS) | {"fluid"}
            xc.check_binned(got, terms, obst, bins, (what, i, bins))
        last = terms
    return last


# ------------------------------------------------------ 1. one-cell bins ----

@pytest.mark.parametrize("nx,ny", GRIDS)
def test_one_cell_bins_bitwise(gpu_lib, nx, ny):
    p, obst, cells0, phi0 = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        terms = _sequence(e, p, obst, cells0, phi0, [(1, 1)], (nx, ny))
    assert obst.any() and all(np.abs(terms[n]).max() > 1e-4 for n in lio.SBIN_FIELDS)


@pytest.mark.parametrize("nx,ny", [(1, 1), (1, 9), (9, 1), (3, 5), (4, 1), (8, 2)])
def test_degenerate_shapes_bitwise(gpu_lib, nx, ny):
    """The periodic self-neighbour, the tail path and the lane-63 / row-end direct loads."""
    p, obst, cells0, phi0 = _problem(nx, ny, 5 + nx + 10 * ny, obstacles=0.2 if nx * ny > 4 else 0.0)
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, [(1, 1), (nx, ny)], (nx, ny), chunks=(3, 2))


# -------------------------------------------------------- 2. larger bins ----

@pytest.mark.parametrize("nx,ny", GRIDS)
def test_larger_bins_within_the_fold_bound(gpu_lib, nx, ny):
    p, obst, cells0, phi0 = _problem(nx, ny, 7 * nx + ny)
    bins = [(nx, 1), (1, ny), (nx, ny), (5, 3), (4, 4), (7, 2)]
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, bins, (nx, ny), chunks=(3, 2))


def test_a_row_of_two_waves(gpu_lib):
    """nx = 300: a row spans two waves, so the cross-lane move meets a wave border; ny = 5."""
    p, obst, cells0, phi0 = _problem(300, 5, 11)
    with gpu_lib.Engine(p, obst) as e:
        _sequence(e, p, obst, cells0, phi0, [(1, 1), (300, 5), (300, 1), (7, 2)], "300x5", chunks=(2, 1))


# ----------------------------------- 3. every flow kernel, both numerics ----

@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_every_kernel(gpu_lib, mode):
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
        _sequence(e, p, obst, cells0, phi0, [(1, 1), (5, 3)], mode)
        assert e.kernel_in_use() in want
        assert e.numerics() == ("tolerance" if mode == "stream_tolerance" else "bitwise")


# ------------------------------------------------------ 4. decomposed ----

@pytest.fixture(scope="module")
def single(gpu_lib):
    """{grid: (p, obst, cells0, phi0, one-cell sums of the single-domain handle after the sequence)}:
    the reference of the decomposed cases, computed once and left unchanged."""
    out = {}
    for nx, ny in GRIDS:
        p, obst, cells0, phi0 = _problem(nx, ny, 31 + nx)
        with gpu_lib.Engine(p, obst, parts=1) as e:
            assert len(e.local_rects()) == 1
            _sequence(e, p, obst, cells0, phi0, [(1, 1)], "single")
            ref = e.scalar_binned(1, 1)
        for a in (obst, cells0, phi0) + tuple(ref.values()):
            a.setflags(write=False)
        out[(nx, ny)] = (p, obst, cells0, phi0, ref)
    return out


@pytest.mark.parametrize("grid", [(1, 2), (2, 1), (2, 2)])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_bits_do_not_depend_on_the_decomposition(gpu_lib, single, nx, ny, grid):
    p, obst, cells0, phi0, ref = single[(nx, ny)]
    with gpu_lib.Engine(p, obst, parts=grid[0] * grid[1], grid=grid, devices=[0]) as e:
        rects = e.local_rects()
        assert len(rects) == grid[0] * grid[1]
        _sequence(e, p, obst, cells0, phi0, [(1, 1), (nx, ny), (5, 3), (nx, 1), (1, ny)], (nx, ny, grid))
        got = e.scalar_binned(1, 1)
    for name in ref:
        assert np.array_equal(got[name].view(np.uint64), ref[name].view(np.uint64)), name
    if grid[1] == 2 and nx == 37:
        assert any(r[0] % 4 for r in rects)              # a sub-domain off the 16-B alignment


# --------------------------------------------------- 5. `which` subsets ----

def test_which_subsets(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 3)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        _begin(e, p, obst, cells0, phi0)
        e.run_steps(3, accelerate_first=True)
        e.scalar_advance(2)
        terms = _terms(e, obst)
        full = e.scalar_binned(1, 1)
        for which in (FACES, ("fy",), ("fx",), ("phi", "fy"), ("phiphi",), ("uyphi",), ("uxphi", "fx")):
            got = e.scalar_binned(1, 1, which=which)
            assert set(got) == set(which) | {"fluid"}
            for name in which:                                   # equal to the same fields of the full call
                assert np.array_equal(got[name].view(np.uint64), full[name].view(np.uint64)), (which, name)
            for bins in ((5, 3), (37, 1), (37, 19)):
                xc.check_binned(e.scalar_binned(*bins, which=which), terms, obst, bins, (which, bins))
        with pytest.raises(ValueError):
            e.scalar_binned(1, 1, which=("fz",))
        with pytest.raises(ValueError):
            e.scalar_binned(1, 1, 1)
        # every entry NULL: OK, and nothing is launched
        launches = lambda: sum(k["launches"] for k in e.profile_summary())          # noqa: E731
        before = launches()
        none = (ctypes.POINTER(ctypes.c_double) * 6)()
        assert e._L.lbm_scalar_store_binned(e._h, 2, 2, none) == n.LBM_OK and launches() == before
        assert e._L.lbm_scalar_store_binned(e._h, 2, 2, None) == n.LBM_OK and launches() == before


# ------------------------------------------------------------ 6. purity ----

def test_calls_change_nothing(gpu_lib):
    p, obst, cells0, phi0 = _problem(64, 32, 21)

    def run(with_calls):
        with gpu_lib.Engine(p, obst) as e:
            _begin(e, p, obst, cells0, phi0)
            e.run_steps(3, accelerate_first=True)
            e.scalar_advance(2)
            if with_calls:
                cells, g = e.store(n_av=0)[0], e.scalar(populations=True)[1]
                a, b = e.scalar_binned(5, 3), e.scalar_binned(5, 3)
                for name in a:                                   # two calls: identical bits
                    assert np.array_equal(a[name].view(np.uint64), b[name].view(np.uint64)), name
                e.scalar_binned(1, 1, which=FACES)
                e.scalar_profile(1)
                assert _same(e.store(n_av=0)[0], cells) and _same(e.scalar(populations=True)[1], g)
                assert e.scalar_steps == 2
            e.run_steps(4)
            e.scalar_advance(3)
            return e.store(n_av=0)[0], e.scalar(populations=True)[1]

    (cells_a, g_a), (cells_b, g_b) = run(True), run(False)
    assert _same(cells_a, cells_b) and _same(g_a, g_b)


# ---------------------------------------------------------- 7. contract ----

def test_contract_and_profile_classes(gpu_lib):
    n = gpu_lib
    p, obst, cells0, phi0 = _problem(37, 19, 9)
    f64p = ctypes.POINTER(ctypes.c_double)
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        L, h = e._L, e._h
        out = np.full((6, p.ny, p.nx), 7.0)
        table = (f64p * 6)(*[out[f].ctypes.data_as(f64p) for f in range(6)])
        call = lambda bw=1, bh=1: L.lbm_scalar_store_binned(h, bw, bh, table)       # noqa: E731
        assert L.lbm_scalar_store_binned(None, 1, 1, table) == n.LBM_E_INVALID
        assert call() == n.LBM_E_STATE                                    # before scalar_begin
        e.scalar_begin(phi0, omega_s=OMEGA_S)
        assert call() == n.LBM_E_STATE                                    # before the lattice is loaded
        e.load_cells(cells0)
        for bw, bh in ((0, 1), (1, 0), (-1, 1), (p.nx + 1, 1), (1, p.ny + 1)):
            assert call(bw, bh) == n.LBM_E_INVALID, (bw, bh)
        assert (out == 7).all()
        assert not [k for k in e.profile_summary() if "scalar_binned" in k["name"]]
        assert call() == n.LBM_OK and not (out == 7).any()
        e.scalar_binned(5, 3, which=FACES)
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["scalar_binned"]["launches"] == 2 and prof["scalar_binned fold"]["launches"] == 2
        assert prof["scalar_binned"]["total_ms"] > 0
        e.scalar_end()
        assert call() == n.LBM_E_STATE
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:       # a handle that never calls launches nothing new
        _begin(e, p, obst, cells0, phi0)
        e.run_scalar(4, 1, accelerate_first=True)
        assert not [k for k in e.profile_summary() if "scalar_binned" in k["name"]]


# ------------------------------------------- 8. profiles and histories ----

def test_profile_nusselt_and_history(gpu_lib):
    p, obst, cells0, phi0 = _problem(64, 32, 3)
    with gpu_lib.Engine(p, obst) as e:
        _begin(e, p, obst, cells0, phi0)
        e.run_steps(3, accelerate_first=True)
        e.scalar_advance(2)
        prof = e.scalar_profile(1)
        rows = e.scalar_binned(64, 1)
        assert all(prof[k].shape == (32,) and np.array_equal(prof[k], rows[k].reshape(-1)) for k in rows)
        cols = e.scalar_profile(0, which=("fx",))
        assert cols["fx"].shape == (64,) and np.array_equal(cols["fx"], e.scalar_binned(1, 32)["fx"].reshape(-1))
        d = lio.scalar_diffusivity(np.float32(OMEGA_S), 2)
        nu = e.nusselt(1, 2.0, 30.0)
        assert np.array_equal(nu, lio.nusselt_number(prof["fy"], 64, d, 2.0, 30.0))
        assert np.array_equal(e.nusselt(0, 1.0, 5.0), lio.nusselt_number(cols["fx"], 32, d, 1.0, 5.0))
        with pytest.raises(ValueError):
            e.scalar_profile(2)
    accel = (0.0, 1e-4)
    for kw in (dict(), dict(accel=accel, phi_ref=0.1, stride=2)):
        with gpu_lib.Engine(p, obst) as e:                   # by hand
            _begin(e, p, obst, cells0, phi0)
            want = []
            for n in (5, 5, 3):
                if kw:
                    e.run_thermal(n, accel, 0.1, 2)
                else:
                    e.run_scalar(n, 1)
                want.append(e.scalar_binned(8, 4, which=("phi", "uyphi", "fy")))
        with gpu_lib.Engine(p, obst) as e:
            _begin(e, p, obst, cells0, phi0)
            hist = e.transport_history(13, 5, 8, 4, which=("phi", "uyphi", "fy"), **kw)
            assert hist["step"].tolist() == [5, 10, 13] and e.scalar_steps == 13
            assert set(hist) == {"phi", "uyphi", "fy", "step", "fluid"} and hist["fy"].shape == (3, 8, 8)
            for i, w in enumerate(want):
                assert all(np.array_equal(hist[k][i].view(np.uint64), w[k].view(np.uint64)) for k in ("phi", "uyphi", "fy"))
            assert np.array_equal(hist["fluid"], want[0]["fluid"])
            with pytest.raises(ValueError):
                e.transport_history(5, 0, 8, 4)


# ---------------------------------------------------- 9. device physics ----

def test_rayleigh_benard_heat_flux_on_the_device(gpu_lib):
    """nusselt(1, 1.0, 19.0) after run_thermal(6000, stride 1) on rayleigh_benard(3000): flat over the planes
    y = 1 .. 19 within the bound of the CPU test, and the plane mean within 1e-3 of the CPU loop's 1.88762."""
    p, obst, cells0, phi0, fixed, s = tc.rayleigh_benard(3000)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.scalar_begin(phi0, omega_s=tc.RB_OMEGA)
        e.scalar_fix(*fixed)
        e.run_thermal(xc.RB_STEPS, s, stride=1)
        nu = e.nusselt(1, 1.0, 19.0)
        conv = e.scalar_profile(1, which=("uyphi",))["uyphi"] / xc.rb_unit()
    planes = nu[1:20]
    mean = planes.mean()
    spread = (planes.max() - planes.min()) / mean
    print(f"device, Ra 3000: planes [{planes.min():.6f}, {planes.max():.6f}] mean {mean:.6f} spread {spread:.2e}; "
          f"CPU loop {xc.RB_NU_CPU}; difference {abs(mean / xc.RB_NU_CPU - 1):.2e}; convective {conv[10:12].tolist()}")
    assert nu.shape == (p.ny,)
    assert spread <= xc.RB_FLAT
    assert abs(mean / xc.RB_NU_CPU - 1) <= 1e-3
    assert (0 < conv[10:12]).all() and (conv[10:12] < planes[9:11].min()).all()
