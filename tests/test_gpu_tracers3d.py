"""Lagrangian tracers and point probes on the device, D3Q19 (lbm3d_tracer_*;
include/lbm_tracers_hip.h, csrc/lbm3d_tracers.hip, csrc/lbm_tracers.hpp).

Bar: after every advance the positions are BITWISE (uint64 patterns)
lio.tracer_advance3d of the same handle's fields() at the moment of the call,
the blocked flags lio.tracer_blocked3d, and tracer_sample lio.tracer_interp3d of
those fields, for both schemes and both numerics; a handle of two z slabs gives
the single-slab handle's positions.  No tolerance anywhere.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest

from lbm_amd import io as lio
from oracle import oracle
from tracer_util import N, SENTINEL64, _b64, _same, seeds

pytestmark = pytest.mark.gpu

ALL = ("ux", "uy", "uz", "pressure")
CHUNKS = (3, 1, 4, 2, 5)      # odd and even: both lattices of the pair get read
GRIDS = [(13, 9, 7), (16, 12, 8)]
SCHEMES = ["euler", "heun"]


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _problem(nx, ny, nz, seed):
    """The channel walls plus about 10 % random obstacles; populations perturbed by 5 %."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.85)
    rng = np.random.default_rng(seed)
    obst = lio.channel_obstacles3d(nx, ny, nz) | (rng.random((nz, ny, nx)) < 0.1).astype(np.uint8)
    obst[nz // 2, ny // 2, nx // 2] = 0
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    for a in (obst, c0):
        a.setflags(write=False)
    return p, obst, c0


def _seeds(p, seed=5):
    """The shared edge cases, and points on and next to the border of two z slabs (z = nz / 2)."""
    x, y, z = seeds(np.random.default_rng(seed), (p.nx, p.ny, p.nz))
    k = 100
    for off in (0.0, -1.0, -0.5, -1e-3, -1e-9, 1e-9, 1e-3, 0.5, -0.02, 0.02, -0.1, 0.1):
        z[k], k = p.nz // 2 + off, k + 1
        z[k], y[k], k = p.nz // 2 + off, 1.0 + abs(off), k + 1
    return x, y, z


def _advance_and_check(e, obst, pos, n, scheme, what=""):
    if n:
        e.run_steps(n)
    f = e.fields(ALL)
    pos = lio.tracer_advance3d(f["ux"], f["uy"], f["uz"], *pos, float(n), scheme)
    e.tracers_advance(n, scheme)
    t = e.tracers()
    assert tuple(t) == ("x", "y", "z", "blocked")
    for c, want in zip("xyz", pos):
        bad = _b64(t[c]) != _b64(want)
        assert not bad.any(), (what, n, c, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert np.array_equal(t["blocked"], lio.tracer_blocked3d(obst, *pos)), (what, n)
    s = e.tracer_sample()
    assert tuple(s) == ALL
    for name in ALL:
        bad = _b64(s[name]) != _b64(lio.tracer_interp3d(f[name], *pos))
        assert not bad.any(), (what, n, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return pos


def _sequence(e, p, obst, c0, scheme, what=""):
    e.load_cells(c0)
    pos = _seeds(p)
    e.tracers_begin(*pos)
    assert e.tracer_count == N
    for n in CHUNKS:
        pos = _advance_and_check(e, obst, pos, n, scheme, what)
    for c, ext in zip(pos, (p.nx, p.ny, p.nz)):
        assert (c >= 0).all() and (c < ext).all()
    return pos


@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_sample_at_cell_centres_is_fields(gpu_lib, nx, ny, nz):
    p, obst, c0 = _problem(nx, ny, nz, 3)
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    centres = [a.ravel().astype(np.float64) for a in (xx, yy, zz)]
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.tracers_begin(*centres)
        for steps in (0, 3, 1):
            if steps:
                e.run_steps(steps)
            f, s = e.fields(ALL), e.tracer_sample()
            for name in ALL:
                assert _same(s[name], f[name].astype(np.float64).ravel()), (name, steps)
        t = e.tracers()
    assert np.array_equal(t["blocked"], obst.ravel()) and _same(t["z"], centres[2])
    ob = obst.ravel() != 0
    assert ob.any() and not any(_b64(s[c])[ob].any() for c in ("ux", "uy", "uz"))
    third = np.float32(p.density) * np.float32(np.float32(1) / np.float32(3))
    assert (_b64(s["pressure"])[ob] == _b64(np.float64(third))).all()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("form", ["bitwise", "tolerance"])
@pytest.mark.parametrize("nx,ny,nz", GRIDS)
def test_advance_sequences_bitwise(gpu_lib, nx, ny, nz, form, scheme):
    p, obst, c0 = _problem(nx, ny, nz, 7)
    x0 = _seeds(p)[0]
    kw = dict(devices=[0], flags=gpu_lib.FLAG_TOLERANCE if form == "tolerance" else 0)
    with gpu_lib.Engine3D(p, obst, **kw) as e:
        pos = _sequence(e, p, obst, c0, scheme, (nx, ny, nz, form, scheme))
    assert (np.abs(pos[0] - x0) > 1e-4).sum() > N // 2       # the points moved


@pytest.fixture(scope="module")
def single_16x12x8(gpu_lib):
    """(p, obst, c0, {scheme: positions}) of the single-slab handle: the reference of the slab
    case, computed once and left unchanged."""
    p, obst, c0 = _problem(16, 12, 8, 11)
    out = {}
    for scheme in SCHEMES:
        with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
            assert len(e.local_slabs()) == 1
            out[scheme] = _sequence(e, p, obst, c0, scheme, "single")
    # a Heun midpoint of the first advance lies in the other slab than its point
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(CHUNKS[0])
        f = e.fields(("uz",))
    x, y, z = _seeds(p)
    mz = lio.tracer_wrap(z + float(CHUNKS[0]) * lio.tracer_interp3d(f["uz"], x, y, z), p.nz)
    assert ((z < 4) != (mz < 4)).any()
    for c in out["euler"] + out["heun"]:
        c.setflags(write=False)
    return p, obst, c0, out


@pytest.mark.parametrize("scheme", SCHEMES)
def test_positions_do_not_depend_on_the_slabs(gpu_lib, single_16x12x8, scheme):
    p, obst, c0, ref = single_16x12x8
    with gpu_lib.Engine3D(p, obst, parts=2, devices=[0]) as e:
        assert e.local_slabs() == [(0, 4), (4, 4)]
        pos = _sequence(e, p, obst, c0, scheme, ("slabs", scheme))
    for got, want in zip(pos, ref[scheme]):
        assert _same(got, want)


def test_tracers_touch_no_engine_state(gpu_lib):
    p, obst, c0 = _problem(16, 12, 8, 21)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.tracers_begin(*_seeds(p))
        e.run_steps(7)
        e.tracers_advance(7, "heun")
        e.tracer_sample()
        e.tracers()
        e.run_steps(6)
        cells_a, _ = e.store()
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.run_steps(13)
        cells, _ = e.store()
    assert np.array_equal(_b32(cells_a), _b32(cells))


def test_run_traced_and_probe_history(gpu_lib):
    p, obst, c0 = _problem(13, 9, 7, 5)
    pos0 = _seeds(p)
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        pos, fields = pos0, []
        for n in (5, 5, 3):
            e.run_steps(n)
            fields.append(e.fields(ALL))
            pos = lio.tracer_advance3d(fields[-1]["ux"], fields[-1]["uy"], fields[-1]["uz"], *pos, float(n), "euler")
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.tracers_begin(*pos0)
        dts, advance = [], e.tracers_advance
        e.tracers_advance = lambda dt, scheme="heun": (dts.append(dt), advance(dt, scheme))[1]
        av = e.run_traced(13, 5, scheme="euler")
        assert dts == [5, 5, 3] and av.size == 0
        t = e.tracers()
        with pytest.raises(ValueError):
            e.run_traced(5, 5, accelerate_first=True)
    for c, want in zip("xyz", pos):
        assert _same(t[c], want), c
    with gpu_lib.Engine3D(p, obst, devices=[0]) as e:
        e.load_cells(c0)
        e.tracers_begin(*pos0)
        hist = e.probe_history(13, 5, which=("uz",))
        t = e.tracers()
    assert all(_same(t[c], w) for c, w in zip("xyz", pos0))
    assert hist["step"].tolist() == [5, 10, 13] and hist["uz"].shape == (3, N)
    for k in range(3):
        assert _same(hist["uz"][k], lio.tracer_interp3d(fields[k]["uz"], *pos0)), k


def test_tracer_contract(gpu_lib):
    n = gpu_lib
    p, obst, c0 = _problem(13, 9, 7, 9)
    x, y, z = _seeds(p)
    f64p, u8p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint8)
    ptr = lambda a: a.ctypes.data_as(f64p)
    with n.Engine3D(p, obst, devices=[0]) as e:
        L, h = e._L, e._h
        out = [np.full(N, SENTINEL64, np.uint64).view(np.float64) for _ in range(4)]
        untouched = lambda: all((_b64(a) == SENTINEL64).all() for a in out)
        cnt = ctypes.c_int64(-1)
        assert L.lbm3d_tracer_count(h, ctypes.byref(cnt)) == n.LBM_OK and cnt.value == 0
        assert L.lbm3d_tracer_advance(h, 1.0, n.TRACER_HEUN) == n.LBM_E_STATE
        assert L.lbm3d_tracer_sample(h, *[ptr(a) for a in out]) == n.LBM_E_STATE
        assert L.lbm3d_tracer_store(h, ptr(out[0]), None, None, None) == n.LBM_E_STATE
        assert L.lbm3d_tracer_end(h) == n.LBM_OK
        for bad in (float(p.nz), -1e-9, np.nan, np.inf):
            zb = z.copy()
            zb[N - 1] = bad
            assert L.lbm3d_tracer_begin(h, N, ptr(x), ptr(y), ptr(zb)) == n.LBM_E_INVALID, bad
        assert L.lbm3d_tracer_begin(h, N, ptr(x), ptr(y), None) == n.LBM_E_INVALID
        assert e.tracer_count == 0
        e.tracers_begin(x, y, z)
        assert L.lbm3d_tracer_advance(h, 1.0, n.TRACER_EULER) == n.LBM_E_STATE      # no lattice yet
        assert L.lbm3d_tracer_sample(h, ptr(out[0]), None, None, None) == n.LBM_E_STATE and untouched()
        e.load_cells(c0)
        e.run_steps(2)
        for dt, scheme in ((np.nan, 0), (np.inf, 1), (1.0, 2)):
            assert L.lbm3d_tracer_advance(h, dt, scheme) == n.LBM_E_INVALID
        assert L.lbm3d_tracer_sample(h, None, None, None, None) == n.LBM_OK and untouched()
        f = e.fields(ALL)
        assert L.lbm3d_tracer_sample(h, None, None, ptr(out[2]), None) == n.LBM_OK
        assert _same(out[2], lio.tracer_interp3d(f["uz"], x, y, z))
        _b64(out[2])[...] = SENTINEL64
        assert untouched()
        e.tracers_advance(2, "heun")
        moved = e.tracers()
        zb = z.copy()
        zb[3] = np.nan
        assert L.lbm3d_tracer_begin(h, N, ptr(x), ptr(y), ptr(zb)) == n.LBM_E_INVALID
        kept = e.tracers()
        assert e.tracer_count == N and all(_same(kept[c], moved[c]) for c in "xyz") and not _same(moved["x"], x)
        e.tracers_begin(x[:7], y[:7], z[:7])
        assert e.tracer_count == 7 and _same(e.tracers()["z"], z[:7])
        with pytest.raises(ValueError):
            e.tracers_begin(x, y)
        e.tracers_end()
        assert e.tracer_count == 0 and L.lbm3d_tracer_advance(h, 1.0, 0) == n.LBM_E_STATE
        e.tracers_begin(x, y, z)       # the handle is destroyed with a set: lbm3d_destroy frees it
