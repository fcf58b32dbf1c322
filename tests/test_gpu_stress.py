"""Strain rate and wall shear from the non-equilibrium moments on the device, D2Q9
(lbm_store_stress / lbm_stress_stats; include/lbm_stress_hip.h, csrc/lbm_stress.hip).

Bar: every field is BITWISE (uint32 patterns) lio.neq_strain of the same
handle's store() cells -- the numpy restatement of the header's definition,
pinned by arithmetic in tests/test_stress_host.py -- for the shapes around the
kernel's work units (a lane's quad of 4 cells, a block's 2048 consecutive
quads), every step kernel, both lattice layouts, both sides of the ping-pong
pair and decomposed handles.  The maxima and the near-wall count are exact; the
fp64 sums lie within 2 (n - 1) 2^-53 of math.fsum over their n terms (the bound
of any order of summing n non-negative terms) and repeat bit for bit.
"""
from __future__ import annotations

import ctypes
import struct
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

SENTINEL32 = 0x7FC00001       # a quiet NaN pattern no computation produces
QUAD, BLOCK_QUADS = 4, 2048   # native.STRESS_QUAD / STRESS_BLOCK_QUADS (asserted below)
OMEGA, DENSITY = 1.85, 0.1


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _d64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _perturbed(p, seed):
    rng = np.random.default_rng(seed)
    return (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((p.ny, p.nx, 9)))).astype(np.float32)


def _obstacles(nx, ny, seed, borders=()):
    """About 10 % random obstacles, plus blocked cells on the domain's edge rows and
    columns, on both sides of every block border of the kernel (the last cell of quad
    2048 k - 1 and the first of quad 2048 k, row-major over ceil(nx / 4) quads per row),
    and on the given sub-domain borders (("x", i) / ("y", j)); one cell kept fluid."""
    rng = np.random.default_rng(seed)
    obst = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    for x in (0, nx - 2, nx - 1):
        if x >= 0:
            obst[0, x] = 1
            obst[ny - 1, x] = 1
    obst[ny // 2, 0] = obst[ny // 2, nx - 1] = 1
    qpr = (nx + QUAD - 1) // QUAD
    for q in range(BLOCK_QUADS, qpr * ny, BLOCK_QUADS):
        obst[q // qpr, (q % qpr) * QUAD] = 1
        obst[(q - 1) // qpr, min(((q - 1) % qpr) * QUAD + QUAD, nx) - 1] = 1
    for axis, i in borders:
        if axis == "x":
            obst[ny // 4, i - 1] = obst[ny // 4 + 1, i] = 1
        else:
            obst[i - 1, nx // 4] = obst[i, nx // 4 + 1] = 1
    obst[min(ny - 1, 2), min(nx - 1, 2)] = 0
    return obst


def _problem(nx, ny, seed, iters=8, borders=()):
    p = lio.Params(nx, ny, iters, 10, DENSITY, 0.005, OMEGA)
    return p, _obstacles(nx, ny, seed, borders), _perturbed(p, seed + 1)


def _reference(e, p, obst):
    cells, _ = e.store(n_av=0)
    return lio.neq_strain(np.asarray(cells).reshape(p.ny, p.nx, 9), obst, p.omega)


def _assert_fields(got, ref, names, what=""):
    for name in names:
        assert got[name].dtype == np.float32 and got[name].shape == ref[name].shape
        bad = _b32(got[name]) != _b32(ref[name])
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _assert_stats(stats, ref, obst, what=""):
    s2, ms, nw, sw, mw = stats
    near = lio.near_wall(obst)
    rs2, rms, rnw, rsw, rmw = lio.strain_stats(ref, obst, near)
    n = int((np.asarray(obst) == 0).sum())
    assert nw == rnw == int(near.sum()), (what, nw, rnw)
    assert _b32(np.float32(ms)) == _b32(rms) and _b32(np.float32(mw)) == _b32(rmw), (what, ms, rms, mw, rmw)
    print(what, "sum_s2", s2, rs2, "sum_wall_strain", sw, rsw, "cells", n, "near-wall", nw)
    assert abs(s2 - rs2) <= 2 * max(n - 1, 0) * 2.0 ** -53 * rs2, (what, s2, rs2)
    assert abs(sw - rsw) <= 2 * max(nw - 1, 0) * 2.0 ** -53 * rsw, (what, sw, rsw)


def _same_stats(a, b):
    return [_d64(a[0]), a[1], a[2], _d64(a[3]), a[4]] == [_d64(b[0]), b[1], b[2], _d64(b[3]), b[4]]


def _check(e, p, obst, what=""):
    """strain_rate() and strain_stats() of the handle against the restatement of its store()."""
    ref = _reference(e, p, obst)
    got = e.strain_rate()
    assert tuple(got) == e._STRESS_FIELDS
    _assert_fields(got, ref, e._STRESS_FIELDS, what)
    stats = e.strain_stats()
    _assert_stats(stats, ref, obst, what)
    assert _same_stats(stats, e.strain_stats()), what
    ob = np.asarray(obst) != 0
    for name in e._STRESS_FIELDS:
        assert not _b32(got[name])[ob].any(), (what, name)      # obstacle cells: +0
    return got, stats


# ------------------------------------------------------------ 1. shapes ----

# below, at and above a quad (widths 3, 4, 5) and a block of 2048 quads: one row of 2047, 2048 and
# 2049 quads, 16 quads per row (the last ragged) over 128 and 129 rows; (131, 67) is 33 x 67 = 2211 quads
SHAPES = [(1, 1), (1, 8), (8, 1), (2, 3), (3, 5), (131, 67), (132, 70),
          (4, 3), (5, 3), (QUAD * BLOCK_QUADS - 4, 1), (QUAD * BLOCK_QUADS, 1), (QUAD * BLOCK_QUADS + 4, 1),
          (62, 127), (62, 128), (62, 129)]


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_strain_shapes_bitwise(gpu_lib, nx, ny):
    assert (gpu_lib.STRESS_QUAD, gpu_lib.STRESS_BLOCK_QUADS) == (QUAD, BLOCK_QUADS)
    p, obst, cells = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        _check(e, p, obst, (nx, ny, "loaded"))
        e.run_steps(3, accelerate_first=True)      # an odd ...
        got, _ = _check(e, p, obst, (nx, ny, 3))
        e.run_steps(1)                             # ... and an even number of steps: both sides of the pair
        _check(e, p, obst, (nx, ny, 4))
        one = e.strain_rate(("sxy",))
        assert tuple(one) == ("sxy",)
        with pytest.raises(ValueError):
            e.strain_rate(("speed",))
    assert got["strain"].any() and got["sxy"].any()


# ----------------------------------------------- 2. every step kernel ----

@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_strain_every_kernel_bitwise(gpu_lib, mode):
    n = gpu_lib
    kw, want = {
        "auto": (dict(), ("resident", "step2")),
        "stream": (dict(kernel=n.KERNEL_STREAM), ("stream",)),
        "stream_tolerance": (dict(kernel=n.KERNEL_STREAM, flags=n.FLAG_TOLERANCE), ("stream",)),
        "step2": (dict(kernel=n.KERNEL_STEP2), ("step2",)),
        "scalar": (dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP), ("scalar",)),
        "pipeline": (dict(kernel=n.KERNEL_PIPELINE), ("pipeline",)),
    }[mode]
    p, obst, cells0 = _problem(132, 70, 7)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        for i, steps in enumerate((3, 1, 4, 5)):       # odd and even launch counts, remainders included
            e.run_steps(steps, accelerate_first=i == 0)
            _check(e, p, obst, (mode, steps))          # tolerance mode too: the handle's own stored cells
        assert e.kernel_in_use() in want
        if mode == "stream_tolerance":
            assert e.numerics() == "tolerance"


@pytest.mark.parametrize("nx,ny", [(132, 70), (131, 67)])
@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_strain_planar_layout_bitwise(gpu_lib, debug_knobs, monkeypatch, nx, ny, kernel):
    """The planar lattice layout (LBM_LAYOUT=planar, a debug knob)."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    p, obst, cells0 = _problem(nx, ny, 13)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        e.run_steps(3, accelerate_first=True)
        _check(e, p, obst, ("planar", nx, ny, 3))
        e.run_steps(2)
        _check(e, p, obst, ("planar", nx, ny, 5))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------------ 3. decomposed ----

# obstacles on the borders of the 2 x 2 and 1 x 2 partitions of 96 x 80: near-wall cells whose
# blocked neighbour lies in another sub-domain, or across the periodic edge of the domain
BORDERS = (("x", 48), ("y", 40), ("x", 95), ("y", 79))


@pytest.fixture(scope="module")
def single_96x80(gpu_lib):
    """(p, obst, cells0, strain_rate, stats) of the single-domain handle after 5 steps: the
    reference of the decomposed cases, computed once and left unchanged."""
    p, obst, cells0 = _problem(96, 80, 31, borders=BORDERS)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        got, stats = _check(e, p, obst, "single")
    for a in list(got.values()) + [cells0, obst]:
        a.setflags(write=False)
    return p, obst, cells0, got, stats


def _decomposed_kw(native, how):
    if how == "local4":
        return dict(parts=4, grid=(2, 2), devices=[0])
    if how == "local2":
        return dict(parts=2, grid=(1, 2), devices=[0])
    return dict(parts=1, grid=(1, 1), devices=[0], flags=native.FLAG_FORCE_EXCHANGE,
                transport=native.TRANSPORT_RCCL, rank=0, world=1, unique_id=native.rccl_unique_id())


@pytest.mark.parametrize("how", ["local4", "local2", "rccl1"])
def test_strain_decomposed_bitwise(gpu_lib, single_96x80, how):
    p, obst, cells0, ref, ref_stats = single_96x80
    near = lio.near_wall(obst)
    # the case holds near-wall cells whose only blocked neighbours lie in another quarter of the 2 x 2
    # partition, or across the periodic edge: a quarter's own cells alone (zero-padded) miss them
    missed = 0
    for y0, x0 in ((0, 0), (0, 48), (40, 0), (40, 48)):
        inside = lio.near_wall(np.pad(obst[y0:y0 + 40, x0:x0 + 48], 1))[1:-1, 1:-1]
        missed += int((near[y0:y0 + 40, x0:x0 + 48] & ~inside).sum())
    assert missed > 4
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        got = e.strain_rate()
        local = e.strain_rate_local()
        rects = e.local_rects()
        stats = e.strain_stats()
        assert _same_stats(stats, e.strain_stats())
        assert len(rects) == {"local4": 4, "local2": 2, "rccl1": 1}[how]
    _assert_fields(got, ref, gpu_lib.STRESS_FIELDS, how)
    for (x0, y0, w, h), blk in zip(rects, local):
        for name in gpu_lib.STRESS_FIELDS:
            assert blk[name].shape == (h, w)
            assert np.array_equal(_b32(blk[name]), _b32(ref[name][y0:y0 + h, x0:x0 + w])), (how, name, x0, y0)
    assert stats[2] == int(near.sum()) == ref_stats[2]
    assert stats[1] == ref_stats[1] and stats[4] == ref_stats[4]
    n = int((obst == 0).sum())
    assert abs(stats[0] - ref_stats[0]) <= 2 * (n - 1) * 2.0 ** -53 * ref_stats[0], (how, stats, ref_stats)
    assert abs(stats[3] - ref_stats[3]) <= 2 * (stats[2] - 1) * 2.0 ** -53 * ref_stats[3], (how, stats, ref_stats)


# -------------------------------------------- 4. no engine state touched ----

@pytest.mark.parametrize("how", ["single", "local4"])
def test_strain_touches_no_engine_state(gpu_lib, how):
    """7 steps, strain_rate() and strain_stats(), 6 steps: the lattice and av_vels equal
    those of the same 7 + 6 run without the calls, and the lattice one 13-step run's."""
    p, obst, cells0 = _problem(132, 70, 21, iters=13)
    kw = {} if how == "single" else _decomposed_kw(gpu_lib, how)
    with gpu_lib.Engine(p, obst, **kw) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        cells, _ = e.store(n_av=13)

    def chunked(with_calls):
        with gpu_lib.Engine(p, obst, **kw) as e:
            e.load_cells(cells0)
            e.run_steps(7, accelerate_first=True)
            av7 = e.store(cells=False, n_av=7)[1].copy()
            if with_calls:
                e.strain_rate()
                e.strain_stats()
            e.run_steps(6)
            got_cells, av6 = e.store(n_av=6)
            return got_cells, np.concatenate([av7, av6])

    got_cells, got_av = chunked(True)
    plain_cells, plain_av = chunked(False)
    assert np.array_equal(_b32(got_cells), _b32(cells))
    assert np.array_equal(_b32(got_cells), _b32(plain_cells)) and np.array_equal(_b32(got_av), _b32(plain_av))


def test_strain_leaves_the_averages_alone(gpu_lib):
    p, obst, cells0 = _problem(131, 67, 23)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin()
        e.run_steps(4, accelerate_first=True)
        e.avg_sample()
        before = e.avg_sums()
        e.strain_rate()
        e.strain_stats()
        after = e.avg_sums()
        assert e.avg_samples == 1
    for name in gpu_lib.AVG_FIELDS:
        assert np.array_equal(before[name].view(np.uint64), after[name].view(np.uint64)), name


# ---------------------------------------------------------- 5. contract ----

def _ptrs(n, arrays):
    out = (ctypes.POINTER(ctypes.c_float) * n)()
    for i, a in arrays.items():
        out[i] = a.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    return out


def _stat_refs():
    v = (ctypes.c_double(-1), ctypes.c_float(-1), ctypes.c_int64(-1), ctypes.c_double(-1), ctypes.c_float(-1))
    return v, [ctypes.byref(x) for x in v]


def test_strain_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells = _problem(131, 67, 9)
    nf = len(n.STRESS_FIELDS)
    classes = ("neq_strain", "neq_strain stats")
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        L, h = e._L, e._h
        out = {i: np.full((p.ny, p.nx), SENTINEL32, np.uint32).view(np.float32) for i in range(nf)}
        vals, refs = _stat_refs()
        # before load
        assert L.lbm_store_stress(h, _ptrs(nf, out)) == n.LBM_E_STATE
        assert L.lbm_store_stress_local(h, _ptrs(nf, out)) == n.LBM_E_STATE
        assert L.lbm_stress_stats(h, *refs) == n.LBM_E_STATE
        assert all((_b32(a) == SENTINEL32).all() for a in out.values()) and all(v.value == -1 for v in vals)
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.fields()
        # every output NULL: LBM_OK and no launch
        assert L.lbm_store_stress(h, _ptrs(nf, {})) == n.LBM_OK
        assert L.lbm_store_stress_local(h, _ptrs(nf, {})) == n.LBM_OK
        assert L.lbm_store_stress(h, None) == n.LBM_OK
        assert L.lbm_stress_stats(h, None, None, None, None, None) == n.LBM_OK
        names = [k["name"] for k in e.profile_summary()]
        assert names and not [k for k in names if k in classes]
        # a selection writes only the entries given
        ref = _reference(e, p, obst)
        assert L.lbm_store_stress(h, _ptrs(nf, {1: out[1]})) == n.LBM_OK
        assert np.array_equal(_b32(out[1]), _b32(ref["sxy"]))
        assert all((_b32(out[i]) == SENTINEL32).all() for i in (0, 2, 3))
        assert L.lbm_stress_stats(h, None, refs[1], None, None, None) == n.LBM_OK
        assert _b32(np.float32(vals[1].value)) == _b32(ref["strain"].max())
        assert all(vals[i].value == -1 for i in (0, 2, 3, 4))
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["neq_strain"]["launches"] == 1 and prof["neq_strain"]["total_ms"] > 0
        assert prof["neq_strain stats"]["launches"] == 1


def test_strain_refuses_omega_one(gpu_lib):
    """At omega = 1 the post-collision lattice is the equilibrium: all three calls answer
    LBM_E_INVALID with a text that names omega, and the handle runs and stores as ever."""
    n = gpu_lib
    nx, ny = 33, 17
    p = lio.Params(nx, ny, 8, 10, DENSITY, 0.005, 1.0)
    obst, cells0 = _obstacles(nx, ny, 5), _perturbed(p, 6)
    nf = len(n.STRESS_FIELDS)
    with n.Engine(p, obst) as e:
        L, h = e._L, e._h
        e.load_cells(cells0)
        e.run_steps(3, accelerate_first=True)
        before, _ = e.store(n_av=0)
        before = before.copy()
        out = {i: np.full((ny, nx), SENTINEL32, np.uint32).view(np.float32) for i in range(nf)}
        vals, refs = _stat_refs()
        for call in (lambda: L.lbm_store_stress(h, _ptrs(nf, out)),
                     lambda: L.lbm_store_stress_local(h, _ptrs(nf, out)),
                     lambda: L.lbm_stress_stats(h, *refs)):
            assert call() == n.LBM_E_INVALID
            assert b"omega" in L.lbm_last_error(h)
        assert all((_b32(a) == SENTINEL32).all() for a in out.values()) and all(v.value == -1 for v in vals)
        with pytest.raises(n.LbmError, match="omega"):
            e.strain_rate()
        after, _ = e.store(n_av=0)
        assert np.array_equal(_b32(before), _b32(after))
        e.run_steps(2)
        assert np.isfinite(e.store(n_av=0)[0]).all()
        assert e.fields()["ux"].any()


def test_strain_history(gpu_lib):
    p, obst, cells0 = _problem(132, 70, 3, iters=12)
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(12, accelerate_first=True)
        cells, av = e.store(n_av=12)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        samples, got_av = e.strain_history(12, every=4, accelerate_first=True)
        got_cells, _ = e.store(n_av=0)
        with pytest.raises(ValueError):
            e.strain_history(5, 0)
    assert [s[0] for s in samples] == [4, 8, 12]
    assert got_av.dtype == np.float32 and np.array_equal(_b32(got_av), _b32(av))
    assert np.array_equal(_b32(got_cells), _b32(cells))
    with gpu_lib.Engine(p, obst) as e:      # the same stats taken by hand at those steps
        e.load_cells(cells0)
        for i, s in enumerate(samples):
            e.run_steps(4, accelerate_first=i == 0)
            assert _same_stats(e.strain_stats(), s[1:]), i
    assert samples[-1][1] > 0 and samples[-1][3] == int(lio.near_wall(obst).sum()) and samples[-1][4] > 0


# ------------------------------------------------------------ 6. runner ----

def test_runner_stress(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "50"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    r = subprocess.run([str(exe), "--device", "gpu", "--runs", "0", "--stress", "--params", str(params),
                        "--obstacles", str(obst_file), "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "==done==" in r.stdout
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(lio.init_cells(p))
        e.run_steps(50, accelerate_first=True)
        want = e.strain_rate()
    got = lio.read_stress_state(str(tmp_path / "stress_state.dat"), p.nx, p.ny)
    for name in gpu_lib.STRESS_FIELDS:
        assert np.array_equal(_b32(got[name]), _b32(want[name])), name
    ob = np.asarray(obst).reshape(p.ny, p.nx)
    assert np.array_equal(got["obstacle"], (ob != 0).astype(np.uint8))
    assert np.array_equal(got["near_wall"], lio.near_wall(ob).astype(np.uint8))
    assert want["strain"].any()
