"""Vorticity, divergence, strain rate and Q derived on the device, D2Q9
(lbm_store_gradients / lbm_gradient_stats; include/lbm_gradients_hip.h,
csrc/lbm_gradients.hip).

Bar: every field is BITWISE (uint32 patterns) lio.velocity_gradients of the
same handle's fields() -- the numpy restatement of the header's definition,
pinned by arithmetic in tests/test_gradients_host.py -- for the shapes around
the kernel's strips (248 owned columns) and segments (32 rows), every step
kernel, both lattice layouts, both sides of the ping-pong pair and decomposed
handles.  The maxima are bitwise the fields' maxima; the fp64 sums lie within
2 (n - 1) 2^-53 of math.fsum over the n fluid cells (the bound of any order of
summing n non-negative terms, as tests/test_gpu_fields.py uses for the mass)
and repeat bit for bit.
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

VEL = ("ux", "uy")
SENTINEL32 = 0x7FC00001       # a quiet NaN pattern no computation produces
STRIP, SEG = 248, 32          # native.GRAD_STRIP_COLS / GRAD_SEGMENT_ROWS (asserted below)


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _d64(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def _perturbed(p, seed):
    rng = np.random.default_rng(seed)
    return (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((p.ny, p.nx, 9)))).astype(np.float32)


def _obstacles(nx, ny, seed, borders=()):
    """About 10 % random obstacles, plus blocked cells on the domain's edge rows and
    columns, on both sides of every strip and segment border of the kernel, and on the
    given sub-domain borders (x or y indices as ("x", i) / ("y", j)); one cell kept fluid."""
    rng = np.random.default_rng(seed)
    obst = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    for x in (0, nx - 2, nx - 1):
        if x >= 0:
            obst[0, x] = 1
            obst[ny - 1, x] = 1
    obst[ny // 2, 0] = obst[ny // 2, nx - 1] = 1
    for xb in range(STRIP, nx, STRIP):
        obst[ny // 3, xb - 1] = obst[(2 * ny) // 3, xb] = 1
    for yb in range(SEG, ny, SEG):
        obst[yb - 1, nx // 3] = obst[yb, (2 * nx) // 3] = 1
    for axis, i in borders:
        if axis == "x":
            obst[ny // 4, i - 1] = obst[ny // 4 + 1, i] = 1
        else:
            obst[i - 1, nx // 4] = obst[i, nx // 4 + 1] = 1
    obst[min(ny - 1, 2), min(nx - 1, 2)] = 0
    return obst


def _problem(nx, ny, seed, iters=8, borders=()):
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, 1.85)
    return p, _obstacles(nx, ny, seed, borders), _perturbed(p, seed + 1)


def _reference(e, obst):
    f = e.fields(VEL)
    return lio.velocity_gradients(f["ux"], f["uy"], obst)


def _assert_fields(got, ref, names, what=""):
    for name in names:
        assert got[name].dtype == np.float32 and got[name].shape == ref[name].shape
        bad = _b32(got[name]) != _b32(ref[name])
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _assert_stats(stats, ref, obst, what=""):
    w2, s2, mw, md = stats
    rw2, rs2, rmw, rmd = lio.gradient_stats(ref, obst)
    n = int((np.asarray(obst) == 0).sum())
    assert _b32(np.float32(mw)) == _b32(rmw) and _b32(np.float32(md)) == _b32(rmd), (what, mw, rmw, md, rmd)
    bound = 2 * max(n - 1, 0) * 2.0 ** -53
    print(what, "sum_w2", w2, rw2, "sum_s2", s2, rs2, "bound", bound)
    assert abs(w2 - rw2) <= bound * rw2, (what, w2, rw2)
    assert abs(s2 - rs2) <= bound * rs2, (what, s2, rs2)


def _check(e, obst, what=""):
    """gradients() and gradient_stats() of the handle against the restatement of its fields()."""
    ref = _reference(e, obst)
    got = e.gradients()
    assert tuple(got) == e._GRAD_FIELDS
    _assert_fields(got, ref, e._GRAD_FIELDS, what)
    stats = e.gradient_stats()
    _assert_stats(stats, ref, obst, what)
    again = e.gradient_stats()
    assert [_d64(v) for v in stats[:2]] == [_d64(v) for v in again[:2]] and stats[2:] == again[2:], what
    ob = np.asarray(obst) != 0
    for name in e._GRAD_FIELDS:
        assert not _b32(got[name])[ob].any(), (what, name)      # obstacle cells: +0
    return got, stats


# ------------------------------------------------------------ 1. shapes ----

SHAPES = [(1, 1), (1, 8), (8, 1), (2, 3), (3, 5), (131, 67), (132, 70),
          (STRIP - 1, SEG - 1), (STRIP + 1, SEG + 1), (2 * STRIP - 1, 2 * SEG - 1), (2 * STRIP + 1, 2 * SEG + 1),
          (STRIP, SEG), (4, 2 * SEG)]


@pytest.mark.parametrize("nx,ny", SHAPES)
def test_gradients_shapes_bitwise(gpu_lib, nx, ny):
    assert (gpu_lib.GRAD_STRIP_COLS, gpu_lib.GRAD_SEGMENT_ROWS) == (STRIP, SEG)
    p, obst, cells = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        _check(e, obst, (nx, ny, "loaded"))
        e.run_steps(3, accelerate_first=True)      # an odd ...
        got, _ = _check(e, obst, (nx, ny, 3))
        e.run_steps(1)                             # ... and an even number of steps: both sides of the pair
        _check(e, obst, (nx, ny, 4))
        one = e.gradients(("q",))
        assert tuple(one) == ("q",)
        with pytest.raises(ValueError):
            e.gradients(("speed",))
    if nx > 2 and ny > 2:
        assert got["vorticity"].any() and got["strain"].any()


# ----------------------------------------------- 2. every step kernel ----

@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_gradients_every_kernel_bitwise(gpu_lib, mode):
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
            _check(e, obst, (mode, steps))
        assert e.kernel_in_use() in want
        if mode == "stream_tolerance":
            assert e.numerics() == "tolerance"


@pytest.mark.parametrize("nx,ny", [(132, 70), (131, 67)])
@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_gradients_planar_layout_bitwise(gpu_lib, debug_knobs, monkeypatch, nx, ny, kernel):
    """The planar lattice layout (LBM_LAYOUT=planar, a debug knob)."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    p, obst, cells0 = _problem(nx, ny, 13)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        e.run_steps(3, accelerate_first=True)
        _check(e, obst, ("planar", nx, ny, 3))
        e.run_steps(2)
        _check(e, obst, ("planar", nx, ny, 5))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------------ 3. decomposed ----

# obstacles on the borders of the 2 x 2 and 1 x 2 partitions of 96 x 80
BORDERS = {"plain": (), "on_borders": (("x", 48), ("y", 40), ("x", 95), ("y", 79))}


@pytest.fixture(scope="module", params=sorted(BORDERS))
def single_96x80(gpu_lib, request):
    """(p, obst, cells0, gradients, stats) of the single-domain handle after 5 steps: the
    reference of the decomposed cases, computed once and left unchanged."""
    p, obst, cells0 = _problem(96, 80, 31, borders=BORDERS[request.param])
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        got, stats = _check(e, obst, "single")
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
def test_gradients_decomposed_bitwise(gpu_lib, single_96x80, how):
    p, obst, cells0, ref, ref_stats = single_96x80
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        got = e.gradients()
        local = e.gradients_local()
        rects = e.local_rects()
        stats = e.gradient_stats()
        assert stats == e.gradient_stats()
        assert len(rects) == {"local4": 4, "local2": 2, "rccl1": 1}[how]
    _assert_fields(got, ref, gpu_lib.GRAD_FIELDS, how)
    for (x0, y0, w, h), blk in zip(rects, local):
        for name in gpu_lib.GRAD_FIELDS:
            assert blk[name].shape == (h, w)
            assert np.array_equal(_b32(blk[name]), _b32(ref[name][y0:y0 + h, x0:x0 + w])), (how, name, x0, y0)
    n = int((obst == 0).sum())
    bound = 2 * (n - 1) * 2.0 ** -53
    assert stats[2:] == ref_stats[2:]
    for a, b in zip(stats[:2], ref_stats[:2]):
        assert abs(a - b) <= bound * b, (how, a, b)


# -------------------------------------------- 4. no engine state touched ----

@pytest.mark.parametrize("how", ["single", "local4"])
def test_gradients_touch_no_engine_state(gpu_lib, how):
    """7 steps, gradients() and gradient_stats(), 6 steps: the lattice equals one 13-step
    run's bit for bit, and the lattice and av_vels equal those of the same 7 + 6 run
    without the gradient calls.  Single-domain the av_vels also equal the 13-step run's;
    on the 2 x 2 handle the engine's own chunking moves the last bit of the av_vel of the
    first chunk's last step (measured: the 7 + 6 run without any gradient call differs from
    the 13-step run in av_vels[6] alone, by 2 ulp), so there the unchunked av_vels are no
    reference and the chunked run without gradient calls is."""
    p, obst, cells0 = _problem(132, 70, 21, iters=13)
    kw = {} if how == "single" else _decomposed_kw(gpu_lib, how)
    with gpu_lib.Engine(p, obst, **kw) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        cells, av = e.store(n_av=13)

    def chunked(with_gradients):
        with gpu_lib.Engine(p, obst, **kw) as e:
            e.load_cells(cells0)
            e.run_steps(7, accelerate_first=True)
            av7 = e.store(cells=False, n_av=7)[1].copy()
            if with_gradients:
                e.gradients()
                e.gradient_stats()
            e.run_steps(6)
            got_cells, av6 = e.store(n_av=6)
            return got_cells, np.concatenate([av7, av6])

    got_cells, got_av = chunked(True)
    plain_cells, plain_av = chunked(False)
    assert np.array_equal(_b32(got_cells), _b32(cells))
    assert np.array_equal(_b32(got_cells), _b32(plain_cells)) and np.array_equal(_b32(got_av), _b32(plain_av))
    print(how, "av_vels differing from the 13-step run:", np.nonzero(_b32(got_av) != _b32(av))[0].tolist())
    if how == "single":
        assert np.array_equal(_b32(got_av), _b32(av))


def test_gradients_leave_the_averages_alone(gpu_lib):
    p, obst, cells0 = _problem(131, 67, 23)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin()
        e.run_steps(4, accelerate_first=True)
        e.avg_sample()
        before = e.avg_sums()
        e.gradients()
        e.gradient_stats()
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


def test_gradients_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells = _problem(131, 67, 9)
    nf = len(n.GRAD_FIELDS)
    classes = ("velocity_gradients", "velocity_gradients stats", "edge_velocities")
    with n.Engine(p, obst, flags=n.FLAG_PROFILE) as e:
        L, h = e._L, e._h
        out = {i: np.full((p.ny, p.nx), SENTINEL32, np.uint32).view(np.float32) for i in range(nf)}
        w2, s2, mw, md = ctypes.c_double(-1), ctypes.c_double(-1), ctypes.c_float(-1), ctypes.c_float(-1)
        # before load
        assert L.lbm_store_gradients(h, _ptrs(nf, out)) == n.LBM_E_STATE
        assert L.lbm_store_gradients_local(h, _ptrs(nf, out)) == n.LBM_E_STATE
        assert L.lbm_gradient_stats(h, ctypes.byref(w2), ctypes.byref(s2), ctypes.byref(mw),
                                    ctypes.byref(md)) == n.LBM_E_STATE
        assert all((_b32(a) == SENTINEL32).all() for a in out.values()) and w2.value == -1
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.fields()
        # every output NULL: LBM_OK and no launch
        assert L.lbm_store_gradients(h, _ptrs(nf, {})) == n.LBM_OK
        assert L.lbm_store_gradients_local(h, _ptrs(nf, {})) == n.LBM_OK
        assert L.lbm_store_gradients(h, None) == n.LBM_OK
        assert L.lbm_gradient_stats(h, None, None, None, None) == n.LBM_OK
        names = [k["name"] for k in e.profile_summary()]
        assert names and not [k for k in names if k in classes]
        # a selection writes only the entries given
        ref = _reference(e, obst)
        assert L.lbm_store_gradients(h, _ptrs(nf, {2: out[2]})) == n.LBM_OK
        assert np.array_equal(_b32(out[2]), _b32(ref["strain"]))
        assert all((_b32(out[i]) == SENTINEL32).all() for i in (0, 1, 3))
        assert L.lbm_gradient_stats(h, None, None, ctypes.byref(mw), None) == n.LBM_OK
        assert _b32(np.float32(mw.value)) == _b32(np.abs(ref["vorticity"]).max()) and w2.value == -1
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["velocity_gradients"]["launches"] == 1 and prof["velocity_gradients"]["total_ms"] > 0
        assert prof["velocity_gradients stats"]["launches"] == 1
        assert prof["edge_velocities"]["launches"] == 2


def test_gradient_history(gpu_lib):
    p, obst, cells0 = _problem(132, 70, 3, iters=12)
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(12, accelerate_first=True)
        cells, av = e.store(n_av=12)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        samples, got_av = e.gradient_history(12, every=4, accelerate_first=True)
        got_cells, _ = e.store(n_av=0)
        with pytest.raises(ValueError):
            e.gradient_history(5, 0)
    assert [s[0] for s in samples] == [4, 8, 12]
    assert got_av.dtype == np.float32 and np.array_equal(_b32(got_av), _b32(av))
    assert np.array_equal(_b32(got_cells), _b32(cells))
    with gpu_lib.Engine(p, obst) as e:      # the same stats taken by hand at those steps
        e.load_cells(cells0)
        for i, s in enumerate(samples):
            e.run_steps(4, accelerate_first=i == 0)
            hand = e.gradient_stats()
            assert [_d64(v) for v in hand[:2]] == [_d64(v) for v in s[1:3]] and hand[2:] == s[3:], i
    assert samples[-1][1] > 0 and samples[-1][2] > 0


# ------------------------------------------------------------ 6. runner ----

def test_runner_gradients(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "50"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    r = subprocess.run([str(exe), "--device", "gpu", "--runs", "0", "--gradients", "--params", str(params),
                        "--obstacles", str(obst_file), "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "==done==" in r.stdout
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(lio.init_cells(p))
        e.run_steps(50, accelerate_first=True)
        want = e.gradients()
    got = lio.read_gradient_state(str(tmp_path / "gradient_state.dat"), p.nx, p.ny)
    for name in gpu_lib.GRAD_FIELDS:
        assert np.array_equal(_b32(got[name]), _b32(want[name])), name
    assert np.array_equal(got["obstacle"], (np.asarray(obst).reshape(p.ny, p.nx) != 0).astype(np.uint8))
    assert want["vorticity"].any()
