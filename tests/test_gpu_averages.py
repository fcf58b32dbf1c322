"""Time-averaged fields and Reynolds stresses accumulated on the device, D2Q9
(lbm_avg_*; include/lbm_averages_hip.h, csrc/lbm_averages.hip).

Bar: the fp64 sums are BITWISE (uint64 patterns) lio.moment_sums of the same
handle's fields() after each chunk, and the fp32 means and central moments
BITWISE (uint32) lio.moment_means of those sums -- the numpy restatement of the
header's definition, pinned by exact arithmetic in tests/test_averages_host.py
-- for both moment selections, every step kernel, both lattice layouts, both
sides of the ping-pong pair, the quad path and the ragged tail, and decomposed
handles.  No tolerance anywhere.
"""
from __future__ import annotations

import ctypes
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG, small_problems
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

FIRST = ("ux", "uy", "pressure")
CHUNKS = (3, 1, 4, 2, 5)      # odd and even: both lattices of the pair get sampled
SENTINEL32 = 0x7FC00001       # quiet NaN patterns no computation produces
SENTINEL64 = 0x7FF8000000000001


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _perturbed(p, seed):
    rng = np.random.default_rng(seed)
    return (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((p.ny, p.nx, 9)))).astype(np.float32)


def _obstacles(nx, ny, seed):
    """About 10 % random obstacles; row 0 blocked at x = 0, nx-2, nx-1 (both row ends and
    the ragged tail meet the mask); one cell kept fluid so that every shape has one."""
    rng = np.random.default_rng(seed)
    obst = (rng.random((ny, nx)) < 0.1).astype(np.uint8)
    for x in (0, nx - 2, nx - 1):
        if x >= 0:
            obst[0, x] = 1
    obst[min(ny - 1, 2), min(nx - 1, 2)] = 0
    return obst


def _problem(nx, ny, seed, iters=8):
    p = lio.Params(nx, ny, iters, 10, 0.1, 0.005, 1.85)
    return p, _obstacles(nx, ny, seed), _perturbed(p, seed + 1)


def _names(e, second):
    return e._AVG_FIELDS if second else e._AVG_FIELDS[:len(FIRST)]


def _sample_run(e, chunks=CHUNKS, first=True):
    """Run the chunks, sampling after each; returns the samples fields() gave."""
    samples = []
    for i, n in enumerate(chunks):
        if n:
            e.run_steps(n, accelerate_first=first and i == 0)
        e.avg_sample()
        f = e.fields(FIRST)
        samples.append([f[k] for k in FIRST])
    return samples


def _assert_averages(e, samples, second, what=""):
    """avg_sums() and mean_fields() of the handle against the restatement of its samples."""
    names = _names(e, second)
    assert e.avg_samples == len(samples)
    sums = e.avg_sums()
    assert tuple(sums) == names
    ref = lio.moment_sums(samples, second)
    for name, r in zip(names, ref):
        assert sums[name].dtype == np.float64 and sums[name].shape == r.shape
        bad = _b64(sums[name]) != _b64(r)
        assert not bad.any(), (what, "sum", name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    means = e.mean_fields()
    assert tuple(means) == names
    for name, r in zip(names, lio.moment_means(ref, len(samples))):
        assert means[name].dtype == np.float32
        bad = _b32(means[name]) != _b32(r)
        assert not bad.any(), (what, "mean", name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return sums, means


# ------------------------------------------------------------ 1. shapes ----

@pytest.mark.parametrize("second", [False, True], ids=["mean", "mean_second"])
@pytest.mark.parametrize("nx,ny", [(131, 67), (132, 70), (3, 5), (1, 8), (8, 1), (1, 1)])
def test_averages_shapes_bitwise(gpu_lib, nx, ny, second):
    p, obst, cells = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        e.avg_begin(second=second)
        assert e.avg_samples == 0
        samples = _sample_run(e)
        sums, means = _assert_averages(e, samples, second, (nx, ny))
    ob = obst != 0
    if ob.any():   # obstacle cells: 0, 0, density / 3 in every sample
        for name in ("ux", "uy"):
            assert not _b64(sums[name])[ob].any() and not _b32(means[name])[ob].any()
        assert (_b32(means["pressure"])[ob] ==
                _b32(np.float32(p.density) * np.float32(np.float32(1) / np.float32(3)))).all()


# ----------------------------------------------- 2. every step kernel ----

@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_averages_every_kernel_bitwise(gpu_lib, mode):
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
        e.avg_begin()
        _assert_averages(e, _sample_run(e), True, mode)
        assert e.kernel_in_use() in want
        if mode == "stream_tolerance":
            assert e.numerics() == "tolerance"


@pytest.mark.parametrize("nx,ny", [(132, 70), (131, 67)])
@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_averages_planar_layout_bitwise(gpu_lib, debug_knobs, monkeypatch, nx, ny, kernel):
    """The planar lattice layout (LBM_LAYOUT=planar, a debug knob)."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    p, obst, cells0 = _problem(nx, ny, 13)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        e.avg_begin()
        _assert_averages(e, _sample_run(e), True, ("planar", nx, ny))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------- 3. golden small grids ----

@pytest.mark.parametrize("name", sorted(small_problems()))
def test_averages_small_problems_developed(gpu_lib, name):
    """50 steps sampled every 10.  Every golden problem that flows (its golden av_vels are
    non-zero) must show a velocity variance somewhere.  row16x1 has one row, hence no
    accelerated row: its golden av_vels are exactly 0, the lattice never moves, and there
    every velocity moment must be exactly +0 instead."""
    p, obst, cells0, after = small_problems()[name]
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin()
        samples = _sample_run(e, (10,) * 5)
        _, means = _assert_averages(e, samples, True, name)
    if after[10][1].any():
        assert (means["uxux"] > 0).any()    # a developed, changing flow: not a row of zeros
    else:
        assert name == "row16x1"
        for k in ("ux", "uy", "uxux", "uxuy", "uyuy"):
            assert not _b32(means[k]).any(), k


# ------------------------------------------------------ 4. decomposed ----

@pytest.fixture(scope="module")
def single_96x80(gpu_lib):
    """(p, obst, cells0, sums, means) of the single-domain handle: the reference of the
    decomposed cases, computed once and left unchanged."""
    p, obst, cells0 = _problem(96, 80, 31)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin()
        sums, means = _assert_averages(e, _sample_run(e), True, "single")
    for a in list(sums.values()) + list(means.values()) + [cells0]:
        a.setflags(write=False)
    return p, obst, cells0, sums, means


def _decomposed_kw(native, how):
    if how == "local4":
        return dict(parts=4, grid=(2, 2), devices=[0])
    if how == "local2":
        return dict(parts=2, grid=(1, 2), devices=[0])
    return dict(parts=1, grid=(1, 1), devices=[0], flags=native.FLAG_FORCE_EXCHANGE,
                transport=native.TRANSPORT_RCCL, rank=0, world=1, unique_id=native.rccl_unique_id())


@pytest.mark.parametrize("how", ["local4", "local2", "rccl1"])
def test_averages_decomposed_bitwise(gpu_lib, single_96x80, how):
    p, obst, cells0, ref_sums, ref_means = single_96x80
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        e.load_cells(cells0)
        e.avg_begin()
        _sample_run(e)
        sums, means = e.avg_sums(), e.mean_fields()
        assert len(e.local_rects()) == {"local4": 4, "local2": 2, "rccl1": 1}[how]
    for name in gpu_lib.AVG_FIELDS:
        assert np.array_equal(_b64(sums[name]), _b64(ref_sums[name])), (how, name)
        assert np.array_equal(_b32(means[name]), _b32(ref_means[name])), (how, name)


# ------------------------------------------------- 5. constant lattice ----

def test_averages_of_a_constant_lattice(gpu_lib):
    p, obst, cells = _problem(131, 67, 5)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        e.avg_begin()
        for _ in range(5):
            e.avg_sample()
        f = e.fields(FIRST)
        means = e.mean_fields()
    for name in FIRST:
        assert np.array_equal(_b32(means[name]), _b32(f[name])), name
    for name in gpu_lib.AVG_FIELDS[3:]:
        assert not _b32(means[name]).any(), name     # exactly +0


# -------------------------------------------- 6. no engine state touched ----

def test_sampling_touches_no_engine_state(gpu_lib):
    p, obst, cells0 = _problem(132, 70, 21, iters=13)

    def sampled():
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells0)
            e.avg_begin()
            e.run_steps(7, accelerate_first=True)
            av7 = e.store(cells=False, n_av=7)[1].copy()
            e.avg_sample()
            e.run_steps(6)
            cells, av6 = e.store(n_av=6)
            e.avg_sample()
            return cells, np.concatenate([av7, av6]), e.avg_sums()

    cells_a, av_a, sums_a = sampled()
    cells_b, av_b, sums_b = sampled()
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(13, accelerate_first=True)
        cells, av = e.store(n_av=13)
    assert np.array_equal(_b32(cells_a), _b32(cells)) and np.array_equal(_b32(av_a), _b32(av))
    assert np.array_equal(_b32(cells_b), _b32(cells)) and np.array_equal(_b32(av_b), _b32(av))
    for name in gpu_lib.AVG_FIELDS:
        assert np.array_equal(_b64(sums_a[name]), _b64(sums_b[name])), name


# ---------------------------------------------------------- 7. contract ----

def _ptrs(ctype, n, arrays):
    """The array of n output pointers with arrays {index: ndarray} set, the rest NULL."""
    out = (ctypes.POINTER(ctype) * n)()
    for i, a in arrays.items():
        out[i] = a.ctypes.data_as(ctypes.POINTER(ctype))
    return out


def test_averages_contract(gpu_lib):
    n = gpu_lib
    p, obst, cells = _problem(131, 67, 9)
    nf = len(n.AVG_FIELDS)
    shape = (p.ny, p.nx)
    with n.Engine(p, obst) as e:
        L, h = e._L, e._h
        f32 = {i: np.full(shape, SENTINEL32, np.uint32).view(np.float32) for i in range(nf)}
        f64 = {i: np.full(shape, SENTINEL64, np.uint64).view(np.float64) for i in range(nf)}
        all32, all64 = _ptrs(ctypes.c_float, nf, f32), _ptrs(ctypes.c_double, nf, f64)
        none32, none64 = _ptrs(ctypes.c_float, nf, {}), _ptrs(ctypes.c_double, nf, {})
        cnt = ctypes.c_int64(-1)

        def untouched():
            return all((_b32(a) == SENTINEL32).all() for a in f32.values()) and \
                all((_b64(a) == SENTINEL64).all() for a in f64.values())

        # before begin
        assert L.lbm_avg_sample(h) == n.LBM_E_STATE
        assert L.lbm_avg_store(h, all32) == n.LBM_E_STATE
        assert L.lbm_avg_store_sums(h, all64) == n.LBM_E_STATE
        assert L.lbm_avg_end(h) == n.LBM_OK
        assert L.lbm_avg_samples(h, ctypes.byref(cnt)) == n.LBM_OK and cnt.value == 0
        for bad in (0, 2, 4, 7, -1):
            assert L.lbm_avg_begin(h, bad) == n.LBM_E_INVALID, bad
        assert L.lbm_avg_sample(h) == n.LBM_E_STATE      # a refused begin starts nothing
        # begun, no lattice yet
        assert L.lbm_avg_begin(h, n.AVG_MEAN) == n.LBM_OK
        assert L.lbm_avg_sample(h) == n.LBM_E_STATE
        e.load_cells(cells)
        # zero samples: store refuses, store_sums writes zeros
        first32 = _ptrs(ctypes.c_float, nf, {i: f32[i] for i in range(3)})
        assert L.lbm_avg_store(h, first32) == n.LBM_E_STATE
        first64 = _ptrs(ctypes.c_double, nf, {i: f64[i] for i in range(3)})
        assert L.lbm_avg_store_sums(h, first64) == n.LBM_OK
        assert all(not _b64(f64[i]).any() for i in range(3))
        for i in range(3):
            _b64(f64[i])[...] = SENTINEL64
        assert L.lbm_avg_store(h, none32) == n.LBM_OK and L.lbm_avg_store_sums(h, none64) == n.LBM_OK
        assert untouched()
        # MEAN only: a second-moment entry is refused and nothing is written
        assert L.lbm_avg_sample(h) == n.LBM_OK
        assert L.lbm_avg_store(h, all32) == n.LBM_E_INVALID
        assert L.lbm_avg_store_sums(h, all64) == n.LBM_E_INVALID
        assert L.lbm_avg_store(h, _ptrs(ctypes.c_float, nf, {0: f32[0], 5: f32[5]})) == n.LBM_E_INVALID
        assert untouched()
        with pytest.raises(n.LbmError) as ei:
            e.mean_fields(("uxux",))
        assert ei.value.code == n.LBM_E_INVALID
        with pytest.raises(ValueError):
            e.mean_fields(("vorticity",))
        # selection: only the entries given are written
        fields = e.fields(FIRST)
        assert L.lbm_avg_store(h, _ptrs(ctypes.c_float, nf, {1: f32[1]})) == n.LBM_OK
        assert np.array_equal(_b32(f32[1]), _b32(fields["uy"]))
        assert L.lbm_avg_store_sums(h, _ptrs(ctypes.c_double, nf, {2: f64[2]})) == n.LBM_OK
        assert np.array_equal(_b64(f64[2]), _b64(fields["pressure"].astype(np.float64)))
        _b32(f32[1])[...] = SENTINEL32
        _b64(f64[2])[...] = SENTINEL64
        assert untouched()
        # begin again re-zeroes; begin with other moments re-allocates
        assert L.lbm_avg_begin(h, n.AVG_MEAN) == n.LBM_OK
        assert e.avg_samples == 0 and not any(_b64(v).any() for v in e.avg_sums(FIRST).values())
        assert L.lbm_avg_sample(h) == n.LBM_OK and L.lbm_avg_sample(h) == n.LBM_OK and e.avg_samples == 2
        assert L.lbm_avg_begin(h, n.AVG_MEAN | n.AVG_SECOND) == n.LBM_OK
        assert e.avg_samples == 0 and not any(_b64(v).any() for v in e.avg_sums(n.AVG_FIELDS).values())
        assert L.lbm_avg_sample(h) == n.LBM_OK
        assert L.lbm_avg_store(h, all32) == n.LBM_OK and L.lbm_avg_store_sums(h, all64) == n.LBM_OK
        assert np.array_equal(_b32(f32[0]), _b32(fields["ux"]))
        # end, then sample
        assert L.lbm_avg_end(h) == n.LBM_OK and L.lbm_avg_end(h) == n.LBM_OK
        assert L.lbm_avg_sample(h) == n.LBM_E_STATE
        assert L.lbm_avg_samples(h, ctypes.byref(cnt)) == n.LBM_OK and cnt.value == 0
        assert L.lbm_avg_samples(h, None) == n.LBM_E_INVALID
        e.avg_begin()        # the handle is destroyed while averaging: lbm_destroy frees the sums


# ------------------------------------------------------ 8. run_averaged ----

def test_run_averaged(gpu_lib):
    p, obst, cells0 = _problem(132, 70, 3, iters=23)
    with gpu_lib.Engine(p, obst) as e:
        assert e.numerics() == "bitwise"
        e.load_cells(cells0)
        e.run_steps(23, accelerate_first=True)
        cells, av = e.store(n_av=23)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin()
        got_av = e.run_averaged(23, 5, accelerate_first=True)
        assert e.avg_samples == 5
        got_cells, _ = e.store(n_av=0)
        sums = e.avg_sums()
        with pytest.raises(ValueError):
            e.run_averaged(5, 0)
    assert got_av.dtype == np.float32 and got_av.shape == (23,)
    assert np.array_equal(_b32(got_av), _b32(av)) and np.array_equal(_b32(got_cells), _b32(cells))
    # the same samples taken by hand
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.avg_begin()
        ref = lio.moment_sums(_sample_run(e, (5, 5, 5, 5, 3)), True)
    for name, r in zip(gpu_lib.AVG_FIELDS, ref):
        assert np.array_equal(_b64(sums[name]), _b64(r)), name


# ----------------------------------------------------- 9. profile class ----

def test_averages_profile_class(gpu_lib):
    p, obst, cells = _problem(132, 70, 9)
    classes = ("accumulate_moments", "moment_means")
    with gpu_lib.Engine(p, obst, flags=gpu_lib.FLAG_PROFILE) as e:   # a handle that never averages
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.fields()
        names = [k["name"] for k in e.profile_summary()]
        assert names and not [n for n in names if n in classes]
    with gpu_lib.Engine(p, obst, flags=gpu_lib.FLAG_PROFILE, parts=2, grid=(1, 2), devices=[0]) as e:
        e.load_cells(cells)
        e.avg_begin()
        e.run_steps(4, accelerate_first=True)
        assert not [k for k in e.profile_summary() if k["name"] in classes]
        for _ in range(3):
            e.avg_sample()
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["accumulate_moments"]["launches"] == 3 * 2 and prof["accumulate_moments"]["total_ms"] > 0
        assert "moment_means" not in prof
        e.mean_fields()
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["moment_means"]["launches"] == 2 and prof["accumulate_moments"]["launches"] == 6


# ----------------------------------------------------------- 10. runner ----

def test_runner_mean_every(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "50"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    base = [str(exe), "--device", "gpu", "--runs", "0", "--params", str(params), "--obstacles", str(obst_file)]
    for name, extra in (("plain", []), ("mean", ["--mean-every", "10"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(base + ["--out-dir", str(d)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
    assert not (tmp_path / "plain" / "mean_state.dat").exists()
    for f in ("av_vels.dat", "final_state.dat"):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "mean" / f).read_bytes(), f
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(obst_file))
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(lio.init_cells(p))
        e.avg_begin()
        e.run_averaged(50, 10, accelerate_first=True)
        assert e.avg_samples == 5
        means = e.mean_fields()
    rows = (tmp_path / "mean" / "mean_state.dat").read_text().splitlines()
    assert len(rows) == p.nx * p.ny
    cols = [means[k].ravel().tolist() for k in gpu_lib.AVG_FIELDS]
    ob = obst.ravel().astype(int).tolist()
    for i, row in enumerate(rows):
        want = f"{i % p.nx} {i // p.nx} " + " ".join(f"{c[i]:.12e}" for c in cols) + f" {ob[i]}"
        assert row == want, (i, row, want)
    assert (means["uxux"] > 0).any()
