"""Macroscopic fields and lattice stats computed on the device
(lbm_store_fields / lbm_store_fields_local / lbm_field_stats; csrc/lbm_fields.hip).

Bar: the four fields are BITWISE (compared as uint32 patterns) the values
lio.macroscopic -- the fp32 restatement of writeResults
(LatticeBoltzmannUtils.hpp:221-281) -- derives from the same lattice's AoS
cells, for every step kernel, both ping-pong sides, both widths of the access
path (float4 quads and the ragged w % 4 tail), and decomposed handles.  Every
input keeps the density of each fluid cell positive, so no NaN arises.
"""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG, load_problem, oracle_pressure, small_problems
from lbm_amd import io as lio

pytestmark = pytest.mark.gpu

FIELDS = ("ux", "uy", "speed", "pressure")
SENTINEL = 0x7FC00001   # a quiet NaN pattern no computation produces


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _assert_fields(got, ref, what=""):
    """got: {name: array}; ref: lio.macroscopic's (ux, uy, speed, pressure)."""
    for name, r in zip(FIELDS, ref):
        if name in got:
            bad = _bits(got[name]) != _bits(r)
            assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())


def _perturbed(p, seed):
    rng = np.random.default_rng(seed)
    return (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((p.ny, p.nx, 9)))).astype(np.float32)


def _obstacles(nx, ny, seed):
    """About 10 % random obstacles; row 0 blocked at x = 0, nx-2, nx-1 (both row
    ends and the ragged tail meet the mask); cell (min(nx-1, 2), min(ny-1, 2))
    kept fluid so that every shape has a fluid cell."""
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


# ------------------------------------------------------- 1. bare kernel ----

@pytest.mark.parametrize("nx,ny", [(131, 67), (132, 70), (3, 5), (1, 8), (8, 1), (1, 1), (64, 1)])
def test_fields_of_loaded_cells_bitwise(gpu_lib, nx, ny):
    p, obst, cells = _problem(nx, ny, 100 * nx + ny)
    assert (obst == 0).any()
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        got = e.fields()
    assert set(got) == set(FIELDS) and all(v.shape == (ny, nx) and v.dtype == np.float32 for v in got.values())
    _assert_fields(got, lio.macroscopic(p, obst, cells), (nx, ny))
    ob = obst != 0
    if ob.any():
        for name in ("ux", "uy", "speed"):
            assert not _bits(got[name])[ob].any(), name   # exactly +0
        want = _bits(np.float32(p.density) * np.float32(np.float32(1) / np.float32(3)))
        assert (_bits(got["pressure"])[ob] == want).all()


# ------------------------------------- 2. after steps, every step kernel ----

@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_fields_after_steps_bitwise(gpu_lib, mode):
    n = gpu_lib
    kw, want = {
        # 132x70: small enough for the resident kernel (which a busy device may hand over to step2)
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
        for steps, first in ((7, True), (1, False)):   # the second run ends on the other lattice of the pair
            e.run_steps(steps, accelerate_first=first)
            cells, _ = e.store(n_av=0)
            _assert_fields(e.fields(), lio.macroscopic(p, obst, cells), (mode, steps))
        assert e.kernel_in_use() in want
        if mode == "stream_tolerance":
            assert e.numerics() == "tolerance"


@pytest.mark.parametrize("nx,ny", [(132, 70), (131, 67)])   # float4 quads only; quads + ragged tail
@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_fields_planar_layout_bitwise(gpu_lib, debug_knobs, monkeypatch, nx, ny, kernel):
    """The planar lattice layout (f[k][y][x]: plane stride padded, pitch = one
    plane row; LBM_LAYOUT=planar, a debug knob) on both ping-pong sides."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    p, obst, cells0 = _problem(nx, ny, 13)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        _assert_fields(e.fields(), lio.macroscopic(p, obst, cells0), ("planar", nx, ny, 0))
        for steps, first in ((7, True), (1, False)):
            e.run_steps(steps, accelerate_first=first)
            cells, _ = e.store(n_av=0)
            _assert_fields(e.fields(), lio.macroscopic(p, obst, cells), ("planar", nx, ny, steps))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------- 3. golden small grids ----

@pytest.mark.parametrize("name", sorted(small_problems()))
def test_fields_small_problems_bitwise(gpu_lib, name):
    p, obst, cells0, after = small_problems()[name]
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(10, accelerate_first=True)
        got = e.fields()
    _assert_fields(got, lio.macroscopic(p, obst, after[10][0]), name)


# ------------------------------------------------------ 4. decomposed ----

@pytest.fixture(scope="module")
def single_96x80(gpu_lib):
    """(p, obst, cells after 7 steps, fields) of the single-domain handle: the
    reference of the decomposed cases, computed once and left unchanged."""
    p, obst, cells0 = _problem(96, 80, 31)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(7, accelerate_first=True)
        cells, _ = e.store(n_av=0)
        f = e.fields()
    _assert_fields(f, lio.macroscopic(p, obst, cells), "single")
    for a in list(f.values()) + [cells, cells0]:
        a.setflags(write=False)
    return p, obst, cells0, cells, f


def _decomposed_kw(native, how):
    if how == "local4":
        return dict(parts=4, grid=(2, 2), devices=[0])
    if how == "local2":
        return dict(parts=2, grid=(1, 2), devices=[0])
    return dict(parts=1, grid=(1, 1), devices=[0], flags=native.FLAG_FORCE_EXCHANGE,
                transport=native.TRANSPORT_RCCL, rank=0, world=1, unique_id=native.rccl_unique_id())


@pytest.mark.parametrize("how", ["local4", "local2", "rccl1"])
def test_fields_decomposed_bitwise(gpu_lib, single_96x80, how):
    p, obst, cells0, _, ref = single_96x80
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        e.load_cells(cells0)
        e.run_steps(7, accelerate_first=True)
        full = e.fields()
        local = e.fields_local()
        rects = e.local_rects()
    assert len(rects) == {"local4": 4, "local2": 2, "rccl1": 1}[how] and len(local) == len(rects)
    for name in FIELDS:
        assert np.array_equal(_bits(full[name]), _bits(ref[name])), (how, name)
        for blk, (x0, y0, w, h) in zip(local, rects):
            assert blk[name].shape == (h, w)
            assert np.array_equal(_bits(blk[name]), _bits(ref[name][y0:y0 + h, x0:x0 + w])), (how, name, x0, y0)


# ------------------------------------------------------- 5. selection ----

def test_fields_selection_raw_call(gpu_lib):
    p, obst, cells = _problem(131, 67, 5)
    ref = lio.macroscopic(p, obst, cells)
    f32p = ctypes.POINTER(ctypes.c_float)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        L, h = e._L, e._h
        pressure = np.full((p.ny, p.nx), SENTINEL, np.uint32).view(np.float32)
        assert L.lbm_store_fields(h, None, None, None, pressure.ctypes.data_as(f32p)) == gpu_lib.LBM_OK
        assert np.array_equal(_bits(pressure), _bits(ref[3]))
        # only ux: the pressure array of the earlier call (the library keeps no caller pointer) is not written again
        pressure.view(np.uint32)[...] = SENTINEL
        ux = np.full((p.ny, p.nx), SENTINEL, np.uint32).view(np.float32)
        assert L.lbm_store_fields(h, ux.ctypes.data_as(f32p), None, None, None) == gpu_lib.LBM_OK
        assert np.array_equal(_bits(ux), _bits(ref[0]))
        assert (_bits(pressure) == SENTINEL).all()
        assert L.lbm_store_fields(h, None, None, None, None) == gpu_lib.LBM_OK
        assert L.lbm_store_fields_local(h, None, None, None, None) == gpu_lib.LBM_OK
        assert L.lbm_field_stats(h, None, None) == gpu_lib.LBM_OK
        # the Python selection: exactly the requested names
        got = e.fields(("pressure", "uy"))
        assert sorted(got) == ["pressure", "uy"]
        _assert_fields(got, ref, "subset")
        with pytest.raises(ValueError):
            e.fields(("vorticity",))


# ------------------------------------------------------------ 6. state ----

def test_fields_before_load_is_a_state_error(gpu_lib):
    p = lio.Params(16, 8, 4, 10, 0.1, 0.005, 1.85)
    with gpu_lib.Engine(p, np.zeros((8, 16), np.uint8)) as e:
        for call in (e.fields, e.fields_local, e.field_stats):
            with pytest.raises(gpu_lib.LbmError) as ei:
                call()
            assert ei.value.code == gpu_lib.LBM_E_STATE, call


# ------------------------------------------------------------ 7. stats ----

def _check_stats(e, p, obst):
    cells, _ = e.store(n_av=0)
    rho32 = np.zeros((p.ny, p.nx), np.float32)
    for k in range(9):
        rho32 = rho32 + cells[..., k]
    speed = lio.macroscopic(p, obst, cells)[2]
    mass, umax = e.field_stats()
    again = e.field_stats()
    n = p.nx * p.ny
    mass_ref = float(rho32.astype(np.float64).sum())
    print(f"mass {mass!r} ref {mass_ref!r} rel {abs(mass - mass_ref) / mass_ref:.3e} "
          f"bound {2 * (n - 1) * 2.0 ** -53:.3e}; max |u| {umax!r}")
    # any order of summing n non-negative fp64 terms is within (n-1) 2^-53 relative of the exact sum: both sides
    assert abs(mass - mass_ref) <= 2 * (n - 1) * 2.0 ** -53 * mass_ref
    assert _bits(np.float32(umax)) == _bits(np.max(speed[obst == 0]))
    assert np.float64(again[0]).view(np.uint64) == np.float64(mass).view(np.uint64)
    assert _bits(np.float32(again[1])) == _bits(np.float32(umax))


def test_field_stats_single(gpu_lib):
    p, obst, cells0 = _problem(131, 67, 17)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        _check_stats(e, p, obst)


def test_field_stats_decomposed(gpu_lib, single_96x80):
    p, obst, cells0, _, _ = single_96x80
    with gpu_lib.Engine(p, obst, parts=4, grid=(2, 2), devices=[0]) as e:
        e.load_cells(cells0)
        e.run_steps(7, accelerate_first=True)
        _check_stats(e, p, obst)


def test_field_stats_all_obstacles(gpu_lib):
    p = lio.Params(16, 8, 4, 10, 0.1, 0.005, 1.85)
    obst = np.ones((8, 16), np.uint8)
    cells = _perturbed(p, 2)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        mass, umax = e.field_stats()
    assert umax == 0.0 and _bits(np.float32(umax)) == 0
    assert mass == pytest.approx(float(cells.astype(np.float64).sum()), rel=1e-6)   # obstacle cells carry mass too


# ---------------------------------------------------- 8. reference pin ----

def test_fields_reference_pressure_pin(gpu_lib):
    """The full 128x128 reference run on the default kernel: the device's
    pressure field is the reference-pinned final_state column, bit for bit."""
    p, obst = load_problem("128x128")
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(lio.init_cells(p))
        e.run()
        pressure = e.fields(("pressure",))["pressure"]
    assert np.array_equal(_bits(pressure), _bits(oracle_pressure("128x128")))


# ----------------------------------------------------------- 9. runner ----

def test_runner_device_fields_same_files(gpu_lib, tmp_path):
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "200"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    base = [str(exe), "--device", "gpu", "--runs", "0", "--params", str(params), "--obstacles",
            str(GOLD / "params" / "obstacles_128x128.dat")]
    outs = {}
    for name, extra in (("cells", []), ("fields", ["--device-fields"]), ("debug", ["-d"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(base + ["--out-dir", str(d)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "==done==" in r.stdout
        outs[name] = r.stdout
    want = (tmp_path / "cells" / "final_state.dat").read_bytes()
    assert len(want.splitlines()) == 128 * 128
    assert (tmp_path / "fields" / "final_state.dat").read_bytes() == want
    assert (tmp_path / "fields" / "av_vels.dat").read_bytes() == (tmp_path / "cells" / "av_vels.dat").read_bytes()
    assert "mass:" not in outs["cells"] and "mass:" not in outs["fields"]
    m = re.search(r"^mass: (\S+)  max \|u\|: (\S+)$", outs["debug"], re.M)
    assert m, outs["debug"]
    mass, umax = float(m.group(1)), float(m.group(2))
    # equilibrium at density 0.1 per cell; the flow only redistributes it
    assert mass == pytest.approx(0.1 * 128 * 128, rel=1e-3) and 0 < umax < 0.3


# ---------------------------------------------------- 10. profile class ----

def test_fields_profile_class(gpu_lib):
    p, obst, cells = _problem(132, 70, 9)
    with gpu_lib.Engine(p, obst, flags=gpu_lib.FLAG_PROFILE) as e:   # a handle that never asks for fields
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.store()
        names = [k["name"] for k in e.profile_summary()]
        assert names and not [n for n in names if n.startswith("macroscopic_fields")]
    with gpu_lib.Engine(p, obst, flags=gpu_lib.FLAG_PROFILE) as e:
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        assert not [k for k in e.profile_summary() if k["name"].startswith("macroscopic_fields")]
        e.fields()
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["macroscopic_fields"]["launches"] >= 1 and prof["macroscopic_fields"]["total_ms"] > 0
        e.fields(("pressure",))
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["macroscopic_fields"]["launches"] >= 2
