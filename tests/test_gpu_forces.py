"""Momentum-exchange wall forces computed on the device (lbm_wall_force /
lbm_store_wall_force / lbm_set_bodies / lbm_body_forces;
include/lbm_forces_hip.h, csrc/lbm_forces.hip).

Bar: the per-cell map is BITWISE (uint32 patterns) lio.wall_force_cells -- the
fp32 numpy restatement, pinned by physics in tests/test_forces_host.py -- of
the cells store() returns from the same handle: for every step kernel, both
ping-pong sides, both lattice layouts and decomposed handles (links across
sub-domain borders).  Totals and per-body sums are fp64 sums of those fp32
values in the device's order: within (n - 1) 2^-53 sum|term| of math.fsum,
links exact, repeat calls identical.
"""
from __future__ import annotations

import ctypes
import math
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG
from lbm_amd import io as lio
from test_forces_host import _read_forces, forces_reference, printed_within

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _perturbed(p, seed):
    rng = np.random.default_rng(seed)
    return (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((p.ny, p.nx, 9)))).astype(np.float32)


def _obstacles(nx, ny, seed):
    """The generator of tests/test_gpu_fields.py: about 10 % random obstacles; row 0
    blocked at x = 0, nx-2, nx-1 (row and column ends, wrap links); one cell kept fluid."""
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


def _assert_map(got, obst, cells, what=""):
    ref = lio.wall_force_cells(obst, cells)
    assert len(got) == len(ref)
    for name, g, r in zip("xyz", got, ref):
        assert g.dtype == np.float32 and g.shape == r.shape, (what, name)
        bad = _bits(g) != _bits(r)
        assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    return ref


def _nlinks(links):
    n = np.zeros(links.shape, np.int64)
    for j in range(18):
        n += (links >> np.uint32(j)) & np.uint32(1)
    return n


def assert_sum(got, terms, what="", show=True):
    """got: a device fp64 sum of the fp32 `terms` in some fixed order."""
    t = np.asarray(terms, np.float32).astype(np.float64).ravel()
    ref = math.fsum(t)
    bound = max(t.size - 1, 0) * 2.0 ** -53 * float(np.abs(t).sum())
    if show:
        print(f"{what}: {got!r} ref {ref!r} diff {abs(got - ref):.3e} bound {bound:.3e} (n = {t.size})")
    assert abs(got - ref) <= bound, (what, got, ref, bound)


def check_totals_and_bodies(e, links, fmap, labels=None, nbodies=0, what=""):
    """wall_force() (and body_forces()) of the handle against its own map `fmap`."""
    wall = links != 0
    nl = _nlinks(links)
    total = e.wall_force()
    assert len(total) == len(fmap) + 1
    for name, got, comp in zip("xyz", total, fmap):
        assert_sum(got, comp[wall], f"{what} total f{name}")
    assert total[-1] == int(nl.sum())
    again = e.wall_force()
    assert [np.float64(v).view(np.uint64) for v in again[:-1]] == [np.float64(v).view(np.uint64) for v in total[:-1]]
    assert again[-1] == total[-1]
    if labels is None:
        return total
    bodies = e.body_forces()
    again = e.body_forces()
    assert len(bodies) == len(fmap) + 1 and all(len(b) == nbodies for b in bodies)
    for a, b in zip(bodies, again):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for b in range(nbodies):
        sel = wall & (labels == b)
        for name, got, comp in zip("xyz", bodies, fmap):
            assert_sum(float(got[b]), comp[sel], f"{what} body {b} f{name}", show=b < 4)
        assert int(bodies[-1][b]) == int(nl[sel].sum())
    return total


# ----------------------------------------------------- 1. the map, bitwise ----

@pytest.mark.parametrize("nx,ny", [(131, 67), (132, 70), (3, 5), (1, 8), (8, 1), (1, 1), (64, 1)])
def test_wall_force_map_of_loaded_cells_bitwise(gpu_lib, nx, ny):
    p, obst, cells = _problem(nx, ny, 100 * nx + ny)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        got = e.wall_force_field()
        ref = _assert_map(got, obst, cells, (nx, ny))
        links = lio.wall_links(obst)
        assert not _bits(got[0])[links == 0].any() and not _bits(got[1])[links == 0].any()   # exactly +0
        check_totals_and_bodies(e, links, ref, what=f"{nx}x{ny}")


@pytest.mark.parametrize("mode", ["auto", "stream", "stream_tolerance", "step2", "scalar", "pipeline"])
def test_wall_force_map_after_steps_bitwise(gpu_lib, mode):
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
    links = lio.wall_links(obst)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        for steps, first in ((7, True), (1, False)):   # the second run ends on the other lattice of the pair
            e.run_steps(steps, accelerate_first=first)
            cells, _ = e.store(n_av=0)
            ref = _assert_map(e.wall_force_field(), obst, cells, (mode, steps))
            check_totals_and_bodies(e, links, ref, what=f"{mode} {steps}")
        assert e.kernel_in_use() in want


@pytest.mark.parametrize("nx,ny", [(132, 70), (131, 67)])
@pytest.mark.parametrize("kernel", ["step2", "scalar"])
def test_wall_force_map_planar_layout_bitwise(gpu_lib, debug_knobs, monkeypatch, nx, ny, kernel):
    """The planar lattice layout (LBM_LAYOUT=planar, a debug knob) on both ping-pong sides."""
    monkeypatch.setenv("LBM_LAYOUT", "planar")
    n = gpu_lib
    kw = dict(kernel=n.KERNEL_STEP2) if kernel == "step2" else dict(kernel=n.KERNEL_SCALAR, flags=n.FLAG_ONE_STEP)
    p, obst, cells0 = _problem(nx, ny, 13)
    with n.Engine(p, obst, **kw) as e:
        e.load_cells(cells0)
        _assert_map(e.wall_force_field(), obst, cells0, ("planar", nx, ny, 0))
        for steps, first in ((7, True), (1, False)):
            e.run_steps(steps, accelerate_first=first)
            cells, _ = e.store(n_av=0)
            _assert_map(e.wall_force_field(), obst, cells, ("planar", nx, ny, steps))
        assert e.kernel_in_use() == kernel


# ------------------------------------------------------------ 2. decomposed ----

@pytest.fixture(scope="module")
def single_96x80(gpu_lib):
    """(p, obst, cells0, map, labels, nbodies) of the single-domain handle after 7
    steps: the reference of the decomposed cases, computed once and left unchanged."""
    p, obst, cells0 = _problem(96, 80, 31)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(7, accelerate_first=True)
        cells, _ = e.store(n_av=0)
        fmap = e.wall_force_field()
    _assert_map(fmap, obst, cells, "single")
    labels, nbodies = lio.label_bodies(obst)
    for a in list(fmap) + [cells0, labels]:
        a.setflags(write=False)
    return p, obst, cells0, fmap, labels, nbodies


def _decomposed_kw(native, how):
    if how == "local4":
        return dict(parts=4, grid=(2, 2), devices=[0])
    if how == "local2":
        return dict(parts=2, grid=(1, 2), devices=[0])
    return dict(parts=1, grid=(1, 1), devices=[0], flags=native.FLAG_FORCE_EXCHANGE,
                transport=native.TRANSPORT_RCCL, rank=0, world=1, unique_id=native.rccl_unique_id())


@pytest.mark.parametrize("how", ["local4", "local2", "rccl1"])
def test_wall_force_decomposed_bitwise(gpu_lib, single_96x80, how):
    p, obst, cells0, ref, labels, nbodies = single_96x80
    links = lio.wall_links(obst)
    with gpu_lib.Engine(p, obst, **_decomposed_kw(gpu_lib, how)) as e:
        e.load_cells(cells0)
        e.run_steps(7, accelerate_first=True)
        assert len(e.local_rects()) == {"local4": 4, "local2": 2, "rccl1": 1}[how]
        got = e.wall_force_field()
        for name, g, r in zip("xy", got, ref):
            assert np.array_equal(_bits(g), _bits(r)), (how, name)
        e.set_bodies(labels, nbodies)
        check_totals_and_bodies(e, links, ref, labels, nbodies, what=how)


# ------------------------------------------------------ 3. totals and bodies ----

def test_body_forces_single(gpu_lib, single_96x80):
    p, obst, cells0, _, labels, nbodies = single_96x80
    links = lio.wall_links(obst)
    assert nbodies > 50
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(5, accelerate_first=True)
        fmap = e.wall_force_field()
        before = e.wall_force()
        e.set_bodies(labels, nbodies)
        total = check_totals_and_bodies(e, links, fmap, labels, nbodies, what="single")
        assert total[2] == before[2]
        # a negative label: body 3 belongs to no body, the totals stay
        lab2 = np.where(labels == 3, -1, labels)
        e.set_bodies(lab2, nbodies)
        check_totals_and_bodies(e, links, fmap, lab2, nbodies, what="negative label")
        b = e.body_forces()
        assert b[0][3] == 0 and b[1][3] == 0 and b[2][3] == 0
        # fewer, coarser bodies: two halves of the domain
        halves = np.where(obst != 0, (np.arange(p.nx)[None, :] >= p.nx // 2).astype(np.int32), -1).astype(np.int32)
        e.set_bodies(halves, 2)
        check_totals_and_bodies(e, links, fmap, halves, 2, what="halves")
        # a label >= nbodies on a blocked cell is refused and the bodies set before stay
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.set_bodies(labels, 3)
        assert ei.value.code == gpu_lib.LBM_E_INVALID
        check_totals_and_bodies(e, links, fmap, halves, 2, what="halves again")
        # labels on fluid cells are ignored
        junk = np.where(obst != 0, halves, 77).astype(np.int32)
        e.set_bodies(junk, 2)
        check_totals_and_bodies(e, links, fmap, halves, 2, what="junk on fluid")
        # cleared: body_forces is a state error again, totals unchanged in value
        e.set_bodies(None, 0)
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.body_forces()
        assert ei.value.code == gpu_lib.LBM_E_STATE
        check_totals_and_bodies(e, links, fmap, what="cleared")
        # the map after all of that, and the lattice untouched
        for g, r in zip(e.wall_force_field(), fmap):
            assert np.array_equal(_bits(g), _bits(r))


def test_body_chunk_boundaries(gpu_lib):
    """Bodies of exactly one chunk of the per-body reduction (512 wall cells), one cell
    more (two chunks), several chunks, one cell, and a body without wall cells."""
    nx, ny = 64, 60
    p = lio.Params(nx, ny, 8, 10, 0.1, 0.005, 1.85)
    obst = np.zeros((ny, nx), np.uint8)
    obst[::2] = 1                                     # every blocked cell is a wall cell: 30 x 64 = 1920
    links = lio.wall_links(obst)
    assert int((links != 0).sum()) == 1920
    rank = np.cumsum(obst.ravel()).reshape(ny, nx) - 1    # row-major rank among the blocked cells
    bounds = [0, 512, 1025, 1026, 1026, 1920]             # sizes 512, 513, 1, 0, 894
    labels = np.full((ny, nx), -1, np.int32)
    for b in range(5):
        labels[(obst != 0) & (rank >= bounds[b]) & (rank < bounds[b + 1])] = b
    cells0 = _perturbed(p, 4)
    for kw in (dict(), dict(parts=2, grid=(2, 1), devices=[0])):
        with gpu_lib.Engine(p, obst, **kw) as e:
            e.load_cells(cells0)
            e.run_steps(3, accelerate_first=True)
            fmap = e.wall_force_field()
            e.set_bodies(labels, 5)
            check_totals_and_bodies(e, links, fmap, labels, 5, what=f"chunks {sorted(kw)}")
            b = e.body_forces()
            assert b[0][3] == 0 and b[1][3] == 0 and b[2][3] == 0


def test_invalid_body_arguments(gpu_lib):
    p, obst, cells = _problem(16, 8, 3)
    i32p, f64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
    lab = np.zeros((8, 16), np.int32)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells)
        L, h = e._L, e._h
        assert L.lbm_set_bodies(h, lab.ctypes.data_as(i32p), 0) == gpu_lib.LBM_E_INVALID
        assert L.lbm_set_bodies(h, lab.ctypes.data_as(i32p), -1) == gpu_lib.LBM_E_INVALID
        assert L.lbm_set_bodies(h, None, 2) == gpu_lib.LBM_E_INVALID
        assert L.lbm_body_forces(h, None, None, None, 1) == gpu_lib.LBM_E_STATE   # none set
        assert L.lbm_set_bodies(h, lab.ctypes.data_as(i32p), 1) == gpu_lib.LBM_OK
        lab[...] = 5   # the library kept no pointer to the labels
        fx = np.zeros(1)
        assert L.lbm_body_forces(h, fx.ctypes.data_as(f64p), None, None, 1) == gpu_lib.LBM_OK
        tot = ctypes.c_double()
        assert L.lbm_wall_force(h, ctypes.byref(tot), None, None) == gpu_lib.LBM_OK
        assert abs(fx[0] - tot.value) <= 1e-12 * abs(tot.value)
        assert L.lbm_body_forces(h, None, None, None, 2) == gpu_lib.LBM_E_STATE   # another nbodies
        assert L.lbm_wall_force(h, None, None, None) == gpu_lib.LBM_OK
        assert L.lbm_store_wall_force(h, None, None) == gpu_lib.LBM_OK
        only_y = np.full((8, 16), 7.0, np.float32)
        assert L.lbm_store_wall_force(h, None, only_y.ctypes.data_as(ctypes.POINTER(ctypes.c_float))) == gpu_lib.LBM_OK
        assert np.array_equal(_bits(only_y), _bits(lio.wall_force_cells(obst, cells)[1]))


def test_no_obstacles_and_all_obstacles(gpu_lib):
    p = lio.Params(16, 8, 4, 10, 0.1, 0.005, 1.85)
    cells = _perturbed(p, 2)
    for obst in (np.zeros((8, 16), np.uint8), np.ones((8, 16), np.uint8)):
        with gpu_lib.Engine(p, obst) as e:
            e.load_cells(cells)
            fx, fy, links = e.wall_force()
            assert (fx, fy, links) == (0.0, 0.0, 0)
            assert math.copysign(1, fx) == 1 and math.copysign(1, fy) == 1   # exactly +0
            for g in e.wall_force_field():
                assert not _bits(g).any()
            if obst.any():
                e.set_bodies(np.zeros((8, 16), np.int32), 1)
                b = e.body_forces()
                assert b[0][0] == 0 and b[1][0] == 0 and b[2][0] == 0


def test_force_calls_before_load_are_state_errors(gpu_lib):
    p = lio.Params(16, 8, 4, 10, 0.1, 0.005, 1.85)
    obst = _obstacles(16, 8, 1)
    with gpu_lib.Engine(p, obst) as e:
        calls = (e.wall_force, e.wall_force_field, e.body_forces, lambda: e.set_bodies(np.zeros((8, 16), np.int32), 1),
                 lambda: e.set_bodies(None, 0))
        for call in calls:
            with pytest.raises(gpu_lib.LbmError) as ei:
                call()
            assert ei.value.code == gpu_lib.LBM_E_STATE, call
        e.load_cells(_perturbed(p, 2))
        with pytest.raises(gpu_lib.LbmError) as ei:
            e.body_forces()          # loaded, but no bodies set
        assert ei.value.code == gpu_lib.LBM_E_STATE


# ------------------------------------------------------------------ 4. purity ----

@pytest.mark.parametrize("kw", [dict(), dict(parts=4, grid=(2, 2), devices=[0])], ids=["single", "local4"])
def test_force_calls_change_no_engine_state(gpu_lib, single_96x80, kw):
    p, obst, cells0, _, labels, nbodies = single_96x80
    out = []
    for ask in (False, True):
        with gpu_lib.Engine(p, obst, **kw) as e:
            e.load_cells(cells0)
            e.run_steps(5, accelerate_first=True)
            if ask:
                e.wall_force()
                e.wall_force_field()
                e.set_bodies(labels, nbodies)
                e.body_forces()
            e.run_steps(6)
            cells, av = e.store(n_av=6)
            out.append((cells, av))
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))


def test_force_history(gpu_lib):
    p, obst, cells0 = _problem(132, 70, 7, iters=12)
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        samples, av = e.force_history(12, 4, accelerate_first=True)
        cells, _ = e.store(n_av=0)
    assert [s[0] for s in samples] == [4, 8, 12] and av.shape == (12,) and av.dtype == np.float32
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        e.run_steps(12, accelerate_first=True)
        ref_cells, ref_av = e.store(n_av=12)
    assert np.array_equal(_bits(cells), _bits(ref_cells)) and np.array_equal(_bits(av), _bits(ref_av))
    with gpu_lib.Engine(p, obst) as e:
        e.load_cells(cells0)
        for i, chunk in enumerate((4, 4, 4)):
            e.run_steps(chunk, accelerate_first=i == 0)
            assert samples[i][1:] == e.wall_force()
    with gpu_lib.Engine(p, obst) as e:       # the remainder chunk comes last
        e.load_cells(cells0)
        samples, av = e.force_history(11, 4, accelerate_first=True)
        assert [s[0] for s in samples] == [4, 8, 11] and av.shape == (11,)
        assert np.array_equal(_bits(av), _bits(ref_av[:11]))


# ----------------------------------------------------------- 5. profile class ----

def test_wall_force_profile_class(gpu_lib):
    p, obst, cells = _problem(132, 70, 9)
    with gpu_lib.Engine(p, obst, flags=gpu_lib.FLAG_PROFILE) as e:   # a handle that never asks for forces
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.store()
        e.fields()
        names = [k["name"] for k in e.profile_summary()]
        assert names and not [n for n in names if n.startswith("wall_force")]
    with gpu_lib.Engine(p, obst, flags=gpu_lib.FLAG_PROFILE) as e:
        e.load_cells(cells)
        e.run_steps(4, accelerate_first=True)
        e.wall_force()
        prof = {k["name"]: k for k in e.profile_summary()}
        assert prof["wall_force"]["launches"] >= 1 and prof["wall_force"]["total_ms"] > 0
        e.wall_force_field()
        lab, n = lio.label_bodies(obst)
        e.set_bodies(lab, n)
        e.body_forces()
        prof = {k["name"]: k for k in e.profile_summary()}
        assert all(prof[c]["launches"] >= 1 for c in ("wall_force", "wall_force map", "wall_force bodies"))


# ------------------------------------------------------------------ 6. runner ----

def test_runner_gpu_forces(gpu_lib, tmp_path):
    from oracle import oracle
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "50"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    base = [str(exe), "--runs", "0", "--params", str(params), "--obstacles",
            str(GOLD / "params" / "obstacles_128x128.dat")]
    runs = (("plain", ["--device", "gpu"]), ("gpu", ["--device", "gpu", "--forces"]),
            ("loop", ["--device", "loopback", "-n", "4", "--forces"]), ("cpu", ["--device", "cpu", "--forces"]))
    outs = {}
    for name, extra in runs:
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(base + ["--out-dir", str(d)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[name] = "\n".join(line for line in r.stdout.splitlines() if "compute time" not in line)
    assert not (tmp_path / "plain" / "forces.dat").exists()
    assert outs["gpu"] == outs["plain"]
    for f in ("av_vels.dat", "final_state.dat"):
        assert (tmp_path / "gpu" / f).read_bytes() == (tmp_path / "plain" / f).read_bytes()
    p = lio.Params.from_file(str(params))
    obst = lio.read_obstacles(p.nx, p.ny, str(GOLD / "params" / "obstacles_128x128.dat"))
    cells, _ = oracle.run(p, obst, 50, lio.init_cells(p))
    ref = forces_reference(obst, cells)
    for name in ("gpu", "loop", "cpu"):
        got = _read_forces(tmp_path / name / "forces.dat")
        assert len(got) == len(ref)
        for (gx, gy, gl), (rx, ry, rl, bx, by) in zip(got, ref):
            assert gl == rl
            assert printed_within(gx, rx, bx) and printed_within(gy, ry, by), (name, gx, rx, bx, gy, ry, by)


# ------------------------------------------------------- 7. 64-bit offsets ----

def test_wall_force_16384_64bit_offsets(gpu_lib):
    """16384^2 in one sub-domain: the rows above y = 14450 start more than 2^31 floats
    into the row-interleaved lattice, so a wall-list offset formed in 32 bits would wrap
    at the top wall.  Walls on rows 0 and ny-1 only: the flow stays invariant in x bit
    for bit, so the map is one column's map everywhere; the column comes from a
    64 x 16384 engine."""
    n = 16384
    small = lio.Params(64, n, 3, 10, 0.1, 0.005, 1.85)
    sobst = np.zeros((n, 64), np.uint8)
    sobst[0] = sobst[-1] = 1
    with gpu_lib.Engine(small, sobst) as e:
        e.init_equilibrium()
        e.run_steps(3, accelerate_first=True)
        cells, _ = e.store(n_av=0)
    column = [c[:, 5] for c in lio.wall_force_cells(sobst, cells)]
    assert np.abs(column[1][[0, -1]]).min() > 1e-3     # the walls carry the pressure
    p = lio.Params(n, n, 3, 10, 0.1, 0.005, 1.85)
    obst = np.zeros((n, n), np.uint8)
    obst[0] = obst[-1] = 1
    with gpu_lib.Engine(p, obst) as e:
        e.init_equilibrium()
        e.run_steps(3, accelerate_first=True)
        fmap = e.wall_force_field()
        total = e.wall_force()
    for name, g, col in zip("xy", fmap, column):
        assert np.array_equal(_bits(g), np.broadcast_to(_bits(col)[:, None], g.shape)), name
    assert total[2] == 3 * 2 * n
    for i, col in enumerate(column):
        terms = col[[0, -1]].astype(np.float64)
        ref = float(terms.sum()) * n
        bound = (2 * n - 1) * 2.0 ** -53 * float(np.abs(terms).sum()) * n
        print(f"f{'xy'[i]}: total {total[i]!r} ref {ref!r} bound {bound:.3e}")
        assert abs(total[i] - ref) <= 2 * bound
