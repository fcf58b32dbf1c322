"""Momentum-exchange wall forces on the host (no GPU): the numpy restatement
lio.wall_links / wall_force_cells / wall_force (+3d), lio.label_bodies, the
runner's --device cpu --forces path and the exports of include/lbm_forces_hip.h.

The definition is checked by physics, not against itself: over one step the
fluid's momentum changes by the body force minus what the walls took, and the
wall force of a lattice is the momentum handed over in the step that produced
it, so with trapezoid weights
    P_f(2) - P_f(1) = A - (F(1) + F(2)) / 2
per component, A = (fluid cells of row ny-2) * density * accel / 3 for x and 0
for y.  Bound: 16 * 2^-24 * (fluid mass), a few fp32 ulps of density per
colliding cell.  A wrong sign or a swapped direction misses by about |F| ~ 1e-3.
"""
from __future__ import annotations

import math
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG, ROOT, load_problem, small_problems
from lbm_amd import io as lio
from lbm_amd import native

BALANCE = sorted(n for n, v in small_problems().items() if v[0].ny >= 2)


def _fluid_momentum(obst, cells):
    c = cells.astype(np.float64)
    fl = obst == 0
    px = ((c[..., 1] + c[..., 5] + c[..., 8]) - (c[..., 3] + c[..., 6] + c[..., 7]))[fl].sum()
    py = ((c[..., 2] + c[..., 5] + c[..., 6]) - (c[..., 4] + c[..., 7] + c[..., 8]))[fl].sum()
    return np.array([px, py]), float(c.sum(-1)[fl].sum())


@pytest.mark.parametrize("name", BALANCE)
def test_momentum_balance(name):
    p, obst, _, after = small_problems()[name]
    (p1, mass), (p2, _) = _fluid_momentum(obst, after[1][0]), _fluid_momentum(obst, after[2][0])
    f1, f2 = lio.wall_force(obst, after[1][0]), lio.wall_force(obst, after[2][0])
    a = np.array([float((obst[p.ny - 2] == 0).sum()) * float(np.float32(p.density)) * float(np.float32(p.accel)) / 3, 0.0])
    res = (p2 - p1) - (a - (np.array(f1[:2]) + np.array(f2[:2])) / 2)
    bound = 16 * 2.0 ** -24 * mass
    print(f"{name}: residual {res}, bound {bound:.3e}, F(1) {f1}")
    assert np.all(np.abs(res) <= bound), (name, res, bound)


def test_exact_values():
    probs = small_problems()
    assert len(BALANCE) == 6 and "row16x1" not in BALANCE   # the balance above covers every problem with ny >= 2
    p, obst, _, after = probs["open12x10"]
    assert not lio.wall_links(obst).any()
    for n in (1, 2, 10):
        fx, fy, links = lio.wall_force(obst, after[n][0])
        assert (fx, fy, links) == (0.0, 0.0, 0) and math.copysign(1, fx) == 1 and math.copysign(1, fy) == 1
        for f in lio.wall_force_cells(obst, after[n][0]):
            assert f.dtype == np.float32 and not f.view(np.uint32).any()   # +0 everywhere
    assert lio.wall_force(probs["box16x8"][1], probs["box16x8"][3][1][0])[2] == 116
    assert lio.wall_force(probs["chan20x24"][1], probs["chan20x24"][3][1][0])[2] == 242


def test_links_by_hand():
    obst = np.zeros((4, 5), np.uint8)
    obst[1, 1] = obst[1, 2] = 1
    links = lio.wall_links(obst)
    assert links.dtype == np.uint32 and links.shape == (4, 5)
    # (1,1): every neighbour is fluid but E (1,2)
    assert links[1, 1] == 0xFF & ~0x01 and links[1, 2] == 0xFF & ~0x04
    assert not links[obst == 0].any()
    # a blocked cell that is its own neighbour in every direction has no links
    assert not lio.wall_links(np.ones((1, 1), np.uint8)).any()
    one = lio.wall_links(np.array([[1, 0, 0]], np.uint8))   # ny = 1: N/S neighbours are the cell itself
    assert one[0, 0] == (1 << 0) | (1 << 2) | (1 << 4) | (1 << 5) | (1 << 6) | (1 << 7)
    # 3-D: a single blocked cell in open space has all 18 links
    o3 = np.zeros((3, 3, 3), np.uint8)
    o3[1, 1, 1] = 1
    assert lio.wall_links3d(o3)[1, 1, 1] == (1 << 18) - 1 and int((lio.wall_links3d(o3) != 0).sum()) == 1


def test_force_cells_3d_direction_table():
    """One blocked cell, one population at a time: the force points against the
    stored (reversed) population's velocity, twice its value."""
    o3 = np.zeros((3, 3, 3), np.uint8)
    o3[1, 1, 1] = 1
    for j in range(1, 19):
        cells = np.zeros((3, 3, 3, 19), np.float32)
        cells[1, 1, 1, j] = 0.25
        f = [float(c[1, 1, 1]) for c in lio.wall_force_cells3d(o3, cells)]
        assert f == [-0.5 * e for e in lio.E3[j]], j
        tot = lio.wall_force3d(o3, cells)
        assert tot[:3] == tuple(f) and tot[3] == 18
    o2 = np.zeros((3, 3), np.uint8)
    o2[1, 1] = 1
    for j in range(1, 9):
        cells = np.zeros((3, 3, 9), np.float32)
        cells[1, 1, j] = 0.25
        assert [float(c[1, 1]) for c in lio.wall_force_cells(o2, cells)] == [-0.5 * e for e in lio.E2[j]], j


def test_label_bodies():
    o = np.zeros((8, 10), np.uint8)
    o[1:3, 1:3] = 1          # box A
    o[5:7, 6:9] = 1          # box B
    lab, n = lio.label_bodies(o)
    assert n == 2 and lab.dtype == np.int32 and (lab[o == 0] == -1).all()
    assert (lab[1:3, 1:3] == 0).all() and (lab[5:7, 6:9] == 1).all()
    # a box across the periodic edges is one body, and it is numbered first (its first cell is (0, 0))
    o = np.zeros((6, 7), np.uint8)
    o[0, 0] = o[0, 6] = o[5, 0] = o[5, 6] = 1
    o[3, 3] = 1
    lab, n = lio.label_bodies(o)
    assert n == 2 and lab[0, 0] == lab[0, 6] == lab[5, 0] == lab[5, 6] == 0 and lab[3, 3] == 1
    # cells that touch by a corner are one body
    o = np.zeros((6, 6), np.uint8)
    o[1, 1] = o[2, 2] = 1
    o[4, 1] = 1
    lab, n = lio.label_bodies(o)
    assert n == 2 and lab[1, 1] == lab[2, 2] == 0 and lab[4, 1] == 1
    # a long snake: many propagation rounds
    o = np.zeros((9, 40), np.uint8)
    o[1, 1:39] = o[1:8, 38] = o[7, 1:39] = o[3:8, 1] = o[3, 1:36] = 1
    lab, n = lio.label_bodies(o)
    assert n == 1 and (lab[o != 0] == 0).all()
    assert lio.label_bodies(np.zeros((3, 3), np.uint8))[1] == 0
    # 3-D: 26-connected, periodic in z
    o3 = np.zeros((4, 4, 4), np.uint8)
    o3[0, 0, 0] = o3[3, 3, 3] = 1      # corner neighbours through the wrap in all three directions
    o3[1, 2, 2] = 1
    lab, n = lio.label_bodies(o3)
    assert n == 2 and lab[0, 0, 0] == lab[3, 3, 3] == 0 and lab[1, 2, 2] == 1


@pytest.mark.parametrize("name", ["box16x8", "wall32x32", "ragged13x7"])
def test_body_sums_add_up(name):
    p, obst, _, after = small_problems()[name]
    cells = after[10][0]
    lab, n = lio.label_bodies(obst)
    assert n >= 1
    total, (bfx, bfy, bl) = lio.wall_force(obst, cells, lab, n)
    assert total == lio.wall_force(obst, cells)
    fx, fy = lio.wall_force_cells(obst, cells)
    wall = lio.wall_links(obst) != 0
    assert int(bl.sum()) == total[2]
    for got, comp, tot in ((bfx, fx, total[0]), (bfy, fy, total[1])):
        terms = comp[wall].astype(np.float64)
        assert abs(float(got.sum()) - tot) <= 2 * terms.size * 2.0 ** -53 * float(np.abs(terms).sum())
        for b in range(n):
            t = comp[wall & (lab == b)].astype(np.float64)
            assert abs(got[b] - math.fsum(t)) <= max(t.size - 1, 0) * 2.0 ** -53 * float(np.abs(t).sum())
    # a negative label takes a body's cells out of the bodies, not out of the total
    lab2 = np.where(lab == 0, -1, lab)
    total2, (bfx2, _, bl2) = lio.wall_force(obst, cells, lab2, n)
    assert total2 == total and bfx2[0] == 0 and bl2[0] == 0
    with pytest.raises(ValueError):
        lio.wall_force(obst, cells, lab + 1, n)


# ---------------------------------------------------------------- runner ----

def _read_forces(path):
    rows = [line.split() for line in path.read_text().splitlines()]
    assert rows and rows[-1][0] == "total" and all(len(r) == 4 for r in rows)
    assert [r[0] for r in rows[:-1]] == [str(i) for i in range(len(rows) - 1)]
    for r in rows:
        assert re.fullmatch(r"-?\d\.\d{12}E[+-]\d{2,}", r[1]) and re.fullmatch(r"-?\d\.\d{12}E[+-]\d{2,}", r[2]), r
    return [(float(r[1]), float(r[2]), int(r[3])) for r in rows]


def printed_within(value, ref, bound):
    """`value` was printed with %.12E: it lies within `bound` of `ref` iff it is
    between the %.12E prints of ref - bound and ref + bound (printing is monotone)."""
    lo, hi = float(f"{ref - bound:.12E}"), float(f"{ref + bound:.12E}")
    return lo <= value <= hi


def forces_reference(obst, cells):
    """[(fx, fy, links, bound_x, bound_y)] per body of lio.label_bodies, then the total:
    math.fsum of the fp32 per-cell values and the bound (n-1) 2^-53 sum|term|."""
    lab, n = lio.label_bodies(obst)
    links = lio.wall_links(obst)
    nl = np.zeros(links.shape, np.int64)
    for j in range(8):
        nl += (links >> np.uint32(j)) & np.uint32(1)
    fx, fy = lio.wall_force_cells(obst, cells)
    out = []
    for sel in [(links != 0) & (lab == b) for b in range(n)] + [links != 0]:
        row = []
        for comp in (fx, fy):
            t = comp[sel].astype(np.float64)
            row.append((math.fsum(t), max(t.size - 1, 0) * 2.0 ** -53 * float(np.abs(t).sum())))
        out.append((row[0][0], row[1][0], int(nl[sel].sum()), row[0][1], row[1][1]))
    return out


def test_runner_cpu_forces(tmp_path):
    from oracle import oracle
    exe = PKG / "build" / "lbm_runner"
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = "50"
    params = tmp_path / "p.params"
    params.write_text("\n".join(lines))
    base = [str(exe), "--device", "cpu", "--runs", "0", "--params", str(params), "--obstacles",
            str(GOLD / "params" / "obstacles_128x128.dat")]
    outs = {}
    for name, extra in (("plain", []), ("forces", ["--forces"])):
        d = tmp_path / name
        d.mkdir()
        r = subprocess.run(base + ["--out-dir", str(d)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[name] = "\n".join(line for line in r.stdout.splitlines() if "compute time" not in line)
    assert not (tmp_path / "plain" / "forces.dat").exists()
    assert outs["plain"] == outs["forces"] and "==done==" in outs["plain"]
    for f in ("av_vels.dat", "final_state.dat"):
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "forces" / f).read_bytes()
    got = _read_forces(tmp_path / "forces" / "forces.dat")
    p, obst = load_problem("128x128", 50)
    cells, _ = oracle.run(p, obst, 50, lio.init_cells(p))
    ref = forces_reference(obst, cells)
    assert len(got) == len(ref) >= 2
    for (gx, gy, gl), (rx, ry, rl, bx, by) in zip(got, ref):
        print(f"fx {gx!r} ref {rx!r} bound {bx:.3e}; fy {gy!r} ref {ry!r} bound {by:.3e}; links {gl}")
        assert gl == rl and rl > 0
        assert printed_within(gx, rx, bx) and printed_within(gy, ry, by)
    assert abs(got[-1][0]) > 1e-3    # a developed drag, not a row of zeros


# --------------------------------------------------------------- exports ----

def test_library_exports_every_force_symbol():
    text = (ROOT / "include" / "lbm_forces_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 8 and sorted(native.EXPORTED_FORCES) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    assert L.lbm_abi_version() == 5
    assert not set(syms) & (set(native.EXPORTED) | set(native.EXPORTED3D) | set(native.EXPORTED3D_FIELDS))


def test_null_handle_is_invalid():
    L = native.load_library()
    assert L.lbm_wall_force(None, None, None, None) == native.LBM_E_INVALID
    assert L.lbm_store_wall_force(None, None, None) == native.LBM_E_INVALID
    assert L.lbm_set_bodies(None, None, 0) == native.LBM_E_INVALID
    assert L.lbm_body_forces(None, None, None, None, 0) == native.LBM_E_INVALID
    assert L.lbm3d_wall_force(None, None, None, None, None) == native.LBM_E_INVALID
    assert L.lbm3d_store_wall_force(None, None, None, None) == native.LBM_E_INVALID
    assert L.lbm3d_set_bodies(None, None, 0) == native.LBM_E_INVALID
    assert L.lbm3d_body_forces(None, None, None, None, None, 0) == native.LBM_E_INVALID
