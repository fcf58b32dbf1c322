"""Host side of the binned sums (include/lbm_binned_hip.h; CPU only).

* The header declares exactly native.EXPORTED_BINNED: four symbols, all exported
  by the library and disjoint from the other headers' lists; the ABI version
  stays 5; the enum values are the positions in BIN_FIELDS / BIN_FIELDS3D; the
  work-unit constants the GPU tests place their borders around are the kernels'.
* The numpy restatement the GPU tests compare against (lio.binned_sums /
  binned_sums3d / binned_means) is pinned by arithmetic, not against itself:
  one-cell bins against lio.macroscopic, the whole-domain density against an
  fsum of the fluid densities, a ragged grid against a brute-force double loop.
* lbm_runner --device cpu --binned (lbmhost::binnedSums, a second
  implementation that adds row after row) writes what the restatement derives
  from the same run's cells, within the header's bound.
"""
from __future__ import annotations

import math
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD, PKG, ROOT
from lbm_amd import io as lio
from lbm_amd import native
from oracle import oracle

EXE = PKG / "build" / "lbm_runner"
F2 = ("rho", "jx", "jy", "ux", "uy", "speed", "uxux", "uxuy", "uyuy")
F3 = ("rho", "jx", "jy", "jz", "ux", "uy", "uz", "speed", "uxux", "uxuy", "uxuz", "uyuy", "uyuz", "uzuz")


def _b32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _random2(seed, ny=9, nx=11, density=0.1):
    rng = np.random.default_rng(seed)
    p = lio.Params(nx, ny, 4, 10, density, 0.005, 1.85)
    cells = (lio.init_cells(p) * (1 + 0.05 * rng.standard_normal((ny, nx, 9)))).astype(np.float32)
    obst = (rng.random((ny, nx)) < 0.2).astype(np.uint8)
    return p, obst, cells


def _random3(seed, nz=5, ny=6, nx=7):
    rng = np.random.default_rng(seed)
    p = lio.Params3D(nx, ny, nz, 4, 0.1, 0.005, 1.7)
    w = np.array([(1 / 3, 1 / 18, 1 / 36)[sum(c * c for c in e)] for e in lio.E3])
    cells = (0.1 * w * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    obst = (rng.random((nz, ny, nx)) < 0.2).astype(np.uint8)
    return p, obst, cells


# --------------------------------------------------------------- exports ----

def test_library_exports_every_binned_symbol():
    text = (ROOT / "include" / "lbm_binned_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 4 and sorted(native.EXPORTED_BINNED) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    assert L.lbm_abi_version() == 5
    others = (set(native.EXPORTED) | set(native.EXPORTED3D) | set(native.EXPORTED3D_FIELDS)
              | set(native.EXPORTED_FORCES) | set(native.EXPORTED_AVERAGES) | set(native.EXPORTED_GRADIENTS)
              | set(native.EXPORTED_STRESS))
    assert not set(syms) & others


def test_field_name_lists_follow_the_header_enums():
    text = (ROOT / "include" / "lbm_binned_hip.h").read_text()
    assert native.BIN_FIELDS == F2 == lio.BIN_FIELDS and native.BIN_FIELDS3D == F3 == lio.BIN_FIELDS3D
    for prefix, names in (("LBM_BIN_", F2), ("LBM3D_BIN_", F3)):
        for i, n in enumerate(names):
            assert re.search(rf"\b{prefix}{n.upper()} = {i}\b", text), (prefix, n)
        assert re.search(rf"\b{prefix}FIELDS = {len(names)}\b", text)
    hpp = (PKG / "csrc" / "lbm_binned.hpp").read_text()
    num = {k: int(v) for k, v in re.findall(r"\b(BN_QUAD|BN_WAVE_COLS|BN3_WAVE_COLS|BN_CHUNK) = (\d+)", hpp)}
    assert (native.BIN_QUAD, native.BIN_WAVE_COLS, native.BIN_CHUNK_ROWS, native.BIN3D_WAVE_COLS) == (
        num["BN_QUAD"], num["BN_WAVE_COLS"], num["BN_CHUNK"], num["BN3_WAVE_COLS"])
    assert native.BIN_WAVE_COLS == 64 * native.BIN_QUAD


def test_null_handle_is_invalid():
    L = native.load_library()
    assert L.lbm_store_binned(None, 1, 1, None) == native.LBM_E_INVALID
    assert L.lbm_bin_fluid_cells(None, 1, 1, None) == native.LBM_E_INVALID
    assert L.lbm3d_store_binned(None, 1, 1, 1, None) == native.LBM_E_INVALID
    assert L.lbm3d_bin_fluid_cells(None, 1, 1, 1, None) == native.LBM_E_INVALID


# ------------------------------------------------------- arithmetic pins ----

def test_one_cell_bins_are_macroscopic():
    p, obst, cells = _random2(1)
    s = lio.binned_sums(p, obst, cells, 1, 1)
    assert tuple(s) == F2 + ("fluid",)
    ux, uy, u, pressure = lio.macroscopic(p, obst, cells)
    fluid = obst == 0
    assert np.array_equal(s["fluid"], fluid.astype(np.int64)) and s["fluid"].dtype == np.int64
    for name, f in (("ux", ux), ("uy", uy), ("speed", u)):
        assert s[name].dtype == np.float64 and np.array_equal(_b64(s[name]), _b64(f.astype(np.float64))), name
    # the density is three times macroscopic's pressure only up to rounding: pin it by its own sum
    rho = np.zeros((p.ny, p.nx), np.float32)
    for k in range(9):
        rho = rho + cells[..., k]
    assert np.array_equal(_b64(s["rho"]), _b64(np.where(fluid, rho, 0).astype(np.float64)))
    # jx / rho in fp32 reproduces ux bit for bit (and jy / rho uy)
    for j, f in (("jx", ux), ("jy", uy)):
        q = s[j].astype(np.float32)[fluid] / s["rho"].astype(np.float32)[fluid]
        assert np.array_equal(_b64(s[j].astype(np.float32).astype(np.float64)), _b64(s[j])), j   # fp32 values
        assert np.array_equal(_b32(q), _b32(f[fluid])), j
    # products: exact in fp64
    for a, b in (("ux", "ux"), ("ux", "uy"), ("uy", "uy")):
        assert np.array_equal(_b64(s[a + b]), _b64(s[a] * s[b] + 0.0)), a + b
    # obstacle cells: +0 in every field
    for name in F2:
        assert not _b64(s[name])[~fluid].any(), name
    assert (~fluid).any() and fluid.any()


def test_whole_domain_density_is_the_fsum():
    p, obst, cells = _random2(2, ny=13, nx=17)
    s = lio.binned_sums(p, obst, cells, p.nx, p.ny)
    rho = np.zeros((p.ny, p.nx), np.float32)
    for k in range(9):
        rho = rho + cells[..., k]
    want = math.fsum(float(v) for v in rho[obst == 0])
    assert s["rho"].shape == (1, 1) and s["rho"][0, 0] == want
    assert s["fluid"][0, 0] == int((obst == 0).sum())


def test_ragged_bins_against_a_double_loop():
    p, obst, cells = _random2(3, ny=7, nx=10)
    obst[3:6, 4:8] = 1                                   # bin (1, 1) of (4, 3): no fluid cell
    bw, bh = 4, 3
    s = lio.binned_sums(p, obst, cells, bw, bh)
    t = lio.binned_terms(p, obst, cells)
    assert s["rho"].shape == (3, 3)
    for name in F2:
        for by in range(3):
            for bx in range(3):
                terms = [t[name][y, x] for y in range(by * bh, min(p.ny, (by + 1) * bh))
                         for x in range(bx * bw, min(p.nx, (bx + 1) * bw)) if not obst[y, x]]
                assert s[name][by, bx] == math.fsum(terms), (name, bx, by)
    assert s["fluid"][1, 1] == 0 and all(_b64(s[n])[1, 1] == 0 for n in F2)
    assert s["fluid"].sum() == int((obst == 0).sum()) and s["fluid"][2, 2] == int((obst[6:, 8:] == 0).sum())
    m = lio.binned_means(s)
    assert m["ux"][1, 1] == 0 and m["ux"][0, 0] == s["ux"][0, 0] / s["fluid"][0, 0]
    assert np.array_equal(m["fluid"], s["fluid"])


def test_binned_sums3d_pins():
    p, obst, cells = _random3(4)
    s = lio.binned_sums3d(p, obst, cells, 1, 1, 1)
    assert tuple(s) == F3 + ("fluid",)
    ux, uy, uz, u, _ = lio.macroscopic3d(p, obst, cells)
    fluid = obst == 0
    for name, f in (("ux", ux), ("uy", uy), ("uz", uz), ("speed", u)):
        assert np.array_equal(_b64(s[name]), _b64(f.astype(np.float64))), name
    for j, f in (("jx", ux), ("jy", uy), ("jz", uz)):
        q = s[j].astype(np.float32)[fluid] / s["rho"].astype(np.float32)[fluid]
        assert np.array_equal(_b32(q), _b32(f[fluid])), j
    for a, b in (("ux", "uz"), ("uy", "uz"), ("uz", "uz"), ("ux", "uy")):
        assert np.array_equal(_b64(s[a + b]), _b64(s[a] * s[b] + 0.0)), a + b
    r = lio.binned_sums3d(p, obst, cells, 3, 2, 5)          # ragged along x: 7 = 3 + 3 + 1
    assert r["rho"].shape == (1, 3, 3)
    t = lio.binned_terms3d(p, obst, cells)
    for name in F3:
        want = math.fsum(t[name][:, 2:4, 6:7].ravel().tolist())
        assert r[name][0, 1, 2] == want, name
    assert r["fluid"][0, 1, 2] == int(fluid[:, 2:4, 6:7].sum())
    whole = lio.binned_sums3d(p, obst, cells, p.nx, p.ny, p.nz)
    assert whole["fluid"][0, 0, 0] == int(fluid.sum())


# ---------------------------------------------------------------- runner ----

def test_cpu_runner_writes_binned_state(tmp_path):
    """The golden 128 x 128 problem, 50 steps, on the host backend with --binned 4x3 (ragged
    both ways: 128 = 42 * 3 + 2): binned_state.dat (lbmhost::binnedSums, fp64 sums in row
    order) equals the restatement over the oracle's cells of the same run within the
    header's bound 2 (n - 1) 2^-53 sum|term| plus the rounding of the file's %.12E, half a
    unit of its thirteenth digit: 5e-13 |value|."""
    steps, bw, bh = 50, 4, 3
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = str(steps)
    params = tmp_path / "short.params"
    params.write_text("\n".join(lines))
    p = lio.Params.from_file(str(params))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    r = subprocess.run([str(EXE), "--device", "cpu", "--binned", f"{bw}x{bh}", "--params", str(params),
                        "--obstacles", str(obst_file), "--runs", "0", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    obst = np.asarray(lio.read_obstacles(p.nx, p.ny, str(obst_file))).reshape(p.ny, p.nx)
    cells, _ = oracle.run(p, obst, steps, lio.init_cells(p))
    cells = np.asarray(cells).reshape(p.ny, p.nx, 9)
    want = lio.binned_sums(p, obst, cells, bw, bh)
    nbx, nby = -(-p.nx // bw), -(-p.ny // bh)
    got = lio.read_binned_state(str(tmp_path / "binned_state.dat"), nbx, nby)
    assert np.array_equal(got["fluid"], want["fluid"]) and 0 < want["fluid"].min() < want["fluid"].max() == bw * bh
    terms = lio.binned_terms(p, obst, cells)
    n = want["fluid"].astype(np.float64)
    for name in F2:
        mag = lio.bin_reduce(np.abs(terms[name]), (bw, bh))
        bound = 2 * np.maximum(n - 1, 0) * 2.0 ** -53 * mag + 5e-13 * np.abs(want[name])
        err = np.abs(got[name] - want[name])
        print(name, "largest error / bound", float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (name, np.argwhere(err > bound)[:4].tolist())
    assert np.abs(want["jx"]).max() > 0
    # a bin size outside 1..n is refused
    bad = subprocess.run([str(EXE), "--device", "cpu", "--binned", "129x1", "--params", str(params), "--obstacles",
                          str(obst_file), "--runs", "0", "--out-dir", str(tmp_path)], capture_output=True, text=True,
                         timeout=120)
    assert bad.returncode != 0 and "--binned" in bad.stderr
