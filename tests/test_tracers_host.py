"""Host side of the tracers and point probes (include/lbm_tracers_hip.h; CPU only).

All comparisons are bitwise: the uint64 patterns of the doubles.

* The header declares exactly native.EXPORTED_TRACERS, all exported by the
  library and disjoint from the other headers' lists; the ABI version stays 5.
* The numpy restatement the GPU tests compare against (lio.tracer_interp /
  tracer_advance / tracer_blocked and their 3-D twins) is pinned by arithmetic,
  not against itself: cell centres, exact rational arithmetic on dyadic inputs,
  uniform fields, and the order of the two schemes on a solid-body rotation.
* lbm_tracer_advance_ref / lbm_tracer_sample_ref and the 3-D twins -- the C++
  per-point functions of the kernels, compiled for the host -- equal the
  restatement bit for bit, edge seeds, multi-period wraps and non-finite field
  entries included.
* lbm_runner --device cpu --tracers writes what the restatement derives from
  the same chunked run.
"""
from __future__ import annotations

import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from conftest import GOLD, PKG, ROOT
from lbm_amd import io as lio
from lbm_amd import native
from oracle import oracle
from tracer_util import _b64, _same, seeds

EXE = PKG / "build" / "lbm_runner"
N = 1003                     # not a multiple of 64 or 256
DTS = (1.0, 10.0, -3.0, 1e6)


def fields2(seed, ny=19, nx=37, scale=0.05):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal((ny, nx))).astype(np.float32) for _ in range(3)]


def fields3(seed, nz=7, ny=9, nx=13, scale=0.05):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal((nz, ny, nx))).astype(np.float32) for _ in range(4)]


# --------------------------------------------------------------- exports ----

def test_library_exports_every_tracer_symbol():
    text = (ROOT / "include" / "lbm_tracers_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 16 and sorted(native.EXPORTED_TRACERS) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    assert L.lbm_abi_version() == 5
    others = (set(native.EXPORTED) | set(native.EXPORTED3D) | set(native.EXPORTED3D_FIELDS)
              | set(native.EXPORTED_FORCES) | set(native.EXPORTED_AVERAGES) | set(native.EXPORTED_GRADIENTS)
              | set(native.EXPORTED_STRESS) | set(native.EXPORTED_BINNED))
    assert not set(syms) & others
    assert re.search(r"\bLBM_TRACER_EULER = 0\b", text) and re.search(r"\bLBM_TRACER_HEUN = 1\b", text)
    assert (native.TRACER_EULER, native.TRACER_HEUN) == (0, 1) and lio.TRACER_SCHEMES == native.TRACER_SCHEMES
    assert re.search(rf"\bLBM_TRACER_MAX_PARTS = {native.TRACER_MAX_PARTS}\b", text)
    hpp = (PKG / "csrc" / "lbm_tracers.hpp").read_text()
    assert re.search(rf"\bBLOCK = {native.TRACER_BLOCK}\b", hpp)


def test_null_handle_is_invalid():
    L = native.load_library()
    for pre, extra in (("lbm_", ()), ("lbm3d_", (None,))):
        assert getattr(L, pre + "tracer_begin")(None, 1, None, None, *extra) == native.LBM_E_INVALID
        assert getattr(L, pre + "tracer_count")(None, None) == native.LBM_E_INVALID
        assert getattr(L, pre + "tracer_advance")(None, 1.0, 0) == native.LBM_E_INVALID
        assert getattr(L, pre + "tracer_sample")(None, None, None, None, *extra) == native.LBM_E_INVALID
        assert getattr(L, pre + "tracer_store")(None, None, None, None, *extra) == native.LBM_E_INVALID
        assert getattr(L, pre + "tracer_end")(None) == native.LBM_E_INVALID


# ------------------------------------------------------- arithmetic pins ----

def test_cell_centres_return_the_field():
    f = fields2(1)[0]
    ny, nx = f.shape
    yy, xx = np.mgrid[0:ny, 0:nx]
    got = lio.tracer_interp(f, xx.ravel().astype(np.float64), yy.ravel().astype(np.float64))
    assert got.dtype == np.float64 and _same(got, f.astype(np.float64).ravel())
    g = fields3(2)[0]
    nz, ny, nx = g.shape
    zz, yy, xx = np.mgrid[0:nz, 0:ny, 0:nx]
    got = lio.tracer_interp3d(g, *[a.ravel().astype(np.float64) for a in (xx, yy, zz)])
    assert _same(got, g.astype(np.float64).ravel())


def test_dyadic_inputs_equal_rational_arithmetic():
    """Field values and fractions that are multiples of 2^-8 in [1, 2): every product and sum of the
    interpolation is exact in fp64, so it must equal the same expression over Fractions."""
    rng = np.random.default_rng(3)
    nx, ny, nz = 11, 7, 5
    f2 = (1 + rng.integers(0, 256, (ny, nx)) / 256).astype(np.float32)
    f3 = (1 + rng.integers(0, 256, (nz, ny, nx)) / 256).astype(np.float32)
    n = 200
    x, y, z = [rng.integers(0, e, n) + rng.integers(0, 256, n) / 256 for e in (nx, ny, nz)]

    def lerp(a, b, t):
        return a + t * (b - a)

    def parts(c, e):
        i0 = int(c)
        return i0, (i0 + 1) % e, Fraction(c) - i0

    got2, got3 = lio.tracer_interp(f2, x, y), lio.tracer_interp3d(f3, x, y, z)
    for p in range(n):
        i0, i1, tx = parts(x[p], nx)
        j0, j1, ty = parts(y[p], ny)
        k0, k1, tz = parts(z[p], nz)
        F = lambda a: Fraction(float(a))
        want = lerp(lerp(F(f2[j0, i0]), F(f2[j0, i1]), tx), lerp(F(f2[j1, i0]), F(f2[j1, i1]), tx), ty)
        assert Fraction(float(got2[p])) == want, p
        pl = [lerp(lerp(F(f3[k, j0, i0]), F(f3[k, j0, i1]), tx), lerp(F(f3[k, j1, i0]), F(f3[k, j1, i1]), tx), ty)
              for k in (k0, k1)]
        assert Fraction(float(got3[p])) == lerp(pl[0], pl[1], tz), p


@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_uniform_field_moves_every_point_by_dt_u(scheme):
    rng = np.random.default_rng(4)
    nx, ny, nz = 37, 19, 7
    u = (np.float32(0.0625), np.float32(-0.03125), np.float32(0.125))       # dyadic: k1 + k2 = 2 u exactly
    x, y, z = seeds(rng, (nx, ny, nz))
    for dt in (1.0, 10.0, -3.0):
        gx, gy = lio.tracer_advance(np.full((ny, nx), u[0]), np.full((ny, nx), u[1]), x, y, dt, scheme)
        assert _same(gx, lio.tracer_wrap(x + dt * float(u[0]), nx)) and _same(gy, lio.tracer_wrap(y + dt * float(u[1]), ny))
        g3 = lio.tracer_advance3d(*[np.full((nz, ny, nx), c) for c in u], x, y, z, dt, scheme)
        for got, c, uc, e in zip(g3, (x, y, z), u, (nx, ny, nz)):
            assert _same(got, lio.tracer_wrap(c + dt * float(uc), e))
            assert (got >= 0).all() and (got < e).all()


def test_wrap_pins():
    w = lio.tracer_wrap(np.array([0.0, -0.0, 36.999, 37.0, -1.0, 74.5, np.nan, np.inf, -np.inf, 1e300, -1e-300]), 37)
    assert (w >= 0).all() and (w < 37).all()
    assert w[0] == 0 and w[3] == 0 and w[4] == 36 and w[5] == 0.5 and w[6] == 0 and w[7] == 0 and w[8] == 0
    assert w[10] == 0           # -1e-300 + 37 rounds to 37: outside [0, 37), taken to 0


def test_heun_keeps_the_radius_better_than_euler():
    n = 65
    c = (n - 1) / 2
    yy, xx = np.mgrid[0:n, 0:n]
    om = 0.02
    ux, uy = (-om * (yy - c)).astype(np.float32), (om * (xx - c)).astype(np.float32)
    ang = np.linspace(0, 2 * np.pi, 50, endpoint=False)
    x0, y0 = c + 12.3 * np.cos(ang), c + 12.3 * np.sin(ang)
    r0 = np.hypot(x0 - c, y0 - c)
    drift = {}
    for scheme in ("euler", "heun"):
        x, y = x0, y0
        for _ in range(64):
            x, y = lio.tracer_advance(ux, uy, x, y, 1.0, scheme)
        drift[scheme] = np.abs(np.hypot(x - c, y - c) - r0).max()
        assert np.hypot(x - x0, y - y0).min() > 1            # the points went round, not nowhere
    print("radius drift after 64 advances", drift)
    assert drift["heun"] < drift["euler"] and drift["euler"] > 1e-3


def test_blocked_is_the_nearest_cell():
    rng = np.random.default_rng(5)
    o2 = (rng.random((19, 37)) < 0.3).astype(np.uint8)
    o3 = (rng.random((7, 9, 13)) < 0.3).astype(np.uint8)
    x, y, z = seeds(rng, (13, 9, 7))
    x2, y2 = seeds(rng, (37, 19))
    rnd = lambda c, e: np.array([int(np.floor(v + 0.5)) % e for v in c])
    assert np.array_equal(lio.tracer_blocked(o2, x2, y2), o2[rnd(y2, 19), rnd(x2, 37)])
    got = lio.tracer_blocked3d(o3, x, y, z)
    assert got.dtype == np.uint8 and np.array_equal(got, o3[rnd(z, 7), rnd(y, 9), rnd(x, 13)]) and 0 < got.sum() < N


# ------------------------------------------------------- C against numpy ----

@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_c_reference_equals_numpy_2d(scheme):
    ux, uy, pr = fields2(6)
    x, y = seeds(np.random.default_rng(7), (37, 19))
    s = native.tracer_sample_ref(ux, uy, pr, x, y)
    for name, f in (("ux", ux), ("uy", uy), ("pressure", pr)):
        assert _same(s[name], lio.tracer_interp(f, x, y)), name
    only = native.tracer_sample_ref(None, uy, None, x, y)
    assert tuple(only) == ("uy",) and _same(only["uy"], s["uy"])
    wrapped = 0
    for dt in DTS:
        got = native.tracer_advance_ref(ux, uy, x, y, dt, scheme)
        want = lio.tracer_advance(ux, uy, x, y, dt, scheme)
        for g, w, e in zip(got, want, (37, 19)):
            assert _same(g, w), (dt, scheme)
            assert (g >= 0).all() and (g < e).all()
        wrapped += int((np.abs(x + dt * lio.tracer_interp(ux, x, y)) > 2 * 37).sum())
    assert wrapped > N // 2                                  # dt = 1e6: many periods


@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_c_reference_equals_numpy_3d(scheme):
    ux, uy, uz, pr = fields3(8)
    x, y, z = seeds(np.random.default_rng(9), (13, 9, 7))
    s = native.tracer_sample3d_ref(ux, uy, uz, pr, x, y, z)
    for name, f in (("ux", ux), ("uy", uy), ("uz", uz), ("pressure", pr)):
        assert _same(s[name], lio.tracer_interp3d(f, x, y, z)), name
    for dt in DTS:
        got = native.tracer_advance3d_ref(ux, uy, uz, x, y, z, dt, scheme)
        want = lio.tracer_advance3d(ux, uy, uz, x, y, z, dt, scheme)
        for g, w, e in zip(got, want, (13, 9, 7)):
            assert _same(g, w), (dt, scheme)
            assert (g >= 0).all() and (g < e).all()


def test_reference_entry_points_refuse_bad_arguments():
    ux, uy, pr = fields2(10)
    x, y = seeds(np.random.default_rng(11), (37, 19), n=64)
    for bad in (37.0, -1e-9, np.nan, np.inf):
        xb = x.copy()
        xb[5] = bad
        with pytest.raises(native.LbmError) as e:
            native.tracer_advance_ref(ux, uy, xb, y, 1.0, "heun")
        assert e.value.code == native.LBM_E_INVALID
        with pytest.raises(native.LbmError):
            native.tracer_sample_ref(ux, uy, pr, xb, y)
    for dt, scheme in ((np.nan, 0), (np.inf, 1), (1.0, 2), (1.0, -1)):
        with pytest.raises(native.LbmError) as e:
            native.tracer_advance_ref(ux, uy, x, y, dt, scheme)
        assert e.value.code == native.LBM_E_INVALID


def _stencil_mask(bad, idx, nxt):
    """Points one of whose stencil cells (per axis: idx or nxt) is flagged in `bad`."""
    hit = np.zeros(idx[0].shape, bool)
    for corner in np.ndindex(*(2,) * len(idx)):
        sel = tuple((nxt if c else idx)[d] for d, c in enumerate(corner))
        hit |= bad[sel[::-1]]
    return hit


@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_nonfinite_field_entries_2d_and_3d(scheme):
    """NaN, +-Inf and 1e30 entries: every coordinate stays in [0, n), the C++ functions equal the
    restatement (positions bit for bit; samples bit for bit where finite and NaN where NaN: the
    payload of a NaN an operation produces is not part of the definition), and points whose
    stencils hold only finite values move as in the clean field."""
    rng = np.random.default_rng(12)
    for dims in (2, 3):
        extent = (37, 19) if dims == 2 else (13, 9, 7)
        clean = (fields2(13) if dims == 2 else fields3(13))[:dims]
        dirty = [f.copy() for f in clean]
        bad = np.zeros(clean[0].shape, bool)
        for f in dirty:
            for v in (np.nan, np.inf, -np.inf, 1e30):
                at = tuple(int(rng.integers(0, e)) for e in f.shape)
                f[at] = v
                bad[at] = True
        pos = seeds(rng, extent)
        adv_ref = native.tracer_advance_ref if dims == 2 else native.tracer_advance3d_ref
        adv_np = lio.tracer_advance if dims == 2 else lio.tracer_advance3d
        interp = lio.tracer_interp if dims == 2 else lio.tracer_interp3d
        smp = native.tracer_sample_ref(dirty[0], dirty[1], None, *pos) if dims == 2 else \
            native.tracer_sample3d_ref(*dirty, None, *pos)
        for name, f in zip(("ux", "uy", "uz"), dirty):
            want = interp(f, *pos)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(smp[name]), nan) and nan.any(), name
            assert np.array_equal(_b64(smp[name])[~nan], _b64(want)[~nan]), name
        idx = [np.floor(c).astype(int) for c in pos]
        nxt = [(i + 1) % e for i, e in zip(idx, extent)]
        touched = _stencil_mask(bad, idx, nxt)
        assert touched.any() and not touched.all()
        for dt in DTS:
            got, want, ok = adv_ref(*dirty, *pos, dt, scheme), adv_np(*dirty, *pos, dt, scheme), adv_np(*clean, *pos, dt, scheme)
            free = ~touched
            if scheme == "heun":                                  # the midpoint's stencil counts too
                mid = [lio.tracer_wrap(c + dt * interp(f, *pos), e) for c, f, e in zip(pos, clean, extent)]
                midx = [np.floor(c).astype(int) for c in mid]
                free &= ~_stencil_mask(bad, midx, [(i + 1) % e for i, e in zip(midx, extent)])
            for g, w, c, e in zip(got, want, ok, extent):
                assert _same(g, w), (dims, dt)
                assert (g >= 0).all() and (g < e).all()
                assert np.array_equal(_b64(g)[free], _b64(c)[free]), (dims, dt)
            assert free.any()


# ---------------------------------------------------------------- runner ----

@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_cpu_runner_writes_tracers(tmp_path, scheme):
    """The golden 128 x 128 problem, 13 steps in chunks of 5 on the host backend: tracers.dat equals
    the restatement chained over the velocity fields of the same run after 5, 10 and 13 steps
    (dt 5, 5, 3), the positions read back with float() and compared as uint64."""
    steps, every = 13, 5
    lines = (GOLD / "params" / "input_128x128.params").read_text().split("\n")
    lines[2] = str(steps)
    params = tmp_path / "short.params"
    params.write_text("\n".join(lines))
    p = lio.Params.from_file(str(params))
    obst_file = GOLD / "params" / "obstacles_128x128.dat"
    obst = np.asarray(lio.read_obstacles(p.nx, p.ny, str(obst_file))).reshape(p.ny, p.nx)
    x, y = seeds(np.random.default_rng(14), (p.nx, p.ny), n=257)
    (tmp_path / "seeds.txt").write_text("".join(f"{a!r} {b!r}\n" for a, b in zip(x.tolist(), y.tolist())))
    r = subprocess.run([str(EXE), "--device", "cpu", "--tracers", str(tmp_path / "seeds.txt"), "--trace-every",
                        str(every), "--trace-scheme", scheme, "--params", str(params), "--obstacles", str(obst_file),
                        "--runs", "0", "--out-dir", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    cells0 = lio.init_cells(p)
    done = 0
    while done < steps:
        n = min(every, steps - done)
        done += n
        cells, _ = oracle.run(p, obst, done, cells0)
        ux, uy, _, _ = lio.macroscopic(p, obst, np.asarray(cells).reshape(p.ny, p.nx, 9))
        x, y = lio.tracer_advance(ux, uy, x, y, float(n), scheme)
    gx, gy, gb = lio.read_tracers(str(tmp_path / "tracers.dat"))
    assert _same(gx, x) and _same(gy, y)
    assert np.array_equal(gb, lio.tracer_blocked(obst, x, y))
    text = (tmp_path / "tracers.dat").read_text().split("\n")
    assert text[0].split()[0] == "0" and len([t for t in text if t]) == 257
    # the chunked run is the plain run: the same av_vels.dat and final_state.dat as without --tracers
    plain = tmp_path / "plain"
    plain.mkdir()
    r = subprocess.run([str(EXE), "--device", "cpu", "--params", str(params), "--obstacles", str(obst_file),
                        "--runs", "0", "--out-dir", str(plain)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for name in ("av_vels.dat", "final_state.dat"):
        assert (plain / name).read_bytes() == (tmp_path / name).read_bytes(), name
    assert not (plain / "tracers.dat").exists()
    # a seed outside the grid is refused
    (tmp_path / "bad.txt").write_text("128.0 3.0\n")
    bad = subprocess.run([str(EXE), "--device", "cpu", "--tracers", str(tmp_path / "bad.txt"), "--params", str(params),
                          "--obstacles", str(obst_file), "--runs", "0", "--out-dir", str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "tracer" in bad.stderr
