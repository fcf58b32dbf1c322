"""Host side of the time averages (include/lbm_averages_hip.h; CPU only).

* The header declares exactly native.EXPORTED_AVERAGES, 12 symbols, all
  exported by the library and disjoint from the other headers' lists.
* Every entry point answers a NULL handle with LBM_E_INVALID.
* The numpy restatement the GPU tests compare against (lio.moment_sums /
  lio.moment_means) is pinned by arithmetic, not against itself: sums of
  n <= 16 fp32 terms of one binade and of their 48-bit products are exact in
  fp64, so they must equal the exact rational sums (fractions.Fraction) bit
  for bit; n identical samples give mean == sample and central moments of
  exactly +0.
* lbm_runner --device cpu --mean-every is refused: the option is GPU-only.
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

EXE = PKG / "build" / "lbm_runner"


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --------------------------------------------------------------- exports ----

def test_library_exports_every_average_symbol():
    text = (ROOT / "include" / "lbm_averages_hip.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    syms = sorted(set(re.findall(r"\b(lbm(?:3d)?_[a-z_0-9]+)\s*\(", text)))
    assert len(syms) == 12 and sorted(native.EXPORTED_AVERAGES) == syms
    L = native.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    assert L.lbm_abi_version() == 5
    others = (set(native.EXPORTED) | set(native.EXPORTED3D) | set(native.EXPORTED3D_FIELDS)
              | set(native.EXPORTED_FORCES))
    assert not set(syms) & others


def test_field_name_lists_follow_the_header_enums():
    text = (ROOT / "include" / "lbm_averages_hip.h").read_text()
    for prefix, names in (("LBM_AVG_", native.AVG_FIELDS), ("LBM3D_AVG_", native.AVG_FIELDS3D)):
        for i, n in enumerate(names):
            tag = "P" if n == "pressure" else n.upper()
            assert re.search(rf"\b{prefix}{tag} = {i}\b", text), (prefix, n)
        assert re.search(rf"\b{prefix}FIELDS = {len(names)}\b", text)
    assert len(native.AVG_FIELDS) == 7 and len(native.AVG_FIELDS3D) == 11
    assert re.search(r"\bLBM_AVG_MEAN = 1\b", text) and re.search(r"\bLBM_AVG_SECOND = 2\b", text)
    assert (native.AVG_MEAN, native.AVG_SECOND) == (1, 2)


def test_null_handle_is_invalid():
    L = native.load_library()
    for prefix in ("lbm_", "lbm3d_"):
        assert getattr(L, prefix + "avg_begin")(None, 3) == native.LBM_E_INVALID
        assert getattr(L, prefix + "avg_sample")(None) == native.LBM_E_INVALID
        assert getattr(L, prefix + "avg_samples")(None, None) == native.LBM_E_INVALID
        assert getattr(L, prefix + "avg_store_sums")(None, None) == native.LBM_E_INVALID
        assert getattr(L, prefix + "avg_store")(None, None) == native.LBM_E_INVALID
        assert getattr(L, prefix + "avg_end")(None) == native.LBM_E_INVALID


# ----------------------------------------------------------- restatement ----

def _random_samples(rng, n, nv, shape):
    """n samples of nv velocity components and a pressure: full 24-bit random mantissas
    and random signs, each cell and field staying in one binade [2^e, 2^(e+1)) (e random
    per cell and field, -20 .. 0) over the samples.  Then a sum of n <= 16 terms spans at
    most 24 + 4 bits, and a sum of products a * b (each in [2^(ea+eb), 2^(ea+eb+2)), 48
    bits) at most 48 + 2 + 4 - 2 = 52 bits: every partial sum is exact in fp64."""
    expo = [rng.integers(-20, 1, shape) for _ in range(nv + 1)]
    out = []
    for _ in range(n):
        s = []
        for k in range(nv + 1):
            mant = rng.integers(1 << 23, 1 << 24, shape).astype(np.float64)
            sign = np.where(rng.random(shape) < 0.5, -1.0, 1.0) if k < nv else 1.0
            v = (sign * np.ldexp(mant, expo[k] - 23)).astype(np.float32)
            assert np.array_equal(v.astype(np.float64), sign * np.ldexp(mant, expo[k] - 23))
            s.append(v)
        out.append(s)
    return out


def _exact(values):
    """The exact rational sum, rounded once to fp64 (float(Fraction) rounds to nearest even)."""
    return float(sum(values, Fraction(0)))


@pytest.mark.parametrize("nv,n", [(2, 1), (2, 5), (2, 16), (3, 7), (3, 16)])
def test_moment_sums_equal_the_exact_rational_sums(nv, n):
    rng = np.random.default_rng(1000 * nv + n)
    shape = (3, 5)
    samples = _random_samples(rng, n, nv, shape)
    sums = lio.moment_sums(samples, True)
    first = nv + 1
    pairs = [(i, j) for i in range(nv) for j in range(i, nv)] + [(nv, nv)]
    assert len(sums) == first + len(pairs) == (7 if nv == 2 else 11)
    assert [s.dtype for s in sums] == [np.float64] * len(sums)
    assert len(lio.moment_sums(samples, False)) == first
    for idx in np.ndindex(*shape):
        vals = [[Fraction(float(s[k][idx])) for k in range(first)] for s in samples]
        for k in range(first):
            want = _exact([v[k] for v in vals])
            assert _bits64(sums[k][idx]) == _bits64(want), (k, idx)
        for f, (a, b) in enumerate(pairs):
            want = _exact([v[a] * v[b] for v in vals])
            assert _bits64(sums[first + f][idx]) == _bits64(want), (a, b, idx)
    for a, b in zip(lio.moment_sums(samples, False), sums[:first]):
        assert np.array_equal(_bits64(a), _bits64(b))


@pytest.mark.parametrize("nv", [2, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 8, 16])
def test_identical_samples_give_the_sample_and_zero_moments(nv, n):
    """n S / n and n S^2 / n - S S are exact for n <= 16: n x is x shifted or a
    short sum of shifts of a 24-bit number, x * x has 48 bits."""
    rng = np.random.default_rng(7 * nv + n)
    one = _random_samples(rng, 1, nv, (4, 6))[0]
    means = lio.moment_means(lio.moment_sums([one] * n, True), n)
    assert [m.dtype for m in means] == [np.float32] * len(means)
    for k in range(nv + 1):
        assert np.array_equal(_bits32(means[k]), _bits32(one[k])), k
    for m in means[nv + 1:]:
        assert not _bits32(m).any()       # exactly +0
    only = lio.moment_means(lio.moment_sums([one] * n, False), n)
    assert len(only) == nv + 1


def test_moment_means_definition_on_a_worked_cell():
    # samples 1, 2, 4 and pressures 0.5, 0.25, 0.25: mean 7/3, <uu> - <u><u> = 7 - 49/9
    s = [[np.float32([u]), np.float32([-u]), np.float32([p])] for u, p in ((1, .5), (2, .25), (4, .25))]
    sums = lio.moment_sums(s, True)
    assert [float(v[0]) for v in sums] == [7.0, -7.0, 1.0, 21.0, -21.0, 21.0, 0.375]
    m = lio.moment_means(sums, 3)
    d = np.float64
    mean = d(7.0) / d(3.0)
    assert _bits32(m[0]) == _bits32(np.float32(mean))
    assert _bits32(m[3]) == _bits32(np.float32(d(21.0) / d(3.0) - mean * mean))
    assert _bits32(m[4]) == _bits32(np.float32(d(-21.0) / d(3.0) - mean * -mean))
    assert _bits32(m[6]) == _bits32(np.float32(d(0.375) / d(3.0) - (d(1.0) / d(3.0)) * (d(1.0) / d(3.0))))


# ---------------------------------------------------------------- runner ----

def test_cpu_device_refuses_mean_every(tmp_path):
    r = subprocess.run([str(EXE), "--device", "cpu", "--mean-every", "10", "--params",
                        str(GOLD / "params" / "input_128x128.params"), "--obstacles",
                        str(GOLD / "params" / "obstacles_128x128.dat"), "--runs", "0", "--out-dir", str(tmp_path)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "GPU-only" in r.stderr and "--mean-every" in r.stderr
    assert not (tmp_path / "final_state.dat").exists() and not (tmp_path / "mean_state.dat").exists()
