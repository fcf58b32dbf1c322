"""What the transport-sum tests share (tests/test_transport_host.py, tests/test_gpu_transport*.py); no
test lives here: the fold bound of DESIGN 4.14 per bin, the comparison of a device result with the numpy
restatement, and the Rayleigh-Benard plane sums with the figures the CPU loop gave.
"""
from __future__ import annotations

import numpy as np

import thermal_cases as tc
from lbm_amd import io as lio

# Rayleigh-Benard, thermal_cases.rayleigh_benard(3000) after 6000 steps of thermal_cases.cpu_thermal: the mean
# over the planes y = 1 .. 19 of sum_x FY / (D nx / 19), as tests/test_transport_host.py measures and pins it
RB_STEPS = 6000
RB_NU_CPU = 1.88762
RB_FLAT = 1e-4          # spread of the plane sums over their mean: seven times the 1.4e-5 measured


def b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def rb_unit():
    """D nx / 19: what conduction carries through a plane of the Rayleigh-Benard set-up for a unit scalar
    difference over the 19 cells between the fixed rows."""
    return lio.scalar_diffusivity(tc.RB_OMEGA, 2) * tc.RB_NX / 19.0


def fold_bounds(terms, obst, bins):
    """{name: float64 per bin}: 2 (n - 1) 2^-53 sum|term| with n the contributing cells of the bin: every
    cell for the face fluxes ("f?"), the fluid cells for the rest."""
    shape = next(iter(terms.values())).shape
    fluid = (np.asarray(obst).reshape(shape) == 0).astype(np.int64)
    out = {}
    for name, t in terms.items():
        n = lio.bin_reduce(np.ones_like(fluid) if name[0] == "f" else fluid, bins, exact=False)
        out[name] = 2.0 * np.maximum(n - 1, 0) * 2.0 ** -53 * lio.bin_reduce(np.abs(t), bins)
    return out


def check_binned(got, terms, obst, bins, what=""):
    """A device result against the restatement: bitwise at one-cell bins, else within the fold bound of
    the math.fsum value; "fluid" exact.  `got` may hold a subset of the fields."""
    one = all(int(b) == 1 for b in bins)
    bounds = None if one else fold_bounds(terms, obst, bins)
    shape = next(iter(terms.values())).shape
    fluid = (np.asarray(obst).reshape(shape) == 0).astype(np.int64)
    for name, a in got.items():
        if name == "fluid":
            assert np.array_equal(a, lio.bin_reduce(fluid, bins, exact=False)), (what, name)
            continue
        want = lio.bin_reduce(terms[name], bins)
        assert a.dtype == np.float64 and a.shape == want.shape, (what, name, a.shape, want.shape)
        if one:
            bad = b64(a) != b64(want)
            assert not bad.any(), (what, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
        else:
            err = np.abs(a - want)
            assert (err <= bounds[name]).all(), (what, name, float(err.max()), float(bounds[name].max()))
