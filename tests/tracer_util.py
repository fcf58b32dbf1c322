"""What the tracer tests share (test_tracers_host.py, test_gpu_tracers.py, test_gpu_tracers3d.py):
the bitwise comparison of doubles and the seed points with their edge cases."""
from __future__ import annotations

import numpy as np

N = 1003                     # not a multiple of 64 or 256
SENTINEL64 = 0x7FF8000000000001   # a quiet NaN pattern no computation produces


def _b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    return np.array_equal(_b64(a), _b64(b))


def seeds(rng, extent, n=N):
    """n points in the box `extent` (x first): random ones, then exact cell centres, 0, points in
    [n_c - 1, n_c), nextafter(n_c, 0) and the corner cell (its 3-D analogue), on every axis."""
    dims = len(extent)
    pts = [rng.random(n) * e for e in extent]
    k = 0
    for i in range(40):                                          # exact cell centres
        for d in range(dims):
            pts[d][k] = float(rng.integers(0, extent[d]))
        k += 1
    for d in range(dims):                                        # one coordinate on an edge value
        for v in (0.0, extent[d] - 1.0, extent[d] - 0.25, np.nextafter(float(extent[d]), 0.0)):
            pts[d][k] = v
            k += 1
    for v in (lambda e: 0.0, lambda e: e - 0.5, lambda e: np.nextafter(float(e), 0.0), lambda e: e - 1.0):
        for d in range(dims):                                    # every coordinate at once: the corner cell
            pts[d][k] = v(extent[d])
        k += 1
    assert k < n
    return pts
