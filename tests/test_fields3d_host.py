"""Host side of the D3Q19 device-fields path (CPU only).

* include/lbm3d_fields_hip.h declares exactly native.EXPORTED3D_FIELDS, the
  library exports them, lbm3d_hip.h keeps its 13 symbols, and each new entry
  point refuses a NULL handle.
* The definition of the fields (lio.macroscopic3d, the numpy restatement the
  GPU tests compare against) is pinned to the oracle bit for bit: the
  sequential fp32 sum of its |u| over the pulled populations is the `tot`
  oracle3d_step forms from the same lattice.
* Equilibrium at rest: zero velocity bits, pressure = sequential sum / 3.
"""
from __future__ import annotations

import ctypes
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from lbm_amd import io as lio
from lbm_amd import native
from oracle import oracle

CX = np.array([0, 1, -1, 0, 0, 1, -1, 1, -1, 0, 1, -1, 0, 0, 0, -1, 1, 0, 0])
CY = np.array([0, 0, 0, 1, -1, 1, -1, -1, 1, 0, 0, 0, 1, -1, 0, 0, 0, -1, 1])
CZ = np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1])


def header_symbols(name, prefix):
    text = (ROOT / "include" / name).read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(rf"\b({prefix}[a-z_0-9]+)\s*\(", text)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_fields_header_and_exports():
    L = native.load_library()
    syms = header_symbols("lbm3d_fields_hip.h", "lbm3d_")
    assert syms == sorted(native.EXPORTED3D_FIELDS)
    assert len(syms) == 3
    out = subprocess.run(["nm", "-D", "--defined-only", str(native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    for s in syms:
        assert hasattr(L, s), s
        assert re.search(rf"\bT {s}\b", out), s
    # the engine's own header is unchanged: the new names are no part of it
    base = header_symbols("lbm3d_hip.h", "lbm3d_")
    assert len(base) == 13 and sorted(native.EXPORTED3D) == base
    assert not set(base) & set(syms)
    assert native.FIELDS3D == ("ux", "uy", "uz", "speed", "pressure")


def test_null_handle_is_invalid():
    L = native.load_library()
    buf = np.zeros(8, np.float32)
    f = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    box = native.Box3D(0, 0, 0, 1, 1, 1)
    mass, umax = ctypes.c_double(), ctypes.c_float()
    assert L.lbm3d_store_fields(None, f, f, f, f, f) == native.LBM_E_INVALID
    assert L.lbm3d_store_fields_box(None, ctypes.byref(box), f, f, f, f, f) == native.LBM_E_INVALID
    assert L.lbm3d_field_stats(None, ctypes.byref(mass), ctypes.byref(umax)) == native.LBM_E_INVALID
    assert not buf.any()


@pytest.mark.parametrize("nx,ny,nz", [(13, 9, 7), (67, 5, 3), (4, 4, 4), (130, 3, 2)])
def test_macroscopic3d_is_the_oracles_speed_bitwise(nx, ny, nz):
    """|u| of macroscopic3d on the pulled populations, summed sequentially in fp32
    in (z, y, x) order, has the bit pattern of oracle3d_step's `tot` (obstacle
    cells contribute +0 here, nothing there)."""
    p = lio.Params3D(nx, ny, nz, 0, 0.1, 0.002, 1.7)
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    obst = (rng.random((nz, ny, nx)) < 0.10).astype(np.uint8)
    c0 = (oracle.init_cells3d(p) * (1 + 0.05 * rng.standard_normal((nz, ny, nx, 19)))).astype(np.float32)
    pulled = np.stack([np.roll(c0[..., k], (CZ[k], CY[k], CX[k]), axis=(0, 1, 2)) for k in range(19)], axis=-1)
    speed = lio.macroscopic3d(p, obst, pulled)[3]
    assert not speed[obst != 0].any() and np.all(speed[obst == 0] > 0)
    mine = np.cumsum(speed.ravel(), dtype=np.float32)[-1]
    out = np.empty_like(c0)
    f32p, u8p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_uint8)
    L = oracle.lib()
    tot = L.oracle3d_step(ctypes.byref(oracle._p3(p)), c0.ctypes.data_as(f32p), out.ctypes.data_as(f32p),
                          np.ascontiguousarray(obst).ctypes.data_as(u8p))
    assert bits(mine) == bits(np.float32(tot)), (float(mine), float(tot))


def test_macroscopic3d_equilibrium_at_rest():
    p = lio.Params3D(6, 5, 4, 0, 0.7, 0.0, 1.0)
    c = oracle.init_cells3d(p)
    obst = lio.channel_obstacles3d(6, 5, 4)
    ux, uy, uz, speed, pressure = lio.macroscopic3d(p, obst, c)
    for f in (ux, uy, uz, speed):
        assert f.dtype == np.float32 and f.shape == (4, 5, 6)
        assert not bits(f).any()
    rho = np.float32(0) + c[0, 0, 0, 0]
    for k in range(1, 19):
        rho = np.float32(rho + c[0, 0, 0, k])
    third = np.float32(1) / np.float32(3)
    assert np.all(bits(pressure[obst == 0]) == bits(np.float32(rho * third)))
    assert np.all(bits(pressure[obst != 0]) == bits(np.float32(p.density) * third))
