"""ctypes binding of liblbm_hip.so (the C ABI declared in include/lbm_hip.h).

This is the Python-side mirror of the reference host's Engine usage
(main/LbmRunner.cpp:81-144): create/load/run/store/timer.  It is also the
binding a maintainer would add on the reference side.

There is deliberately no CPU fallback: if the HIP library is missing or no
GPU is visible the calls fail loudly.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

PKG_ROOT = Path(__file__).resolve().parent.parent          # lbm-graphcore_amd/
LIB_PATH = Path(os.environ.get("LBM_HIP_LIB", PKG_ROOT / "build" / "liblbm_hip.so"))

Q = 9
ABI_VERSION = 5          # LBM_ABI_VERSION in include/lbm_hip.h

LBM_OK = 0
LBM_E_INVALID, LBM_E_HIP, LBM_E_RCCL, LBM_E_NOMEM, LBM_E_STATE, LBM_E_INTERNAL = -1, -2, -3, -4, -5, -6
TRANSPORT_LOCAL, TRANSPORT_RCCL = 0, 1
KERNEL_AUTO, KERNEL_SCALAR, KERNEL_VEC4, KERNEL_STEP2, KERNEL_STREAM, KERNEL_RESIDENT, KERNEL_PIPELINE = range(7)
FLAG_FORCE_EXCHANGE, FLAG_ONE_STEP, FLAG_TOLERANCE, FLAG_PROFILE = 1, 2, 4, 8
XFER_SEND, XFER_RECV, XFER_SELF = 0, 1, 2
HALO_W1, HALO_WG = 1, 2
FIELDS = ("ux", "uy", "speed", "pressure")   # argument order of lbm_store_fields

# every symbol include/lbm_hip.h declares
EXPORTED = [
    "lbm_abi_version", "lbm_partition", "lbm_halo_plan", "lbm_exchange_schedule", "lbm_device_count",
    "lbm_rccl_unique_id",
    "lbm_create", "lbm_create_ex", "lbm_load_cells", "lbm_init_equilibrium",
    "lbm_run", "lbm_run_steps", "lbm_store", "lbm_load_cells_local", "lbm_store_local", "lbm_local_cells",
    "lbm_store_fields", "lbm_store_fields_local", "lbm_field_stats",
    "lbm_last_run_seconds",
    "lbm_total_free_cells", "lbm_local_rects", "lbm_kernel_in_use", "lbm_steps_per_launch",
    "lbm_run_stats", "lbm_stream_units", "lbm_profile_summary", "lbm_profile_reset", "lbm_placement_probe", "lbm_numerics", "lbm_nonfinite_count", "lbm_source_hash",
    "lbm_last_error", "lbm_destroy",
]
# every symbol include/lbm3d_hip.h declares (D3Q19 extension)
EXPORTED3D = [
    "lbm3d_create", "lbm3d_init_equilibrium", "lbm3d_load_cells", "lbm3d_run_steps", "lbm3d_store",
    "lbm3d_last_run_seconds", "lbm3d_total_free_cells", "lbm3d_local_slabs", "lbm3d_exchange_schedule",
    "lbm3d_run_stats", "lbm3d_numerics",
    "lbm3d_last_error", "lbm3d_destroy",
]
# every symbol include/lbm3d_fields_hip.h declares (D3Q19 fields, box extracts, stats)
EXPORTED3D_FIELDS = ["lbm3d_store_fields", "lbm3d_store_fields_box", "lbm3d_field_stats"]
FIELDS3D = ("ux", "uy", "uz", "speed", "pressure")   # argument order of lbm3d_store_fields
# every symbol include/lbm_forces_hip.h declares (momentum-exchange wall forces, both engines)
EXPORTED_FORCES = [
    "lbm_wall_force", "lbm_store_wall_force", "lbm_set_bodies", "lbm_body_forces",
    "lbm3d_wall_force", "lbm3d_store_wall_force", "lbm3d_set_bodies", "lbm3d_body_forces",
]
# every symbol include/lbm_averages_hip.h declares (time-averaged fields and Reynolds stresses, both engines)
EXPORTED_AVERAGES = [
    "lbm_avg_begin", "lbm_avg_sample", "lbm_avg_samples", "lbm_avg_store_sums", "lbm_avg_store", "lbm_avg_end",
    "lbm3d_avg_begin", "lbm3d_avg_sample", "lbm3d_avg_samples", "lbm3d_avg_store_sums", "lbm3d_avg_store",
    "lbm3d_avg_end",
]
# index order of the output-pointer arrays (LBM_AVG_* / LBM3D_AVG_*): first moments, then second moments
AVG_FIELDS = ("ux", "uy", "pressure", "uxux", "uxuy", "uyuy", "pp")
AVG_FIELDS3D = ("ux", "uy", "uz", "pressure", "uxux", "uxuy", "uxuz", "uyuy", "uyuz", "uzuz", "pp")
AVG_MEAN, AVG_SECOND = 1, 2
# every symbol include/lbm_gradients_hip.h declares (vorticity, divergence, strain rate, Q; both engines)
EXPORTED_GRADIENTS = [
    "lbm_store_gradients", "lbm_store_gradients_local", "lbm_gradient_stats",
    "lbm3d_store_gradients", "lbm3d_store_gradients_box", "lbm3d_gradient_stats",
]
# index order of the output-pointer arrays (LBM_GRAD_* / LBM3D_GRAD_*)
GRAD_FIELDS = ("vorticity", "divergence", "strain", "q")
GRAD_FIELDS3D = ("wx", "wy", "wz", "vorticity", "divergence", "strain", "q")
# work shape of the D2Q9 gradient kernel (csrc/lbm_gradients.hpp): columns a wave owns, rows of a segment
GRAD_STRIP_COLS, GRAD_SEGMENT_ROWS = 248, 32
# every symbol include/lbm_stress_hip.h declares (non-equilibrium strain rate and wall shear; both engines)
EXPORTED_STRESS = [
    "lbm_store_stress", "lbm_store_stress_local", "lbm_stress_stats",
    "lbm3d_store_stress", "lbm3d_store_stress_box", "lbm3d_stress_stats",
]
# index order of the output-pointer arrays (LBM_STRESS_* / LBM3D_STRESS_*)
STRESS_FIELDS = ("sxx", "sxy", "syy", "strain")
STRESS_FIELDS3D = ("sxx", "syy", "szz", "sxy", "sxz", "syz", "strain")
# work units of the strain-rate kernels (csrc/lbm_stress.hpp).  D2Q9: cells of a lane's quad, and
# consecutive quads (row-major over ceil(w / 4) quads per row) a block owns.  D3Q19: cells along x,
# rows and planes a block owns on the 16-B path (one cell per lane: STRESS3D_BLOCK[0] / 4 along x).
STRESS_QUAD, STRESS_BLOCK_QUADS = 4, 2048
STRESS3D_BLOCK = (256, 4, 8)
# every symbol include/lbm_binned_hip.h declares (sums over rectangular bins; both engines)
EXPORTED_BINNED = ["lbm_store_binned", "lbm_bin_fluid_cells", "lbm3d_store_binned", "lbm3d_bin_fluid_cells"]
# index order of the output-pointer arrays (LBM_BIN_* / LBM3D_BIN_*)
BIN_FIELDS = ("rho", "jx", "jy", "ux", "uy", "speed", "uxux", "uxuy", "uyuy")
BIN_FIELDS3D = ("rho", "jx", "jy", "jz", "ux", "uy", "uz", "speed",
                "uxux", "uxuy", "uxuz", "uyuy", "uyuz", "uzuz")
# work units of the binned-sum kernels (csrc/lbm_binned.hpp).  D2Q9: cells of a lane's quad, columns
# of a wave, most rows of a chunk (a chunk never straddles a bin).  D3Q19: columns of a wave (one cell
# per lane); a chunk is at most BIN_CHUNK_ROWS planes.
BIN_QUAD, BIN_WAVE_COLS, BIN_CHUNK_ROWS = 4, 256, 32
BIN3D_WAVE_COLS = 64
# every symbol include/lbm_tracers_hip.h declares (Lagrangian tracers and point probes; both engines)
EXPORTED_TRACERS = [
    "lbm_tracer_begin", "lbm_tracer_count", "lbm_tracer_advance", "lbm_tracer_sample", "lbm_tracer_store",
    "lbm_tracer_end", "lbm_tracer_advance_ref", "lbm_tracer_sample_ref",
    "lbm3d_tracer_begin", "lbm3d_tracer_count", "lbm3d_tracer_advance", "lbm3d_tracer_sample",
    "lbm3d_tracer_store", "lbm3d_tracer_end", "lbm3d_tracer_advance_ref", "lbm3d_tracer_sample_ref",
]
TRACER_EULER, TRACER_HEUN = 0, 1          # LBM_TRACER_EULER / LBM_TRACER_HEUN
TRACER_SCHEMES = {"euler": TRACER_EULER, "heun": TRACER_HEUN}
TRACER_MAX_PARTS = 16                     # LBM_TRACER_MAX_PARTS
TRACER_BLOCK = 256                        # lanes (= points) per block of the tracer kernels (csrc/lbm_tracers.hpp)
# names of tracer_sample()'s arrays, in the argument order of lbm_tracer_sample / lbm3d_tracer_sample
TRACER_FIELDS = ("ux", "uy", "pressure")
TRACER_FIELDS3D = ("ux", "uy", "uz", "pressure")
# every symbol include/lbm_scalar_hip.h declares (passive scalar: D2Q5 beside D2Q9, D3Q7 beside D3Q19)
EXPORTED_SCALAR = [
    "lbm_scalar_begin", "lbm_scalar_set_fixed", "lbm_scalar_advance", "lbm_scalar_steps", "lbm_scalar_store",
    "lbm_scalar_stats", "lbm_scalar_end", "lbm_scalar_step_ref",
    "lbm3d_scalar_begin", "lbm3d_scalar_set_fixed", "lbm3d_scalar_advance", "lbm3d_scalar_steps",
    "lbm3d_scalar_store", "lbm3d_scalar_stats", "lbm3d_scalar_end", "lbm3d_scalar_step_ref",
]
SCALAR_MAX_PARTS = 16                     # LBM_SCALAR_MAX_PARTS
# every symbol include/lbm_thermal_hip.h declares (Boussinesq buoyancy: the scalar's kick on the flow)
EXPORTED_THERMAL = [
    "lbm_scalar_buoyancy", "lbm_scalar_buoyancy_ref", "lbm3d_scalar_buoyancy", "lbm3d_scalar_buoyancy_ref",
]
SCALAR_Q, SCALAR_Q3D = 5, 7               # populations per cell of the scalar lattice
# every symbol include/lbm_transport_hip.h declares (binned transport sums of the scalar; both engines)
EXPORTED_TRANSPORT = [
    "lbm_scalar_store_binned", "lbm3d_scalar_store_binned", "lbm_scalar_terms_ref", "lbm3d_scalar_terms_ref",
]
# index order of the output-pointer arrays (LBM_SBIN_* / LBM3D_SBIN_*)
SBIN_FIELDS = ("phi", "phiphi", "uxphi", "uyphi", "fx", "fy")
SBIN_FIELDS3D = ("phi", "phiphi", "uxphi", "uyphi", "uzphi", "fx", "fy", "fz")
# every symbol include/lbm_scalar_walls_hip.h declares (scalar wall models and the per-body wall flux; both engines)
EXPORTED_WALLS = [
    "lbm_scalar_set_walls", "lbm_scalar_wall_flux", "lbm_scalar_body_flux", "lbm_scalar_store_wall_flux",
    "lbm_scalar_walls_ref",
    "lbm3d_scalar_set_walls", "lbm3d_scalar_wall_flux", "lbm3d_scalar_body_flux", "lbm3d_scalar_store_wall_flux",
    "lbm3d_scalar_walls_ref",
]
# every symbol include/lbm_forcing_hip.h declares (forcing zones: body force, drag, velocity target; both engines)
EXPORTED_FORCING = [
    "lbm_forcing_set_zone", "lbm_forcing_clear", "lbm_forcing_zones", "lbm_forcing_apply", "lbm_forcing_kick_ref",
    "lbm3d_forcing_set_zone", "lbm3d_forcing_clear", "lbm3d_forcing_zones", "lbm3d_forcing_apply",
    "lbm3d_forcing_kick_ref",
]
FORCING_MAX_ZONES = 8                     # LBM_FORCING_MAX_ZONES
# every symbol include/lbm_sgs_hip.h declares (sub-grid model: Smagorinsky, prescribed local rate; both engines)
EXPORTED_SGS = [
    "lbm_sgs_set", "lbm_sgs_apply", "lbm_sgs_store_nut", "lbm_sgs_filter_ref",
    "lbm3d_sgs_set", "lbm3d_sgs_apply", "lbm3d_sgs_store_nut", "lbm3d_sgs_filter_ref",
]
SGS_OFF, SGS_SMAGORINSKY, SGS_OMEGA = 0, 1, 2                            # LBM_SGS_*
SGS_MODES = {"off": SGS_OFF, "smagorinsky": SGS_SMAGORINSKY, "omega": SGS_OMEGA}
SCALAR_WALL_ADIABATIC, SCALAR_WALL_VALUE, SCALAR_WALL_FLUX = 0, 1, 2   # LBM_SCALAR_WALL_*
SCALAR_WALL_KINDS = {"adiabatic": SCALAR_WALL_ADIABATIC, "value": SCALAR_WALL_VALUE, "flux": SCALAR_WALL_FLUX}
Q3 = 19


class LbmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"lbm error {code}: {msg}")
        self.code = code


class Params(ctypes.Structure):
    """lbm_params (mirror of lbm::Params, main/include/LbmParams.hpp:16-65)."""
    _fields_ = [
        ("nx", ctypes.c_int32),
        ("ny", ctypes.c_int32),
        ("max_iters", ctypes.c_int32),
        ("reynolds_dim", ctypes.c_int32),
        ("density", ctypes.c_float),
        ("accel", ctypes.c_float),
        ("omega", ctypes.c_float),
    ]


class Config(ctypes.Structure):
    _fields_ = [
        ("parts", ctypes.c_int32),
        ("grid_rows", ctypes.c_int32),
        ("grid_cols", ctypes.c_int32),
        ("transport", ctypes.c_int32),
        ("rank", ctypes.c_int32),
        ("world", ctypes.c_int32),
        ("devices", ctypes.POINTER(ctypes.c_int32)),
        ("num_devices", ctypes.c_int32),
        ("rccl_unique_id", ctypes.POINTER(ctypes.c_uint8)),
        ("kernel", ctypes.c_int32),
        ("graph_steps", ctypes.c_int32),
        ("flags", ctypes.c_int32),
        ("steps_per_launch", ctypes.c_int32),
    ]


class Params3D(ctypes.Structure):
    """lbm3d_params (include/lbm3d_hip.h)."""
    _fields_ = [("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32), ("max_iters", ctypes.c_int32),
                ("density", ctypes.c_float), ("accel", ctypes.c_float), ("omega", ctypes.c_float)]


class Box3D(ctypes.Structure):
    """lbm3d_box (include/lbm3d_fields_hip.h): cells [x0, x0+nx) x [y0, y0+ny) x [z0, z0+nz)."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("z0", ctypes.c_int32),
                ("nx", ctypes.c_int32), ("ny", ctypes.c_int32), ("nz", ctypes.c_int32)]


class Rect(ctypes.Structure):
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32)]


class KernelTime(ctypes.Structure):
    """lbm_kernel_time (include/lbm_hip.h)."""
    _fields_ = [("name", ctypes.c_char * 64), ("launches", ctypes.c_int64), ("total_ms", ctypes.c_double),
                ("min_ms", ctypes.c_double), ("max_ms", ctypes.c_double)]


class StreamUnit(ctypes.Structure):
    """lbm_stream_unit (include/lbm_hip.h): one work unit of the stream kernel."""
    _fields_ = [("sub", ctypes.c_int32), ("boundary", ctypes.c_int32), ("x0", ctypes.c_int32),
                ("y0", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32),
                ("reads_obstacle", ctypes.c_int32)]


class Xfer(ctypes.Structure):
    """lbm_xfer (include/lbm_hip.h): one post of a halo exchange."""
    _fields_ = [("op", ctypes.c_int32), ("dir", ctypes.c_int32), ("peer", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("floats", ctypes.c_int64)]


_lib = None


def load_library() -> ctypes.CDLL:
    """Load liblbm_hip.so and declare every C-ABI signature (no GPU needed).

    Refuses a library whose compiled-in source hash (lbm_source_hash) differs
    from the hash of the csrc/ and include/ sources beside it: a stale build
    fails loudly instead of silently running old kernels."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise FileNotFoundError(
            f"{LIB_PATH} not found: build the HIP library first (make -C lbm-graphcore_amd "
            "or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(str(LIB_PATH))
    L.lbm_source_hash.argtypes = []
    L.lbm_source_hash.restype = ctypes.c_char_p
    built = L.lbm_source_hash().decode()
    from . import srchash
    if srchash.source_files() and built != srchash.source_hash():
        raise RuntimeError(f"{LIB_PATH} was built from other sources (hash {built}, sources "
                           f"{srchash.source_hash()}): rebuild it (make -C lbm-graphcore_amd)")
    H = ctypes.c_void_p
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    f32p = ctypes.POINTER(ctypes.c_float)
    u8p = ctypes.POINTER(ctypes.c_uint8)
    i32p = ctypes.POINTER(ctypes.c_int32)
    f64p, i64p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    f32pp, f64pp = ctypes.POINTER(f32p), ctypes.POINTER(f64p)
    sig = {
        # include/lbm_hip.h (lbm_source_hash is declared above)
        "lbm_abi_version": ([], i32),
        "lbm_partition": ([i32, i32, i32, i32, i32, i32p, i32p, ctypes.POINTER(Rect)], ctypes.c_int),
        "lbm_halo_plan": ([i32p], ctypes.c_int),
        "lbm_exchange_schedule": ([i32, i32, i32, i32, i32, i32, i32, i32, i32, ctypes.POINTER(Xfer), i32, i32p],
                                  ctypes.c_int),
        "lbm_device_count": ([], i32),
        "lbm_rccl_unique_id": ([u8p], ctypes.c_int),
        "lbm_create": ([ctypes.POINTER(Params), u8p, i32, ctypes.POINTER(H)], ctypes.c_int),
        "lbm_create_ex": ([ctypes.POINTER(Params), u8p, ctypes.POINTER(Config), ctypes.POINTER(H)], ctypes.c_int),
        "lbm_load_cells": ([H, f32p], ctypes.c_int),
        "lbm_init_equilibrium": ([H], ctypes.c_int),
        "lbm_run": ([H], ctypes.c_int),
        "lbm_run_steps": ([H, i32, i32], ctypes.c_int),
        "lbm_store": ([H, f32p, f32p, i32], ctypes.c_int),
        "lbm_load_cells_local": ([H, f32p], ctypes.c_int),
        "lbm_store_local": ([H, f32p, f32p, i32], ctypes.c_int),
        "lbm_local_cells": ([H], i64),
        "lbm_store_fields": ([H, f32p, f32p, f32p, f32p], ctypes.c_int),
        "lbm_store_fields_local": ([H, f32p, f32p, f32p, f32p], ctypes.c_int),
        "lbm_field_stats": ([H, f64p, f32p], ctypes.c_int),
        "lbm_last_run_seconds": ([H, f64p], ctypes.c_int),
        "lbm_total_free_cells": ([H], i64),
        "lbm_local_rects": ([H, ctypes.POINTER(Rect), i32, i32p], ctypes.c_int),
        "lbm_kernel_in_use": ([H], i32),
        "lbm_steps_per_launch": ([H], i32),
        "lbm_run_stats": ([H, i32p, i32p], ctypes.c_int),
        "lbm_stream_units": ([H, ctypes.POINTER(StreamUnit), i32, i32p], ctypes.c_int),
        "lbm_profile_summary": ([H, ctypes.POINTER(KernelTime), i32, i32p], ctypes.c_int),
        "lbm_profile_reset": ([H], ctypes.c_int),
        "lbm_placement_probe": ([H, i32p, i32p, f32p, i32], ctypes.c_int),
        "lbm_numerics": ([H], i32),
        "lbm_nonfinite_count": ([H, i64p], ctypes.c_int),
        "lbm_last_error": ([H], ctypes.c_char_p),
        "lbm_destroy": ([H], None),
        # include/lbm3d_hip.h
        "lbm3d_create": ([ctypes.POINTER(Params3D), u8p, ctypes.POINTER(Config), ctypes.POINTER(H)], ctypes.c_int),
        "lbm3d_init_equilibrium": ([H], ctypes.c_int),
        "lbm3d_load_cells": ([H, f32p], ctypes.c_int),
        "lbm3d_run_steps": ([H, i32], ctypes.c_int),
        "lbm3d_store": ([H, f32p, f32p, i32], ctypes.c_int),
        "lbm3d_last_run_seconds": ([H, f64p], ctypes.c_int),
        "lbm3d_total_free_cells": ([H], i64),
        "lbm3d_local_slabs": ([H, i32p, i32p, i32, i32p], ctypes.c_int),
        "lbm3d_exchange_schedule": ([i32, i32, i32, i32, i32, i32, ctypes.POINTER(Xfer), i32, i32p], ctypes.c_int),
        "lbm3d_run_stats": ([H, i32p, i32p, i32p, i32p], ctypes.c_int),
        "lbm3d_numerics": ([H], i32),
        "lbm3d_last_error": ([H], ctypes.c_char_p),
        "lbm3d_destroy": ([H], None),
        # include/lbm3d_fields_hip.h
        "lbm3d_store_fields": ([H, f32p, f32p, f32p, f32p, f32p], ctypes.c_int),
        "lbm3d_store_fields_box": ([H, ctypes.POINTER(Box3D), f32p, f32p, f32p, f32p, f32p], ctypes.c_int),
        "lbm3d_field_stats": ([H, f64p, f32p], ctypes.c_int),
        # include/lbm_forces_hip.h
        "lbm_wall_force": ([H, f64p, f64p, i64p], ctypes.c_int),
        "lbm_store_wall_force": ([H, f32p, f32p], ctypes.c_int),
        "lbm_set_bodies": ([H, i32p, i32], ctypes.c_int),
        "lbm_body_forces": ([H, f64p, f64p, i64p, i32], ctypes.c_int),
        "lbm3d_wall_force": ([H, f64p, f64p, f64p, i64p], ctypes.c_int),
        "lbm3d_store_wall_force": ([H, f32p, f32p, f32p], ctypes.c_int),
        "lbm3d_set_bodies": ([H, i32p, i32], ctypes.c_int),
        "lbm3d_body_forces": ([H, f64p, f64p, f64p, i64p, i32], ctypes.c_int),
        # include/lbm_averages_hip.h
        "lbm_avg_begin": ([H, i32], ctypes.c_int),
        "lbm_avg_sample": ([H], ctypes.c_int),
        "lbm_avg_samples": ([H, i64p], ctypes.c_int),
        "lbm_avg_store_sums": ([H, f64pp], ctypes.c_int),
        "lbm_avg_store": ([H, f32pp], ctypes.c_int),
        "lbm_avg_end": ([H], ctypes.c_int),
        "lbm3d_avg_begin": ([H, i32], ctypes.c_int),
        "lbm3d_avg_sample": ([H], ctypes.c_int),
        "lbm3d_avg_samples": ([H, i64p], ctypes.c_int),
        "lbm3d_avg_store_sums": ([H, f64pp], ctypes.c_int),
        "lbm3d_avg_store": ([H, f32pp], ctypes.c_int),
        "lbm3d_avg_end": ([H], ctypes.c_int),
        # include/lbm_gradients_hip.h
        "lbm_store_gradients": ([H, f32pp], ctypes.c_int),
        "lbm_store_gradients_local": ([H, f32pp], ctypes.c_int),
        "lbm_gradient_stats": ([H, f64p, f64p, f32p, f32p], ctypes.c_int),
        "lbm3d_store_gradients": ([H, f32pp], ctypes.c_int),
        "lbm3d_store_gradients_box": ([H, ctypes.POINTER(Box3D), f32pp], ctypes.c_int),
        "lbm3d_gradient_stats": ([H, f64p, f64p, f32p, f32p], ctypes.c_int),
        # include/lbm_stress_hip.h
        "lbm_store_stress": ([H, f32pp], ctypes.c_int),
        "lbm_store_stress_local": ([H, f32pp], ctypes.c_int),
        "lbm_stress_stats": ([H, f64p, f32p, i64p, f64p, f32p], ctypes.c_int),
        "lbm3d_store_stress": ([H, f32pp], ctypes.c_int),
        "lbm3d_store_stress_box": ([H, ctypes.POINTER(Box3D), f32pp], ctypes.c_int),
        "lbm3d_stress_stats": ([H, f64p, f32p, i64p, f64p, f32p], ctypes.c_int),
        # include/lbm_binned_hip.h
        "lbm_store_binned": ([H, i32, i32, f64pp], ctypes.c_int),
        "lbm_bin_fluid_cells": ([H, i32, i32, i64p], ctypes.c_int),
        "lbm3d_store_binned": ([H, i32, i32, i32, f64pp], ctypes.c_int),
        "lbm3d_bin_fluid_cells": ([H, i32, i32, i32, i64p], ctypes.c_int),
        # include/lbm_tracers_hip.h
        "lbm_tracer_begin": ([H, i64, f64p, f64p], ctypes.c_int),
        "lbm_tracer_count": ([H, i64p], ctypes.c_int),
        "lbm_tracer_advance": ([H, ctypes.c_double, i32], ctypes.c_int),
        "lbm_tracer_sample": ([H, f64p, f64p, f64p], ctypes.c_int),
        "lbm_tracer_store": ([H, f64p, f64p, u8p], ctypes.c_int),
        "lbm_tracer_end": ([H], ctypes.c_int),
        "lbm_tracer_advance_ref": ([i32, i32, f32p, f32p, i64, f64p, f64p, ctypes.c_double, i32], ctypes.c_int),
        "lbm_tracer_sample_ref": ([i32, i32, f32p, f32p, f32p, i64, f64p, f64p, f64p, f64p, f64p], ctypes.c_int),
        "lbm3d_tracer_begin": ([H, i64, f64p, f64p, f64p], ctypes.c_int),
        "lbm3d_tracer_count": ([H, i64p], ctypes.c_int),
        "lbm3d_tracer_advance": ([H, ctypes.c_double, i32], ctypes.c_int),
        "lbm3d_tracer_sample": ([H, f64p, f64p, f64p, f64p], ctypes.c_int),
        "lbm3d_tracer_store": ([H, f64p, f64p, f64p, u8p], ctypes.c_int),
        "lbm3d_tracer_end": ([H], ctypes.c_int),
        "lbm3d_tracer_advance_ref": ([i32, i32, i32, f32p, f32p, f32p, i64, f64p, f64p, f64p, ctypes.c_double, i32],
                                     ctypes.c_int),
        "lbm3d_tracer_sample_ref": ([i32, i32, i32, f32p, f32p, f32p, f32p, i64, f64p, f64p, f64p,
                                     f64p, f64p, f64p, f64p], ctypes.c_int),
        # include/lbm_scalar_hip.h
        "lbm_scalar_begin": ([H, ctypes.c_float, f32p], ctypes.c_int),
        "lbm_scalar_set_fixed": ([H, i64, i32p, i32p, f32p], ctypes.c_int),
        "lbm_scalar_advance": ([H, i32], ctypes.c_int),
        "lbm_scalar_steps": ([H, i64p], ctypes.c_int),
        "lbm_scalar_store": ([H, f32p, f32p], ctypes.c_int),
        "lbm_scalar_stats": ([H, f64p, f32p, f32p], ctypes.c_int),
        "lbm_scalar_end": ([H], ctypes.c_int),
        "lbm_scalar_step_ref": ([i32, i32, ctypes.c_float, f32p, f32p, u8p, f32p, f32p], ctypes.c_int),
        "lbm3d_scalar_begin": ([H, ctypes.c_float, f32p], ctypes.c_int),
        "lbm3d_scalar_set_fixed": ([H, i64, i32p, i32p, i32p, f32p], ctypes.c_int),
        "lbm3d_scalar_advance": ([H, i32], ctypes.c_int),
        "lbm3d_scalar_steps": ([H, i64p], ctypes.c_int),
        "lbm3d_scalar_store": ([H, f32p, f32p], ctypes.c_int),
        "lbm3d_scalar_stats": ([H, f64p, f32p, f32p], ctypes.c_int),
        "lbm3d_scalar_end": ([H], ctypes.c_int),
        "lbm3d_scalar_step_ref": ([i32, i32, i32, ctypes.c_float, f32p, f32p, f32p, u8p, f32p, f32p], ctypes.c_int),
        # include/lbm_thermal_hip.h
        "lbm_scalar_buoyancy": ([H] + [ctypes.c_float] * 3, ctypes.c_int),
        "lbm3d_scalar_buoyancy": ([H] + [ctypes.c_float] * 4, ctypes.c_int),
        "lbm_scalar_buoyancy_ref": ([i32, i32] + [ctypes.c_float] * 4 + [u8p, f32p, f32p], ctypes.c_int),
        "lbm3d_scalar_buoyancy_ref": ([i32, i32, i32] + [ctypes.c_float] * 5 + [u8p, f32p, f32p], ctypes.c_int),
        # include/lbm_transport_hip.h
        "lbm_scalar_store_binned": ([H, i32, i32, f64pp], ctypes.c_int),
        "lbm3d_scalar_store_binned": ([H, i32, i32, i32, f64pp], ctypes.c_int),
        "lbm_scalar_terms_ref": ([i32, i32, f32p, f32p, u8p, f32p, f64p], ctypes.c_int),
        "lbm3d_scalar_terms_ref": ([i32, i32, i32, f32p, f32p, f32p, u8p, f32p, f64p], ctypes.c_int),
        # include/lbm_scalar_walls_hip.h
        "lbm_scalar_set_walls": ([H, i32p, i32, i32p, f32p], ctypes.c_int),
        "lbm_scalar_wall_flux": ([H, f64p, i64p], ctypes.c_int),
        "lbm_scalar_body_flux": ([H, f64p, i64p, i32], ctypes.c_int),
        "lbm_scalar_store_wall_flux": ([H, f32p], ctypes.c_int),
        "lbm_scalar_walls_ref": ([i32, i32, u8p, i32p, i32, i32p, f32p, f32p, f32p], ctypes.c_int),
        "lbm3d_scalar_set_walls": ([H, i32p, i32, i32p, f32p], ctypes.c_int),
        "lbm3d_scalar_wall_flux": ([H, f64p, i64p], ctypes.c_int),
        "lbm3d_scalar_body_flux": ([H, f64p, i64p, i32], ctypes.c_int),
        "lbm3d_scalar_store_wall_flux": ([H, f32p], ctypes.c_int),
        "lbm3d_scalar_walls_ref": ([i32, i32, i32, u8p, i32p, i32, i32p, f32p, f32p, f32p], ctypes.c_int),
        # include/lbm_forcing_hip.h
        "lbm_forcing_set_zone": ([H] + [i32] * 5 + [f32pp, f32p], ctypes.c_int),
        "lbm_forcing_clear": ([H], ctypes.c_int),
        "lbm_forcing_zones": ([H, i32p, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "lbm_forcing_apply": ([H, ctypes.c_float, f64p], ctypes.c_int),
        "lbm_forcing_kick_ref": ([i32, i32, u8p, f32p] + [i32] * 4 + [f32pp, f32p, ctypes.c_float, f32p], ctypes.c_int),
        "lbm3d_forcing_set_zone": ([H] + [i32] * 7 + [f32pp, f32p], ctypes.c_int),
        "lbm3d_forcing_clear": ([H], ctypes.c_int),
        "lbm3d_forcing_zones": ([H, i32p, ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
        "lbm3d_forcing_apply": ([H, ctypes.c_float, f64p], ctypes.c_int),
        "lbm3d_forcing_kick_ref": ([i32, i32, i32, u8p, f32p] + [i32] * 6 + [f32pp, f32p, ctypes.c_float, f32p],
                                   ctypes.c_int),
        # include/lbm_sgs_hip.h
        "lbm_sgs_set": ([H, i32, ctypes.c_float, f32p], ctypes.c_int),
        "lbm_sgs_apply": ([H, ctypes.c_float, f64p], ctypes.c_int),
        "lbm_sgs_store_nut": ([H, f32p], ctypes.c_int),
        "lbm_sgs_filter_ref": ([i32, i32, u8p, f32p, ctypes.c_float, i32, ctypes.c_float, f32p, ctypes.c_float, f32p],
                               ctypes.c_int),
        "lbm3d_sgs_set": ([H, i32, ctypes.c_float, f32p], ctypes.c_int),
        "lbm3d_sgs_apply": ([H, ctypes.c_float, f64p], ctypes.c_int),
        "lbm3d_sgs_store_nut": ([H, f32p], ctypes.c_int),
        "lbm3d_sgs_filter_ref": ([i32, i32, i32, u8p, f32p, ctypes.c_float, i32, ctypes.c_float, f32p, ctypes.c_float,
                                  f32p], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        fn = getattr(L, name)
        fn.argtypes = args
        fn.restype = res
    if L.lbm_abi_version() != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH}: ABI version {L.lbm_abi_version()}, binding expects {ABI_VERSION}")
    _lib = L
    return L


def _ptr(a: np.ndarray):
    """The array's data as a pointer to its own element type (float32 -> float *, int64 -> int64_t *, ...)."""
    return a.ctypes.data_as(ctypes.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _select(names, which, what):
    """`which` (None: all of `names`) as a tuple, checked; `what` names the kind of field in the error."""
    which = tuple(names if which is None else which)
    if any(n not in names for n in which) or len(set(which)) != len(which):
        raise ValueError(f"{what} are a subset of {names}, each at most once; got {which}")
    return which


def _ptr_list(names, out):
    """One pointer per header name, None (NULL) where `out` has no such array: the positional form."""
    return [_ptr(out[n]) if n in out else None for n in names]


def _ptr_table(names, out, ctype):
    """The same as the `ctype *out[len(names)]` array the store entry points take."""
    return (ctypes.POINTER(ctype) * len(names))(*_ptr_list(names, out))


def _per_rect(rects, packed, *tail):
    """Views [h][w][*tail] per rect (local_rects() order) of a packed array, or of each of a dict of them."""
    out, off = [], 0
    for (_, _, w, h) in rects:
        n = w * h * int(np.prod(tail, dtype=np.int64))
        if isinstance(packed, dict):
            out.append({f: a[off:off + n].reshape(h, w, *tail) for f, a in packed.items()})
        else:
            out.append(packed[off:off + n].reshape(h, w, *tail))
        off += n
    return out


def _tracer_scheme(scheme) -> int:
    if isinstance(scheme, str):
        if scheme not in TRACER_SCHEMES:
            raise ValueError(f"scheme is one of {tuple(TRACER_SCHEMES)}; got {scheme!r}")
        return TRACER_SCHEMES[scheme]
    return int(scheme)


def _ref_fields(fields, dims):
    """Planar fp32 fields of one shape (None allowed) for the *_ref entry points: (arrays, extents x first)."""
    arrs = [None if f is None else np.ascontiguousarray(f, np.float32) for f in fields]
    shapes = {a.shape for a in arrs if a is not None}
    if len(shapes) != 1 or len(next(iter(shapes))) != dims:
        raise ValueError(f"fields must be {dims}-D arrays of one shape")
    return arrs, tuple(int(n) for n in next(iter(shapes))[::-1])


def _ref_points(pos):
    pts = [np.array(c, np.float64, ndmin=1) for c in pos]          # copies: advance_ref moves them in place
    if len({c.shape for c in pts}) != 1 or pts[0].ndim != 1:
        raise ValueError("positions must be 1-D arrays of one length")
    return pts


def tracer_advance_ref(ux, uy, x, y, dt, scheme="heun"):
    """(x', y'): lbm_tracer_advance_ref -- the C++ per-point functions of the kernels, compiled
    for the host, over planar float32[ny][nx] fields (no GPU).  lio.tracer_advance restates it."""
    L = load_library()
    (ux, uy), (nx, ny) = _ref_fields((ux, uy), 2)
    x, y = _ref_points((x, y))
    rc = L.lbm_tracer_advance_ref(nx, ny, _ptr(ux), _ptr(uy), x.size, _ptr(x), _ptr(y), float(dt),
                                  _tracer_scheme(scheme))
    if rc != LBM_OK:
        raise LbmError(rc, "lbm_tracer_advance_ref: invalid argument")
    return x, y


def tracer_advance3d_ref(ux, uy, uz, x, y, z, dt, scheme="heun"):
    """(x', y', z'): lbm3d_tracer_advance_ref over planar float32[nz][ny][nx] fields."""
    L = load_library()
    (ux, uy, uz), (nx, ny, nz) = _ref_fields((ux, uy, uz), 3)
    x, y, z = _ref_points((x, y, z))
    rc = L.lbm3d_tracer_advance_ref(nx, ny, nz, _ptr(ux), _ptr(uy), _ptr(uz), x.size, _ptr(x), _ptr(y), _ptr(z),
                                    float(dt), _tracer_scheme(scheme))
    if rc != LBM_OK:
        raise LbmError(rc, "lbm3d_tracer_advance_ref: invalid argument")
    return x, y, z


def _sample_ref(fn, names, fields, pos):
    dims = len(pos)
    arrs, extent = _ref_fields(fields, dims)
    pts = _ref_points(pos)
    nan = np.float64(np.nan)
    out = {n: np.full(pts[0].size, nan) for n, a in zip(names, arrs) if a is not None}
    rc = fn(*extent, *[None if a is None else _ptr(a) for a in arrs], pts[0].size, *[_ptr(c) for c in pts],
            *_ptr_list(names, out))
    if rc != LBM_OK:
        raise LbmError(rc, "tracer_sample_ref: invalid argument")
    return out


def tracer_sample_ref(ux, uy, pressure, x, y):
    """{name: float64[n]} of the fields given (None: skipped) interpolated at (x, y):
    lbm_tracer_sample_ref.  lio.tracer_interp restates it."""
    return _sample_ref(load_library().lbm_tracer_sample_ref, TRACER_FIELDS, (ux, uy, pressure), (x, y))


def tracer_sample3d_ref(ux, uy, uz, pressure, x, y, z):
    """The D3Q19 twin: lbm3d_tracer_sample_ref."""
    return _sample_ref(load_library().lbm3d_tracer_sample_ref, TRACER_FIELDS3D, (ux, uy, uz, pressure), (x, y, z))


def scalar_step_ref(g, ux, uy, obst, omega_s):
    """float32[5][ny][nx]: lbm_scalar_step_ref -- one step by the C++ per-cell function of the
    kernel, compiled for the host (no GPU).  lio.scalar_step restates it."""
    (ux, uy), (nx, ny) = _ref_fields((ux, uy), 2)
    g = np.ascontiguousarray(g, np.float32)
    obst = np.ascontiguousarray(obst, np.uint8)
    if g.shape != (SCALAR_Q, ny, nx) or obst.shape != (ny, nx):
        raise ValueError("g must be [5][ny][nx] and obst [ny][nx] of the fields' shape")
    out = np.zeros_like(g)
    rc = load_library().lbm_scalar_step_ref(nx, ny, float(omega_s), _ptr(ux), _ptr(uy), _ptr(obst), _ptr(g), _ptr(out))
    if rc != LBM_OK:
        raise LbmError(rc, "lbm_scalar_step_ref: invalid argument")
    return out


def scalar_step3d_ref(g, ux, uy, uz, obst, omega_s):
    """float32[7][nz][ny][nx]: lbm3d_scalar_step_ref.  lio.scalar_step3d restates it."""
    (ux, uy, uz), (nx, ny, nz) = _ref_fields((ux, uy, uz), 3)
    g = np.ascontiguousarray(g, np.float32)
    obst = np.ascontiguousarray(obst, np.uint8)
    if g.shape != (SCALAR_Q3D, nz, ny, nx) or obst.shape != (nz, ny, nx):
        raise ValueError("g must be [7][nz][ny][nx] and obst [nz][ny][nx] of the fields' shape")
    out = np.zeros_like(g)
    rc = load_library().lbm3d_scalar_step_ref(nx, ny, nz, float(omega_s), _ptr(ux), _ptr(uy), _ptr(uz), _ptr(obst),
                                              _ptr(g), _ptr(out))
    if rc != LBM_OK:
        raise LbmError(rc, "lbm3d_scalar_step_ref: invalid argument")
    return out


def _buoyancy_ref(name, q, qs, cells, g, obst, density, s, phi_ref):
    cells = np.array(cells, np.float32, order="C")
    shape = cells.shape[:-1]
    g = np.ascontiguousarray(g, np.float32)
    obst = np.ascontiguousarray(obst, np.uint8)
    if len(s) != len(shape) or cells.shape[-1] != q or g.shape != (qs,) + shape or obst.shape != shape:
        raise ValueError("cells [..][q], g [qs][..] and obst [..] of one domain, s one component per axis")
    rc = getattr(load_library(), name)(*shape[::-1], float(density), *[float(c) for c in s], float(phi_ref),
                                       _ptr(obst), _ptr(g), _ptr(cells))
    if rc != LBM_OK:
        raise LbmError(rc, name + ": invalid argument")
    return cells


def scalar_buoyancy_ref(cells, g, obst, density, s, phi_ref=0.0):
    """A kicked copy of the AoS cells float32[ny][nx][9]: lbm_scalar_buoyancy_ref -- the C++ per-cell
    function of the kernel, compiled for the host (no GPU).  lio.buoyancy_kick restates it."""
    return _buoyancy_ref("lbm_scalar_buoyancy_ref", 9, SCALAR_Q, cells, g, obst, density, s, phi_ref)


def scalar_buoyancy3d_ref(cells, g, obst, density, s, phi_ref=0.0):
    """lbm3d_scalar_buoyancy_ref: cells float32[nz][ny][nx][19].  lio.buoyancy_kick3d restates it."""
    return _buoyancy_ref("lbm3d_scalar_buoyancy_ref", Q3, SCALAR_Q3D, cells, g, obst, density, s, phi_ref)


def _forcing_coefs(dims, ext, lam, target, force):
    """(arrays kept alive, pointer table float *[1 + 2 dims], constants float[1 + 2 dims]) of a zone's
    coefficients in header order: each of lam, target[i], force[i] a number (a constant) or an array of the
    box's shape `ext` (slowest axis first)."""
    target = [0.0] * dims if target is None else list(target)
    force = [0.0] * dims if force is None else list(force)
    if len(target) != dims or len(force) != dims:
        raise ValueError(f"target and force have {dims} components")
    keep, ptrs, konst = [], [], []
    for c in [lam] + target + force:
        if np.ndim(c) == 0:
            ptrs.append(None)
            konst.append(float(c))
        else:
            a = np.ascontiguousarray(c, np.float32)
            if a.shape != tuple(ext):
                raise ValueError(f"a coefficient array has the box's shape {tuple(ext)}; got {a.shape}")
            keep.append(a)
            ptrs.append(_ptr(a))
            konst.append(0.0)
    n = 1 + 2 * dims
    return keep, (ctypes.POINTER(ctypes.c_float) * n)(*ptrs), (ctypes.c_float * n)(*konst)


def _forcing_ref(name, q, cells, obst, box, lam, target, force, n):
    cells = np.array(cells, np.float32, order="C")
    dims = cells.ndim - 1
    obst = np.ascontiguousarray(obst, np.uint8)
    box = [int(v) for v in box]
    if cells.shape[-1] != q or obst.shape != cells.shape[:-1] or len(box) != 2 * dims:
        raise ValueError("cells [..][q] and obst [..] of one domain, box = (x0, y0[, z0], w, h[, d])")
    ext = box[dims:][::-1]
    if min(ext) < 1:
        raise ValueError("the box is not empty")
    keep, table, konst = _forcing_coefs(dims, ext, lam, target, force)
    terms = np.zeros(tuple(ext) + (dims,), np.float32)
    rc = getattr(load_library(), name)(*cells.shape[:-1][::-1], _ptr(obst), _ptr(cells), *box, table, konst,
                                       float(n), _ptr(terms))
    if rc != LBM_OK:
        raise LbmError(rc, name + ": invalid argument")
    return cells, terms


def forcing_kick_ref(cells, obst, box, lam=0.0, target=None, force=None, n=1.0):
    """(kicked copy of the AoS cells float32[ny][nx][9], terms float32[h][w][2]): lbm_forcing_kick_ref -- the
    C++ per-cell function of the kernel, compiled for the host (no GPU) -- of one zone box = (x0, y0, w, h).
    lio.forcing_kick restates it."""
    return _forcing_ref("lbm_forcing_kick_ref", 9, cells, obst, box, lam, target, force, n)


def forcing_kick3d_ref(cells, obst, box, lam=0.0, target=None, force=None, n=1.0):
    """lbm3d_forcing_kick_ref: cells float32[nz][ny][nx][19], box = (x0, y0, z0, w, h, d).  lio.forcing_kick3d
    restates it."""
    return _forcing_ref("lbm3d_forcing_kick_ref", Q3, cells, obst, box, lam, target, force, n)


def _sgs_mode(mode, off=False) -> int:
    m = SGS_MODES.get(mode, mode) if isinstance(mode, str) else mode
    if m not in ((SGS_OFF, SGS_SMAGORINSKY, SGS_OMEGA) if off else (SGS_SMAGORINSKY, SGS_OMEGA)):
        raise ValueError(f"the sub-grid mode is one of {sorted(SGS_MODES)}; got {mode!r}")
    return int(m)


def _sgs_coef(coef, shape):
    """(array kept alive or None, its pointer or NULL, the constant) of a coefficient: a number, or an array
    of the domain's shape."""
    if np.ndim(coef) == 0:
        return None, None, float(coef)
    a = np.ascontiguousarray(coef, np.float32)
    if a.shape != tuple(shape):
        raise ValueError(f"a coefficient array has the domain's shape {tuple(shape)}; got {a.shape}")
    return a, _ptr(a), 0.0


def _sgs_ref(name, q, cells, obst, omega, mode, coef, n):
    cells = np.array(cells, np.float32, order="C")
    obst = np.ascontiguousarray(obst, np.uint8)
    if cells.shape[-1] != q or obst.shape != cells.shape[:-1]:
        raise ValueError("cells [..][q] and obst [..] of one domain")
    keep, ptr, konst = _sgs_coef(coef, obst.shape)
    nut = np.zeros(obst.shape, np.float32)
    rc = getattr(load_library(), name)(*obst.shape[::-1], _ptr(obst), _ptr(cells), float(omega), _sgs_mode(mode),
                                       konst, ptr, float(n), _ptr(nut))
    if rc != LBM_OK:
        raise LbmError(rc, name + ": invalid argument")
    return cells, nut


def sgs_filter_ref(cells, obst, omega, mode, coef, n=1.0):
    """(filtered copy of the AoS cells float32[ny][nx][9], nut float32[ny][nx]): lbm_sgs_filter_ref -- the C++
    per-cell function of the kernel, compiled for the host (no GPU).  lio.sgs_filter restates it."""
    return _sgs_ref("lbm_sgs_filter_ref", 9, cells, obst, omega, mode, coef, n)


def sgs_filter3d_ref(cells, obst, omega, mode, coef, n=1.0):
    """lbm3d_sgs_filter_ref: cells float32[nz][ny][nx][19].  lio.sgs_filter3d restates it."""
    return _sgs_ref("lbm3d_sgs_filter_ref", Q3, cells, obst, omega, mode, coef, n)


def _terms_ref(name, names, qs, g, u, obst):
    u, extent = _ref_fields(u, len(u))
    shape = extent[::-1]
    g = np.ascontiguousarray(g, np.float32)
    obst = np.ascontiguousarray(obst, np.uint8)
    if g.shape != (qs,) + shape or obst.shape != shape:
        raise ValueError(f"g must be [{qs}][..] and obst [..] of the fields' shape")
    terms = np.zeros((len(names),) + shape, np.float64)
    rc = getattr(load_library(), name)(*extent, *[_ptr(c) for c in u], _ptr(obst), _ptr(g), _ptr(terms))
    if rc != LBM_OK:
        raise LbmError(rc, name + ": invalid argument")
    return dict(zip(names, terms))


def scalar_terms_ref(g, ux, uy, obst):
    """{name: float64[ny][nx]} in SBIN_FIELDS order: lbm_scalar_terms_ref -- the per-cell terms of the
    transport sums by the C++ function of the kernel, compiled for the host (no GPU).
    lio.scalar_terms restates it."""
    return _terms_ref("lbm_scalar_terms_ref", SBIN_FIELDS, SCALAR_Q, g, (ux, uy), obst)


def scalar_terms3d_ref(g, ux, uy, uz, obst):
    """lbm3d_scalar_terms_ref: {name: float64[nz][ny][nx]} in SBIN_FIELDS3D order.  lio.scalar_terms3d
    restates it."""
    return _terms_ref("lbm3d_scalar_terms_ref", SBIN_FIELDS3D, SCALAR_Q3D, g, (ux, uy, uz), obst)


def _wall_table(kinds, values):
    """(kind int32[n], value float32[n]); a kind may be a name of SCALAR_WALL_KINDS."""
    kinds = [SCALAR_WALL_KINDS[k] if isinstance(k, str) else int(k) for k in np.asarray(kinds, object).reshape(-1)]
    kind = np.ascontiguousarray(kinds, np.int32)
    value = np.ascontiguousarray(values, np.float32).reshape(-1)
    if kind.size != value.size:
        raise ValueError("one kind and one value per body")
    return kind, value


def _walls_ref(name, qs, g, obst, labels, kinds, values, flux):
    g = np.array(g, np.float32, order="C")
    shape = g.shape[1:]
    obst = np.ascontiguousarray(obst, np.uint8)
    labels = np.ascontiguousarray(labels, np.int32)
    kind, value = _wall_table(kinds, values)
    if g.shape[0] != qs or len(shape) != (2 if qs == SCALAR_Q else 3) or obst.shape != shape or labels.shape != shape:
        raise ValueError(f"g must be [{qs}][..], obst and labels [..] of one domain")
    q = np.zeros(shape, np.float32) if flux else None
    rc = getattr(load_library(), name)(*shape[::-1], _ptr(obst), _ptr(labels), kind.size, _ptr(kind), _ptr(value),
                                       _ptr(g), None if q is None else _ptr(q))
    if rc != LBM_OK:
        raise LbmError(rc, name + ": invalid argument")
    return (g, q) if flux else g


def scalar_walls_ref(g, obst, labels, kinds, values, flux=False):
    """A copy of g float32[5][ny][nx] after the wall pass, and with `flux` also the per-cell wall flux of
    the result: lbm_scalar_walls_ref -- the C++ per-cell functions of the kernels, compiled for the host
    (no GPU).  lio.scalar_apply_walls and lio.scalar_wall_flux_cells restate it."""
    return _walls_ref("lbm_scalar_walls_ref", SCALAR_Q, g, obst, labels, kinds, values, flux)


def scalar_walls3d_ref(g, obst, labels, kinds, values, flux=False):
    """lbm3d_scalar_walls_ref: g float32[7][nz][ny][nx].  lio.scalar_apply_walls3d restates it."""
    return _walls_ref("lbm3d_scalar_walls_ref", SCALAR_Q3D, g, obst, labels, kinds, values, flux)


def partition(nx: int, ny: int, parts: int, grid_rows: int = 0, grid_cols: int = 0):
    """Reference partition rule via the C ABI. Returns (rows, cols, [(x0,y0,w,h)...])."""
    L = load_library()
    rects = (Rect * parts)()
    r, c = ctypes.c_int32(), ctypes.c_int32()
    rc = L.lbm_partition(nx, ny, parts, grid_rows, grid_cols, ctypes.byref(r), ctypes.byref(c), rects)
    if rc != LBM_OK:
        raise LbmError(rc, f"cannot partition {nx}x{ny} into {parts}")
    return r.value, c.value, [(q.x0, q.y0, q.w, q.h) for q in rects]


def halo_plan():
    """[(dx, dy, [planes...]) for the 8 directions E, N, W, S, NE, NW, SW, SE]."""
    t = (ctypes.c_int32 * 48)()
    rc = load_library().lbm_halo_plan(t)
    if rc != LBM_OK:
        raise LbmError(rc, "lbm_halo_plan failed")
    out = []
    for d in range(8):
        dx, dy, n = t[6 * d], t[6 * d + 1], t[6 * d + 2]
        out.append((dx, dy, [t[6 * d + 3 + i] for i in range(n)]))
    return out


def exchange_schedule(nx: int, ny: int, parts: int, rank: int, mode: int = HALO_WG, halo_width: int = 1,
                      grid_rows: int = 0, grid_cols: int = 0, force_exchange: bool = False):
    """The engine's own ordered halo-exchange posts for `rank` (lbm_exchange_schedule):
    [(op, dir, peer, floats), ...] with op XFER_SEND / XFER_RECV / XFER_SELF."""
    L = load_library()
    buf = (Xfer * 32)()
    n = ctypes.c_int32()
    rc = L.lbm_exchange_schedule(nx, ny, parts, grid_rows, grid_cols, rank, mode, halo_width, int(force_exchange),
                                 buf, 32, ctypes.byref(n))
    if rc != LBM_OK:
        raise LbmError(rc, f"lbm_exchange_schedule({nx}, {ny}, {parts}, rank {rank}) failed")
    return [(x.op, x.dir, x.peer, x.floats) for x in buf[:n.value]]


def exchange_schedule3d(nx: int, ny: int, nz: int, parts: int, rank: int, planes: int):
    """The D3Q19 engine's ordered z-slab exchange posts (lbm3d_exchange_schedule);
    dir 0 = +z (up), 1 = -z (down)."""
    L = load_library()
    buf = (Xfer * 4)()
    n = ctypes.c_int32()
    rc = L.lbm3d_exchange_schedule(nx, ny, nz, parts, rank, planes, buf, 4, ctypes.byref(n))
    if rc != LBM_OK:
        raise LbmError(rc, f"lbm3d_exchange_schedule({nx}, {ny}, {nz}, {parts}, rank {rank}) failed")
    return [(x.op, x.dir, x.peer, x.floats) for x in buf[:n.value]]


def device_count() -> int:
    return int(load_library().lbm_device_count())


def rccl_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * 128)()
    rc = load_library().lbm_rccl_unique_id(buf)
    if rc != LBM_OK:
        raise LbmError(rc, "ncclGetUniqueId failed")
    return bytes(buf)


class _Handle:
    """What Engine and Engine3D share: the handle's life, the lookup of the engine's C functions,
    the error check and the chunked-run driver.  The class sets _PREFIX ("lbm_" / "lbm3d_") and
    _shape() (the domain's extents, slowest axis first); the diagnostics' mixins below use both."""

    def _fn(self, name):
        return getattr(self._L, self._PREFIX + name)

    def _check(self, rc: int):
        if rc != LBM_OK:
            raise LbmError(rc, self._fn("last_error")(self._h).decode())

    def _config(self, devices, unique_id) -> Config:
        """A Config with the device list and the RCCL id set; both buffers live as long as the handle."""
        cfg = Config()
        if devices:
            self._devs = (ctypes.c_int32 * len(devices))(*devices)
            cfg.devices = self._devs
            cfg.num_devices = len(devices)
        if unique_id is not None:
            self._uid = (ctypes.c_uint8 * 128).from_buffer_copy(unique_id)
            cfg.rccl_unique_id = self._uid
        return cfg

    def _create(self, name, obst, cfg) -> None:
        self._h = ctypes.c_void_p()
        rc = self._fn(name)(ctypes.byref(self.params), _ptr(obst), ctypes.byref(cfg), ctypes.byref(self._h))
        if rc != LBM_OK:
            raise LbmError(rc, self._fn("last_error")(None).decode())

    def _store_fields(self, name, names, which, shape, dtype, *args, table=True):
        """{n: zeros(shape) for n in which}, filled by the engine's `name`(handle, *args, outputs): the
        outputs as one pointer table, or (table=False) as one positional pointer per header name."""
        out = {n: np.zeros(shape, dtype) for n in which}
        ptrs = [_ptr_table(names, out, np.ctypeslib.as_ctypes_type(dtype))] if table else _ptr_list(names, out)
        self._check(self._fn(name)(self._h, *args, *ptrs))
        return out

    def _chunks(self, steps, every, accelerate_first, collect_av, after, before=None):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last; accelerate_first on the
        first chunk, D2Q9 only) and call after(n, done) behind each (and before(n) ahead of each).  Returns
        the float32 concatenation of the chunks' average velocities where collect_av asks for them (D2Q9
        only), else an empty one."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        two_d = len(self._shape()) == 2
        if accelerate_first and not two_d:
            raise ValueError("accelerate_first applies to the D2Q9 engine only")
        av, done = [], 0
        while done < steps:
            n = min(every, steps - done)
            if before is not None:
                before(n)
            if two_d:
                self.run_steps(n, accelerate_first and done == 0)
                if collect_av:
                    av.append(self.store(cells=False, n_av=n)[1].copy())
            else:
                self.run_steps(n)
            done += n
            after(n, done)
        return np.concatenate(av) if av else np.zeros(0, np.float32)

    def _stat_history(self, steps, every, accelerate_first, stats):
        """([(step,) + stats() after each chunk], av_vels) of _chunks."""
        samples = []
        av = self._chunks(steps, every, accelerate_first, True, lambda n, done: samples.append((done,) + stats()))
        return samples, av

    def close(self) -> None:
        if self._h:
            self._fn("destroy")(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _WallForces:
    """Engine / Engine3D methods over include/lbm_forces_hip.h."""

    _nbodies = 0

    def wall_force(self):
        """(fx, fy[, fz], links): the momentum-exchange force the fluid put on all wall
        cells of this handle's sub-domains in the last step (fp64 sums of the fp32
        per-cell values, folded in a fixed order) and the number of links."""
        f = [ctypes.c_double() for _ in self._shape()]
        links = ctypes.c_int64()
        self._check(self._fn("wall_force")(self._h, *[ctypes.byref(v) for v in f], ctypes.byref(links)))
        return tuple(v.value for v in f) + (links.value,)

    def wall_force_field(self):
        """(fx, fy[, fz]): planar float32 maps of the per-cell force, +0 on every cell that
        is no wall cell -- lio.wall_force_cells of store()'s cells, bit for bit.  RCCL:
        only this rank's part is written."""
        out = [np.zeros(self._shape(), np.float32) for _ in self._shape()]
        self._check(self._fn("store_wall_force")(self._h, *[_ptr(a) for a in out]))
        return tuple(out)

    def set_bodies(self, labels, nbodies: int) -> None:
        """Assign blocked cells to bodies 0..nbodies-1 (labels: int32 map of the full
        domain, e.g. lio.label_bodies; negative = no body).  set_bodies(None, 0) clears."""
        if labels is None:
            self._check(self._fn("set_bodies")(self._h, None, int(nbodies)))
        else:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.size != int(np.prod(self._shape())):
                raise ValueError("labels must cover the full domain")
            self._check(self._fn("set_bodies")(self._h, _ptr(lab), int(nbodies)))
        self._nbodies = int(nbodies) if labels is not None else 0

    def body_forces(self):
        """(fx[nbodies], fy[nbodies][, fz[nbodies]], links[nbodies]) of the bodies set last,
        summed on the device."""
        n = self._nbodies
        f = [np.zeros(max(n, 1), np.float64) for _ in self._shape()]
        links = np.zeros(max(n, 1), np.int64)
        self._check(self._fn("body_forces")(self._h, *[_ptr(a) for a in f], _ptr(links), n))
        return tuple(a[:n] for a in f) + (links[:n],)


class _Averages:
    """Engine / Engine3D methods over include/lbm_averages_hip.h; the class sets _AVG_FIELDS."""

    def _avg_store(self, name, which, dtype):
        """`which` defaults to every field begun: the first moments only after avg_begin(second=False)."""
        names = self._AVG_FIELDS
        if which is None and not getattr(self, "_avg_second", True):
            which = names[:len(self._shape()) + 1]
        which = _select(names, which, "averaged fields")
        return self._store_fields(name, names, which, self._shape(), dtype)

    def avg_begin(self, second: bool = True) -> None:
        """Start (or restart, re-zeroed) averaging: one fp64 sum per cell beside the lattice
        for the first moments (ux, uy[, uz], pressure) and, with `second`, for the velocity
        products and pressure squared.  8 B x fields x cells of device memory."""
        self._check(self._fn("avg_begin")(self._h, AVG_MEAN | AVG_SECOND if second else AVG_MEAN))
        self._avg_second = bool(second)

    def avg_sample(self) -> None:
        """Add the current lattice to the sums (one kernel; nothing goes to the host)."""
        self._check(self._fn("avg_sample")(self._h))

    @property
    def avg_samples(self) -> int:
        n = ctypes.c_int64()
        self._check(self._fn("avg_samples")(self._h, ctypes.byref(n)))
        return n.value

    def avg_end(self) -> None:
        """Free the accumulators (close() frees them too)."""
        self._check(self._fn("avg_end")(self._h))

    def avg_sums(self, which=None):
        """{name: float64 array} of the raw sums (lbm_avg_store_sums): lio.moment_sums of the
        sampled fields(), bit for bit.  Default: every field begun.  RCCL: only this rank's
        part is written."""
        return self._avg_store("avg_store_sums", which, np.float64)

    def mean_fields(self, which=None):
        """{name: float32 array}: the time means of "ux", "uy"[, "uz"], "pressure" and, under
        the second-moment names ("uxux", "uxuy", ..., "pp"), the central moments
        <a b> - <a><b> (Reynolds stresses, pressure variance), formed on the device
        (lbm_avg_store): lio.moment_means of avg_sums(), bit for bit."""
        return self._avg_store("avg_store", which, np.float32)


class _Gradients:
    """Engine / Engine3D methods over include/lbm_gradients_hip.h; the class sets _GRAD_FIELDS."""

    def gradients(self, which=None):
        """{name: float32 array} of the requested fields ("vorticity", "divergence",
        "strain", "q"; D3Q19 also "wx", "wy", "wz"), derived on the device from the
        current lattice (lbm_store_gradients): lio.velocity_gradients[3d] of fields(), bit
        for bit.  Default: every field."""
        names = self._GRAD_FIELDS
        return self._store_fields("store_gradients", names, _select(names, which, "gradient fields"), self._shape(),
                                  np.float32)

    def gradient_stats(self):
        """(sum_w2, sum_s2, max_w, max_div) over this handle's fluid cells
        (lbm_gradient_stats): the fp64 sums of vorticity^2 and S:S and the largest
        |vorticity| and |divergence|.  Enstrophy = sum_w2 / 2; dissipation = 2 nu sum_s2."""
        w2, s2 = ctypes.c_double(), ctypes.c_double()
        mw, md = ctypes.c_float(), ctypes.c_float()
        self._check(self._fn("gradient_stats")(
            self._h, ctypes.byref(w2), ctypes.byref(s2), ctypes.byref(mw), ctypes.byref(md)))
        return w2.value, s2.value, mw.value, md.value


class _Stress:
    """Engine / Engine3D methods over include/lbm_stress_hip.h; the class sets _STRESS_FIELDS."""

    def strain_rate(self, which=None):
        """{name: float32 array} of the requested strain-rate components and "strain"
        (D2Q9: "sxx", "sxy", "syy"; D3Q19 also "szz", "sxz", "syz"), from the
        non-equilibrium moments of the current lattice on the device (lbm_store_stress):
        lio.neq_strain[3d] of store()'s cells, bit for bit.  Default: every field."""
        names = self._STRESS_FIELDS
        return self._store_fields("store_stress", names, _select(names, which, "strain-rate fields"), self._shape(),
                                  np.float32)

    def strain_stats(self):
        """(sum_s2, max_strain, wall_cells, sum_wall_strain, max_wall_strain) over this
        handle's fluid cells (lbm_stress_stats); the last three over the fluid cells with a
        blocked lattice neighbour.  Dissipation = 2 nu sum_s2; in simple shear the wall
        shear stress is rho nu sqrt(2) strain."""
        s2, sw = ctypes.c_double(), ctypes.c_double()
        ms, mw = ctypes.c_float(), ctypes.c_float()
        nw = ctypes.c_int64()
        self._check(self._fn("stress_stats")(
            self._h, ctypes.byref(s2), ctypes.byref(ms), ctypes.byref(nw), ctypes.byref(sw), ctypes.byref(mw)))
        return s2.value, ms.value, nw.value, sw.value, mw.value


class _Binned:
    """Engine / Engine3D methods over include/lbm_binned_hip.h; the class sets _BIN_FIELDS."""

    def _bin_shape(self, bins):
        shape = self._shape()                            # slowest axis first
        if len(bins) != len(shape):
            raise ValueError(f"{len(shape)} bin sizes (x, y[, z]) expected; got {bins}")
        return tuple(-(-n // max(int(b), 1)) for n, b in zip(shape, bins[::-1]))

    def bin_fluid_cells(self, *bins):
        """int64 array of the fluid cells per bin over this handle's sub-domains
        (lbm_bin_fluid_cells).  The obstacle map never changes, so the result is kept
        per bin shape."""
        bins = tuple(int(b) for b in bins)
        cache = self.__dict__.setdefault("_bin_fluid", {})
        if bins not in cache:
            count = np.zeros(self._bin_shape(bins), np.int64)
            self._check(self._fn("bin_fluid_cells")(self._h, *bins, _ptr(count)))
            cache[bins] = count
        return cache[bins].copy()

    def binned(self, *bins, which=None):
        """{name: float64 array} of the sums of the requested per-cell quantities over
        bins of bw x bh[ x bd] cells (binned(bw, bh[, bd])), formed on the device from
        the current lattice (lbm_store_binned), and "fluid": the fluid cells per bin.
        Arrays are [[nbz]][nby][nbx].  lio.binned_sums[3d] of store()'s cells restates
        them; lio.binned_means divides.  Default: every field.  RCCL: this rank's partial
        sums and counts over the full bin grid."""
        bins = tuple(int(b) for b in bins)
        names = self._BIN_FIELDS
        out = self._store_fields("store_binned", names, _select(names, which, "binned fields"), self._bin_shape(bins),
                                 np.float64, *bins)
        out["fluid"] = self.bin_fluid_cells(*bins)
        return out

    def _bin_means(self, bins, which):
        s = self.binned(*bins, which=which)
        fluid = s.pop("fluid")
        return {n: np.divide(a, fluid, out=np.zeros_like(a), where=fluid != 0) for n, a in s.items()}

    def profile_y(self, which=None):
        """{name: float64[ny]}: the means over x (D3Q19: over x and z) of the requested
        quantities per row y -- the profile across the channel.  Bins (nx, 1[, nz])."""
        shape = self._shape()
        bins = (shape[-1], 1) + ((shape[0],) if len(shape) == 3 else ())
        return {n: a.reshape(-1) for n, a in self._bin_means(bins, which).items()}

    def flux_x(self):
        """float64[nx]: the sum of rho u_x over every cross-section x = const (the "jx"
        sums of bins (1, ny[, nz])): the mass flux through it."""
        shape = self._shape()
        return self.binned(*((1,) + shape[::-1][1:]), which=("jx",))["jx"].reshape(-1)

    def coarse_fields(self, k: int):
        """{name: float64 array} of the k x k[ x k] block means of "ux", "uy"[, "uz"] and
        "speed" over the fluid cells of each block (0 where a block holds none)."""
        dims = len(self._shape())
        which = ("ux", "uy", "uz", "speed") if dims == 3 else ("ux", "uy", "speed")
        bins = tuple(min(int(k), n) for n in self._shape()[::-1])
        return self._bin_means(bins, which)

    def binned_history(self, steps: int, every: int, *bins, which=None):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and take
        binned(*bins, which) after each chunk.  Returns {name: float64[samples, ...]} of
        the stacked samples, "step": the steps done at each sample, and "fluid".  The
        operator is linear: sums of the samples over time are the binned time sums.
        No average velocities are collected."""
        which = _select(self._BIN_FIELDS, which, "binned fields")
        samples, at = [], []

        def after(n, done):
            samples.append(self.binned(*bins, which=which))
            at.append(done)
        self._chunks(steps, every, False, False, after)
        shape = self._bin_shape(tuple(int(b) for b in bins))
        out = {n: (np.stack([s[n] for s in samples]) if samples else np.zeros((0,) + shape)) for n in which}
        out["step"] = np.asarray(at, np.int64)
        out["fluid"] = self.bin_fluid_cells(*bins)
        return out


class _Tracers:
    """Engine / Engine3D methods over include/lbm_tracers_hip.h; the class sets _TRACER_FIELDS."""

    def tracers_begin(self, x, y, z=None) -> None:
        """Copy the seed points (cell units, 0 <= x < nx, ...; float64) to the device; a second
        call replaces the set.  16 B (24 B) of device memory per point."""
        dims = len(self._shape())
        pos = (x, y) if dims == 2 else (x, y, z)
        if (z is None) != (dims == 2):
            raise ValueError(f"{dims} coordinate arrays expected")
        pts = [np.ascontiguousarray(c, np.float64).reshape(-1) for c in pos]
        if len({c.size for c in pts}) != 1:
            raise ValueError("coordinate arrays must have one length")
        self._check(self._fn("tracer_begin")(self._h, pts[0].size, *[_ptr(c) for c in pts]))

    @property
    def tracer_count(self) -> int:
        n = ctypes.c_int64()
        self._check(self._fn("tracer_count")(self._h, ctypes.byref(n)))
        return n.value

    def tracers_advance(self, dt, scheme="heun") -> None:
        """Move every point by dt lattice steps of the current lattice's velocity (one gather
        kernel; nothing goes to the host): lio.tracer_advance[3d] of fields(), bit for bit."""
        self._check(self._fn("tracer_advance")(self._h, float(dt), _tracer_scheme(scheme)))

    def tracers(self):
        """{"x", "y"[, "z"]: float64[n], "blocked": uint8[n]}: the current positions and whether
        the nearest cell of each is an obstacle."""
        n = self.tracer_count
        names = ("x", "y", "z")[:len(self._shape())]
        out = {c: np.full(n, np.nan) for c in names}
        out["blocked"] = np.zeros(n, np.uint8)
        self._check(self._fn("tracer_store")(self._h, *[_ptr(out[c]) for c in names], _ptr(out["blocked"])))
        return out

    def tracer_sample(self, which=None):
        """{name: float64[n]} of "ux", "uy"[, "uz"], "pressure" interpolated at the current
        positions: lio.tracer_interp[3d] of fields(), bit for bit.  Default: every field."""
        which = _select(self._TRACER_FIELDS, which, "sampled fields")
        n = self.tracer_count
        out = {f: np.full(n, np.nan) for f in which}
        self._check(self._fn("tracer_sample")(self._h, *_ptr_list(self._TRACER_FIELDS, out)))
        return out

    def tracers_end(self) -> None:
        """Free the set (close() frees it too)."""
        self._check(self._fn("tracer_end")(self._h))

    def run_traced(self, steps: int, every: int, scheme="heun", accelerate_first: bool = False):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and move the
        tracers after each chunk by dt = the steps of that chunk (tracers_begin first), so a
        shorter last chunk gets its own dt.  Returns the float32[steps] concatenation of the
        chunks' average velocities (D3Q19: empty).  Chunking behaves as in run_averaged."""
        scheme = _tracer_scheme(scheme)
        return self._chunks(steps, every, accelerate_first, True, lambda n, done: self.tracers_advance(n, scheme))

    def probe_history(self, steps: int, every: int, which=None, accelerate_first: bool = False):
        """The same chunks without moving the points: tracer_sample(which) after each chunk.
        Returns {name: float64[samples, n]} and "step": the steps done at each sample."""
        which = _select(self._TRACER_FIELDS, which, "sampled fields")
        samples, at = [], []

        def after(n, done):
            samples.append(self.tracer_sample(which))
            at.append(done)
        self._chunks(steps, every, accelerate_first, True, after)
        n = self.tracer_count
        out = {f: (np.stack([s[f] for s in samples]) if samples else np.zeros((0, n))) for f in which}
        out["step"] = np.asarray(at, np.int64)
        return out


class _Scalar:
    """Engine / Engine3D methods over include/lbm_scalar_hip.h, lbm_thermal_hip.h and lbm_transport_hip.h;
    the class sets _SCALAR_Q and _SBIN_FIELDS."""

    def scalar_begin(self, phi0=None, omega_s=None, diffusivity=None) -> None:
        """Start (or restart) a passive scalar at phi0 (float32 array of the domain's shape; None:
        zeros) with the relaxation rate omega_s in (0, 2) or the diffusivity D -- exactly one of the
        two; D = (1 / omega_s - 1/2) / 3 in 2-D, / 4 in 3-D.  40 B (56 B) of device memory per cell."""
        if (omega_s is None) == (diffusivity is None):
            raise ValueError("give exactly one of omega_s and diffusivity")
        dims = len(self._shape())
        if omega_s is None:
            if not float(diffusivity) > 0:
                raise ValueError("diffusivity must be positive")
            omega_s = 1.0 / ((3.0 if dims == 2 else 4.0) * float(diffusivity) + 0.5)
        if phi0 is not None:
            phi0 = np.ascontiguousarray(phi0, np.float32)
            if phi0.shape != self._shape():
                raise ValueError(f"phi0 must have the shape {self._shape()}")
        self._check(self._fn("scalar_begin")(self._h, float(omega_s), None if phi0 is None else _ptr(phi0)))
        self._scalar_omega = float(np.float32(omega_s))           # the rate the device holds, for nusselt()
        self._scalar_nbodies = 0                                  # begin drops the walls

    def scalar_fix(self, x, y, *rest) -> None:
        """scalar_fix(x, y[, z], value): replace the fixed list by these distinct cells, which hold the
        begin state of `value` from now on (set now and again after every scalar step); empty arrays
        clear the list."""
        dims = len(self._shape())
        if len(rest) != dims - 1:
            raise ValueError(f"scalar_fix takes {dims} coordinate arrays and the values")
        coords = [np.ascontiguousarray(c, np.int32).reshape(-1) for c in (x, y) + rest[:-1]]
        value = np.ascontiguousarray(rest[-1], np.float32).reshape(-1)
        if len({c.size for c in coords} | {value.size}) != 1:
            raise ValueError("coordinate and value arrays must have one length")
        self._check(self._fn("scalar_set_fixed")(self._h, value.size, *[_ptr(c) for c in coords], _ptr(value)))

    def scalar_advance(self, n: int = 1) -> None:
        """n scalar steps over the current, frozen lattice (nothing goes to the host): n times
        lio.scalar_step[3d] of fields(), then the fixed list, bit for bit."""
        self._check(self._fn("scalar_advance")(self._h, int(n)))

    def scalar(self, populations: bool = False):
        """phi (float32 array of the domain's shape), or (phi, g) with the planar populations
        float32[5][ny][nx] / [7][nz][ny][nx]."""
        phi = np.zeros(self._shape(), np.float32)
        if not populations:
            self._check(self._fn("scalar_store")(self._h, _ptr(phi), None))
            return phi
        g = np.zeros((self._SCALAR_Q,) + self._shape(), np.float32)
        self._check(self._fn("scalar_store")(self._h, _ptr(phi), _ptr(g)))
        return phi, g

    def scalar_stats(self):
        """(total, min, max): the fp64 sum of every cell's fp32 phi, folded in a fixed order, and the
        extremes over the fluid cells (lbm_scalar_stats)."""
        total, lo, hi = ctypes.c_double(), ctypes.c_float(), ctypes.c_float()
        self._check(self._fn("scalar_stats")(self._h, ctypes.byref(total), ctypes.byref(lo), ctypes.byref(hi)))
        return total.value, lo.value, hi.value

    @property
    def scalar_steps(self) -> int:
        n = ctypes.c_int64()
        self._check(self._fn("scalar_steps")(self._h, ctypes.byref(n)))
        return n.value

    def scalar_end(self) -> None:
        """Free the scalar lattice (close() frees it too)."""
        self._check(self._fn("scalar_end")(self._h))
        self._scalar_nbodies = 0

    def run_scalar(self, steps: int, stride: int = 1, accelerate_first: bool = False):
        """Advance flow and scalar together: repeat "run_steps(stride), then scalar_advance(stride)"
        (the remainder last; scalar_begin first).  stride = 1 is the exact coupling: every scalar
        step sees the velocity of its own flow step.  A stride equal to the fused depth
        (steps_per_launch()) keeps the flow on its fused launches, at the price of a velocity that
        is frozen for that many scalar steps.  Returns the float32[steps] concatenation of the
        chunks' average velocities (D3Q19: empty).  The flow is what run_steps in the same chunks
        gives; chunking behaves as in run_averaged."""
        return self._chunks(steps, stride, accelerate_first, True, lambda n, done: self.scalar_advance(n))

    def scalar_history(self, steps: int, every: int, stride: int = 1, accelerate_first: bool = False):
        """run_scalar(every, stride) chunk after chunk (the remainder last), scalar_stats() after
        each: a list of (step, total, min, max).  accelerate_first applies to the first chunk (D2Q9)."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        out, done = [], 0
        while done < steps:
            n = min(every, steps - done)
            self.run_scalar(n, stride, accelerate_first and done == 0)
            done += n
            out.append((done,) + self.scalar_stats())
        return out

    # Boussinesq buoyancy (include/lbm_thermal_hip.h)

    def scalar_buoyancy(self, s, phi_ref: float = 0.0) -> None:
        """Add the momentum density * s * (phi - phi_ref) to every fluid cell of the current lattice
        (s = (sx, sy[, sz]): acceleration per unit of scalar times the flow steps it stands for):
        lio.buoyancy_kick[3d] of store() and scalar(populations=True), bit for bit.  A run afterwards
        continues as from load_cells of the kicked cells.  s = 0 launches nothing."""
        s = [float(c) for c in s]
        if len(s) != len(self._shape()):
            raise ValueError(f"s has {len(self._shape())} components")
        self._check(self._fn("scalar_buoyancy")(self._h, *s, float(phi_ref)))

    def run_thermal(self, steps: int, accel, phi_ref: float = 0.0, stride: int = 1, accelerate_first: bool = False):
        """Advance flow and scalar with the scalar driving the flow: per chunk of n <= stride steps
        "scalar_buoyancy(n * accel, phi_ref), then run_steps(n), then scalar_advance(n)" (the remainder
        last; scalar_begin first).  accel = (gx, gy[, gz]) is the acceleration per unit of scalar and
        step.  stride = 1 is the exact first-order coupling; a larger stride applies the impulse of n
        steps at once and freezes the velocity for n scalar steps, as run_scalar does.  Returns what
        run_scalar returns."""
        accel = [float(c) for c in accel]
        return self._chunks(steps, stride, accelerate_first, True, lambda n, done: self.scalar_advance(n),
                            before=lambda n: self.scalar_buoyancy([n * c for c in accel], phi_ref))

    def thermal_history(self, steps: int, every: int, accel, phi_ref: float = 0.0, stride: int = 1,
                        accelerate_first: bool = False):
        """run_thermal(every, accel, phi_ref, stride) chunk after chunk (the remainder last),
        scalar_stats() after each: a list of (step, total, min, max)."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        out, done = [], 0
        while done < steps:
            n = min(every, steps - done)
            self.run_thermal(n, accel, phi_ref, stride, accelerate_first and done == 0)
            done += n
            out.append((done,) + self.scalar_stats())
        return out


    # binned transport sums (include/lbm_transport_hip.h)

    def scalar_binned(self, *bins, which=None):
        """{name: float64 array} of the sums over bins of bw x bh[ x bd] cells of the scalar's per-cell
        transport terms -- "phi", "phiphi", "uxphi", "uyphi"[, "uzphi"] over the fluid cells and the face
        fluxes "fx", "fy"[, "fz"] over all cells -- formed on the device from the current lattice and
        scalar (lbm_scalar_store_binned), and "fluid": the fluid cells per bin.  Arrays are
        [[nbz]][nby][nbx].  lio.scalar_binned_sums[3d] of fields() and scalar(populations=True) restates
        them.  Default: every field.  Without a "u?phi" field the flow lattice is not read; with faces
        only, just the planes those faces need."""
        bins = tuple(int(b) for b in bins)
        names = self._SBIN_FIELDS
        out = self._store_fields("scalar_store_binned", names, _select(names, which, "transport fields"),
                                 self._bin_shape(bins), np.float64, *bins)
        out["fluid"] = self.bin_fluid_cells(*bins)
        return out

    def scalar_profile(self, axis: int, which=None):
        """{name: float64[n_axis]}: the sums over every plane normal to `axis` (0 = x, 1 = y, 2 = z) of the
        requested transport terms, and "fluid"."""
        extent = self._shape()[::-1]                              # x first
        if not 0 <= int(axis) < len(extent):
            raise ValueError(f"axis is one of 0..{len(extent) - 1}")
        bins = tuple(1 if c == int(axis) else n for c, n in enumerate(extent))
        return {n: a.reshape(-1) for n, a in self.scalar_binned(*bins, which=which).items()}

    def nusselt(self, axis: int, dphi: float, height: float):
        """float64[n_axis]: per plane normal to `axis` the flux through the faces on its high side over
        what pure conduction carries across `height` cells with the scalar difference dphi, area D dphi /
        height (lio.nusselt_number).  Reads two scalar planes and nothing else.  In a steady state the
        entries between a hot and a cold wall are equal."""
        extent = self._shape()[::-1]
        name = "f" + "xyz"[int(axis)]
        flux = self.scalar_profile(axis, which=(name,))[name]
        area = int(np.prod(extent)) // extent[int(axis)]
        d = (1.0 / self._scalar_omega - 0.5) / (3.0 if len(extent) == 2 else 4.0)
        return flux / (area * d * float(dphi) / float(height))

    def transport_history(self, steps: int, every: int, *bins, which=None, accel=None, phi_ref: float = 0.0,
                          stride: int = 1):
        """run_thermal(every, accel, phi_ref, stride) chunk after chunk when `accel` is given, else
        run_scalar(every, stride) (the remainder last), scalar_binned(*bins, which) after each.  Returns
        {name: float64[samples, ...]} of the stacked samples, "step": the steps done at each sample, and
        "fluid".  The operator is linear: sums of the samples over time are the binned time sums, so time
        means of the scalar and its fluxes at bin resolution are means of these samples."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        which = _select(self._SBIN_FIELDS, which, "transport fields")
        samples, at, done = [], [], 0
        while done < steps:
            n = min(every, steps - done)
            if accel is None:
                self.run_scalar(n, stride)
            else:
                self.run_thermal(n, accel, phi_ref, stride)
            done += n
            samples.append(self.scalar_binned(*bins, which=which))
            at.append(done)
        shape = self._bin_shape(tuple(int(b) for b in bins))
        out = {n: (np.stack([s[n] for s in samples]) if samples else np.zeros((0,) + shape)) for n in which}
        out["step"] = np.asarray(at, np.int64)
        out["fluid"] = self.bin_fluid_cells(*bins)
        return out


    # wall models and the per-body wall flux (include/lbm_scalar_walls_hip.h)

    _scalar_nbodies = 0

    def scalar_walls(self, labels, kinds=None, values=None) -> None:
        """Give the bodies of `labels` (int32 map of the full domain, e.g. lio.label_bodies; negative =
        no body, adiabatic) a wall model each: kinds[b] in ("adiabatic", "value", "flux") or 0..2 and
        values[b], the wall value or the scalar added per link and step.  From the next scalar_advance
        on every step is lio.scalar_step[3d], then lio.scalar_apply_walls[3d], then the fixed list, bit
        for bit.  scalar_walls(None, 0) clears the walls; scalar_begin and scalar_end drop them."""
        if labels is None:
            self._check(self._fn("scalar_set_walls")(self._h, None, 0, None, None))
            self._scalar_nbodies = 0
            return
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.size != int(np.prod(self._shape())):
            raise ValueError("labels must cover the full domain")
        kind, value = _wall_table(kinds, values)
        self._check(self._fn("scalar_set_walls")(self._h, _ptr(lab), kind.size, _ptr(kind), _ptr(value)))
        self._scalar_nbodies = int(kind.size)

    def scalar_wall_values(self, kinds, values) -> None:
        """Replace the per-body table alone (as many bodies as scalar_walls set): a wall value that
        changes in time.  The wall list is not rebuilt."""
        kind, value = _wall_table(kinds, values)
        self._check(self._fn("scalar_set_walls")(self._h, None, kind.size, _ptr(kind), _ptr(value)))

    def scalar_wall_flux(self):
        """(q, links): the scalar all wall cells handed to the fluid in the last scalar step (the fp64 sum
        of the fp32 per-cell values, folded in a fixed order) and the links of all wall cells."""
        q, links = ctypes.c_double(), ctypes.c_int64()
        self._check(self._fn("scalar_wall_flux")(self._h, ctypes.byref(q), ctypes.byref(links)))
        return q.value, links.value

    def scalar_body_flux(self):
        """(q[nbodies], links[nbodies]) of the bodies scalar_walls set, summed on the device."""
        n = self._scalar_nbodies
        q, links = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.int64)
        self._check(self._fn("scalar_body_flux")(self._h, _ptr(q), _ptr(links), n))
        return q[:n], links[:n]

    def scalar_wall_flux_field(self):
        """float32 map of the per-cell wall flux, +0 off the walls -- lio.scalar_wall_flux_cells[3d] of
        scalar(populations=True), bit for bit."""
        q = np.zeros(self._shape(), np.float32)
        self._check(self._fn("scalar_store_wall_flux")(self._h, _ptr(q)))
        return q

    def wall_flux_history(self, steps: int, every: int, accel=None, phi_ref: float = 0.0, stride: int = 1):
        """run_thermal(every, accel, phi_ref, stride) chunk after chunk when `accel` is given, else
        run_scalar(every, stride) (the remainder last), scalar_body_flux() after each.  Returns
        {"step": int64[samples], "q": float64[samples, nbodies], "links": int64[nbodies]}."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        samples, at, done = [], [], 0
        links = np.zeros(self._scalar_nbodies, np.int64)
        while done < steps:
            n = min(every, steps - done)
            if accel is None:
                self.run_scalar(n, stride)
            else:
                self.run_thermal(n, accel, phi_ref, stride)
            done += n
            q, links = self.scalar_body_flux()
            samples.append(q)
            at.append(done)
        return {"step": np.asarray(at, np.int64),
                "q": np.stack(samples) if samples else np.zeros((0, self._scalar_nbodies)), "links": links}


class _Forcing:
    """Forcing zones (include/lbm_forcing_hip.h): a body force, a linear drag and a velocity target on boxes
    of cells, applied as an impulse on the stored populations between runs.  Both engines."""

    def forcing_zone(self, index: int, origin, shape=None, lam=0.0, target=None, force=None) -> None:
        """Set zone `index` (0 .. 7) to the box of `shape` = (w, h[, d]) cells at `origin` = (x0, y0[, z0])
        (shape None: from the origin to the domain's far corner; an extent 0 removes the zone).  Per cell and
        flow step the zone closes the share `lam` of the gap between the cell's velocity and `target`
        = (utx, uty[, utz]) and accelerates it by `force` = (fx, fy[, fz]); each of lam and the components is
        a number or a float32 array of the box's shape, slowest axis first ([h][w] or [d][h][w])."""
        dims = len(self._shape())
        origin = [int(v) for v in origin]
        if len(origin) != dims:
            raise ValueError(f"origin has {dims} components")
        if shape is None:
            shape = [n - o for n, o in zip(self._shape()[::-1], origin)]
        shape = [int(v) for v in shape]
        if len(shape) != dims:
            raise ValueError(f"shape has {dims} components")
        keep, table, konst = _forcing_coefs(dims, shape[::-1], lam, target, force)
        self._check(self._fn("forcing_set_zone")(self._h, int(index), *origin, *shape, table, konst))

    def forcing_clear(self) -> None:
        """Remove every zone and free its coefficients."""
        self._check(self._fn("forcing_clear")(self._h))

    def forcing_zones(self):
        """The indices of the zones set, ascending."""
        n, mask = ctypes.c_int32(), ctypes.c_uint32()
        self._check(self._fn("forcing_zones")(self._h, ctypes.byref(n), ctypes.byref(mask)))
        out = [i for i in range(FORCING_MAX_ZONES) if mask.value >> i & 1]
        assert len(out) == n.value
        return out

    def forcing_apply(self, steps: float = 1.0, impulse: bool = False):
        """Apply every zone once, in index order, as the impulse of `steps` flow steps: lio.forcing_kick[3d] of
        store(), zone after zone, bit for bit.  A run afterwards continues as from load_cells of the kicked
        cells.  impulse=True returns float64[8][dims], the momentum each zone added (rows of unset zones 0);
        else None.  steps = 0 or no zone launches nothing."""
        out = np.zeros((FORCING_MAX_ZONES, len(self._shape())), np.float64) if impulse else None
        self._check(self._fn("forcing_apply")(self._h, float(steps), _ptr(out) if impulse else None))
        return out

    def run_forced(self, steps: int, stride: int = 1, accelerate_first: bool = False):
        """Advance the flow under the zones: per chunk of n <= stride steps "forcing_apply(n), then
        run_steps(n)" (the remainder last).  stride = 1 is the exact first-order splitting; a larger stride
        applies the impulse of n steps at once and keeps the flow on its fused launches.  Returns the
        float32[steps] concatenation of the chunks' average velocities (D3Q19: empty).  To drive a thermal run
        through zones as well, compose by hand: per chunk forcing_apply(n), scalar_buoyancy(n * accel),
        run_steps(n), scalar_advance(n); run_thermal itself knows nothing of the zones."""
        return self._chunks(steps, stride, accelerate_first, True, lambda n, done: None,
                            before=lambda n: self.forcing_apply(n))

    def forcing_history(self, steps: int, every: int, stride: int = 1, accelerate_first: bool = False):
        """run_forced(every, stride) chunk after chunk (the remainder last) with the impulse taken at every
        application: a list of (step, float64[8][dims] impulse summed over the chunk).  accelerate_first
        applies to the first chunk (D2Q9)."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        out, done = [], 0
        while done < steps:
            n = min(every, steps - done)
            total = np.zeros((FORCING_MAX_ZONES, len(self._shape())), np.float64)

            def kick(m, total=total):
                total += self.forcing_apply(m, impulse=True)
            self._chunks(n, stride, accelerate_first and done == 0, False, lambda m, d: None, before=kick)
            done += n
            out.append((done, total))
        return out


class _Sgs:
    """Sub-grid model (include/lbm_sgs_hip.h): a local relaxation rate -- a Smagorinsky eddy viscosity or a
    prescribed rate that varies in space -- by rescaling the stored non-equilibrium part of every cell between
    runs.  No step kernel changes.  Both engines."""

    def sgs_model(self, kind, coef=0.0) -> None:
        """Set the model: kind "smagorinsky" with coef = Cs (>= 0), "omega" with coef = the relaxation rate
        wanted, in (0, 2), or "off" (frees it).  coef is a number or a float32 array of the domain's shape; a
        cell with Cs = 0, or with the handle's own omega, is left alone (a wall-damped Cs, a viscosity sponge)."""
        mode = _sgs_mode(kind, off=True)
        keep, ptr, konst = (None, None, 0.0) if mode == SGS_OFF else _sgs_coef(coef, self._shape())
        self._check(self._fn("sgs_set")(self._h, mode, konst, ptr))

    def sgs_apply(self, steps: float = 1.0, stats: bool = False):
        """One application standing for `steps` flow steps: lio.sgs_filter[3d] of store(), bit for bit.  A run
        afterwards continues as from load_cells of the filtered cells.  stats=True returns (cells that were
        not idle, float64 sum of their nu_add, max(0, largest nu_add)); else None.  steps = 0 or no model
        launches nothing."""
        out = np.zeros(3, np.float64) if stats else None
        self._check(self._fn("sgs_apply")(self._h, float(steps), _ptr(out) if stats else None))
        return (int(out[0]), float(out[1]), float(out[2])) if stats else None

    def eddy_viscosity(self) -> np.ndarray:
        """float32 array of the domain's shape: nu_add of every cell as sgs_apply(1) would form it from the
        current lattice, 0 where the cell would be left alone.  The lattice is not touched.  Call it on a lattice
        that comes from run_steps: after sgs_apply the stored non-equilibrium part is already rescaled and the
        result is low by (1 - w_eff) / (1 - omega)."""
        nut = np.zeros(self._shape(), np.float32)
        self._check(self._fn("sgs_store_nut")(self._h, _ptr(nut)))
        return nut

    def run_les(self, steps: int, stride: int = 1, accelerate_first: bool = False, forced: bool = False):
        """Advance the flow under the model: per chunk of n <= stride steps "run_steps(n), then sgs_apply(n)"
        (the remainder last).  The filter follows the step it corrects and comes before any kick of the next
        chunk.  stride = 1 is the exact model: every step's collision is one with the local rate.  A larger
        stride keeps the flow on its fused launches and applies the correction of n steps at once, first-order
        lumping as in run_forced.  forced=True puts forcing_apply(n) ahead of each chunk's run_steps(n), which
        is run_forced under the model.  Returns the float32[steps] concatenation of the chunks' average
        velocities (D3Q19: empty).  To combine the model with a buoyant scalar, compose by hand: per chunk
        forcing_apply(n), scalar_buoyancy(n * accel), run_steps(n), sgs_apply(n), scalar_advance(n); run_forced
        and run_thermal themselves know nothing of the model.  What params.accel adds (the D2Q9 inlet row, the
        D3Q19 body force) is added after the collision and is scaled with the rest: use accel = 0 or zones."""
        return self._chunks(steps, stride, accelerate_first, True, lambda n, done: self.sgs_apply(n),
                            before=(lambda n: self.forcing_apply(n)) if forced else None)

    def les_history(self, steps: int, every: int, stride: int = 1, accelerate_first: bool = False,
                    forced: bool = False):
        """run_les(every, stride, forced=forced) chunk after chunk (the remainder last) with the statistics of the last
        application of each chunk: a list of (step, cells, mean nu_add over those cells, max nu_add)."""
        steps, every = int(steps), int(every)
        if steps < 0 or every < 1:
            raise ValueError("steps >= 0 and every >= 1")
        out, done = [], 0
        while done < steps:
            n = min(every, steps - done)
            last = [(0, 0.0, 0.0)]

            def after(m, d, last=last):
                last[0] = self.sgs_apply(m, stats=True)
            self._chunks(n, stride, accelerate_first and done == 0, False, after,
                         before=(lambda m: self.forcing_apply(m)) if forced else None)
            done += n
            cells, total, peak = last[0]
            out.append((done, cells, total / cells if cells else 0.0, peak))
        return out


class Engine(_Handle, _WallForces, _Averages, _Gradients, _Stress, _Binned, _Tracers, _Scalar, _Forcing, _Sgs):
    """One lbm_handle: the HIP counterpart of the reference's poplar::Engine."""

    _PREFIX = "lbm_"
    _AVG_FIELDS = AVG_FIELDS
    _GRAD_FIELDS = GRAD_FIELDS
    _STRESS_FIELDS = STRESS_FIELDS
    _BIN_FIELDS = BIN_FIELDS
    _TRACER_FIELDS = TRACER_FIELDS
    _SCALAR_Q = SCALAR_Q
    _SBIN_FIELDS = SBIN_FIELDS

    def __init__(self, params, obstacles: np.ndarray, num_gpus: int = 1, *, parts: int | None = None,
                 grid=(0, 0), transport: int = TRANSPORT_LOCAL, rank: int = 0, world: int = 1,
                 devices=None, unique_id: bytes | None = None, kernel: int = KERNEL_AUTO,
                 graph_steps: int = 0, flags: int = 0, steps_per_launch: int = 0):
        self._L = load_library()
        self.params = Params(int(params.nx), int(params.ny), int(params.max_iters), int(params.reynolds_dim),
                             float(params.density), float(params.accel), float(params.omega))
        obst = np.ascontiguousarray(obstacles, dtype=np.uint8)
        if obst.size != self.params.nx * self.params.ny:
            raise ValueError("obstacles must have ny*nx entries")
        cfg = self._config(devices, unique_id)
        cfg.parts = int(parts if parts is not None else (world if transport == TRANSPORT_RCCL else num_gpus))
        cfg.grid_rows, cfg.grid_cols = int(grid[0]), int(grid[1])
        cfg.transport = transport
        cfg.rank, cfg.world = int(rank), int(world)
        cfg.kernel = kernel
        cfg.graph_steps = graph_steps
        cfg.flags = flags
        cfg.steps_per_launch = int(steps_per_launch)
        self._create("create_ex", obst, cfg)

    def _shape(self):
        return (self.params.ny, self.params.nx)

    def _local(self, name, names, which, table=True):
        """[{name: float32[h][w]}] per local rect of the packed arrays the engine's `name` writes."""
        rects = self.local_rects()
        packed = self._store_fields(name, names, which, int(self._L.lbm_local_cells(self._h)), np.float32,
                                    table=table)
        return _per_rect(rects, packed)

    def force_history(self, steps: int, every: int, accelerate_first: bool = False):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and sample
        wall_force() after each chunk.  Returns (samples, av_vels): samples is a list of
        (step, fx, fy, links) with step = steps done so far, av_vels the float32[steps]
        concatenation of the chunks' average velocities.  accelerate_first applies to the
        first chunk only.  In bitwise mode the lattice and av_vels equal those of one
        run_steps(steps).  In tolerance mode a chunked run differs from an unchunked one
        in the last bits: the steps of a chunk that do not fill a fused launch run as
        remainder launches, and remainder launches are bitwise."""
        return self._stat_history(steps, every, accelerate_first, self.wall_force)

    def gradient_history(self, steps: int, every: int, accelerate_first: bool = False):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and sample
        gradient_stats() after each chunk.  Returns (samples, av_vels): samples is a list of
        (step, sum_w2, sum_s2, max_w, max_div) with step = steps done so far, av_vels the
        float32[steps] concatenation of the chunks' average velocities.  Chunking behaves
        as in force_history."""
        return self._stat_history(steps, every, accelerate_first, self.gradient_stats)

    def strain_history(self, steps: int, every: int, accelerate_first: bool = False):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and sample
        strain_stats() after each chunk.  Returns (samples, av_vels): samples is a list of
        (step, sum_s2, max_strain, wall_cells, sum_wall_strain, max_wall_strain), av_vels the
        float32[steps] concatenation of the chunks' average velocities.  Chunking behaves
        as in force_history."""
        return self._stat_history(steps, every, accelerate_first, self.strain_stats)

    def run_averaged(self, steps: int, every: int, accelerate_first: bool = False):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and
        avg_sample() after each chunk (avg_begin first).  Returns the float32[steps]
        concatenation of the chunks' average velocities.  accelerate_first applies to the
        first chunk only.  In bitwise mode the lattice and av_vels equal those of one
        run_steps(steps).  In tolerance mode a chunked run differs from an unchunked one
        in the last bits: the steps of a chunk that do not fill a fused launch run as
        remainder launches, and remainder launches are bitwise."""
        return self._chunks(steps, every, accelerate_first, True, lambda n, done: self.avg_sample())

    def strain_rate_local(self, which=None):
        """[{name: float32[h][w]}] per local rect (local_rects() order; lbm_store_stress_local)."""
        return self._local("store_stress_local", STRESS_FIELDS, _select(STRESS_FIELDS, which, "strain-rate fields"))

    def gradients_local(self, which=None):
        """[{name: float32[h][w]}] per local rect (local_rects() order; lbm_store_gradients_local)."""
        return self._local("store_gradients_local", GRAD_FIELDS, _select(GRAD_FIELDS, which, "gradient fields"))

    def load_cells(self, cells: np.ndarray) -> None:
        c = np.ascontiguousarray(cells, dtype=np.float32)
        if c.size != self.params.nx * self.params.ny * Q:
            raise ValueError("cells must be AoS float32[ny][nx][9]")
        self._check(self._L.lbm_load_cells(self._h, _ptr(c)))

    def init_equilibrium(self) -> None:
        self._check(self._L.lbm_init_equilibrium(self._h))

    def run(self) -> None:
        self._check(self._L.lbm_run(self._h))

    def run_steps(self, steps: int, accelerate_first: bool = False) -> None:
        self._check(self._L.lbm_run_steps(self._h, int(steps), 1 if accelerate_first else 0))

    def store(self, cells: bool = True, n_av: int | None = None):
        """Returns (cells AoS float32[ny][nx][9] or None, av_vels float32[n_av])."""
        n_av = int(self.params.max_iters if n_av is None else n_av)
        out = np.zeros((self.params.ny, self.params.nx, Q), np.float32) if cells else None
        av = np.zeros(max(n_av, 1), np.float32)
        self._check(self._L.lbm_store(self._h, _ptr(out) if cells else None, _ptr(av), n_av))
        return out, av[:n_av]

    def load_cells_local(self, blocks) -> None:
        """This handle's sub-domains only: one AoS float32[h][w][9] per local rect
        (local_rects() order), as lbm_load_cells_local takes them packed."""
        rects = self.local_rects()
        if len(blocks) != len(rects):
            raise ValueError("one block per local rect")
        for b, (_, _, w, h) in zip(blocks, rects):
            if tuple(np.shape(b)) != (h, w, Q):
                raise ValueError(f"block shape {np.shape(b)} != {(h, w, Q)}")
        packed = np.ascontiguousarray(np.concatenate([np.asarray(b, np.float32).reshape(-1) for b in blocks]))
        assert packed.size == int(self._L.lbm_local_cells(self._h)) * Q
        self._check(self._L.lbm_load_cells_local(self._h, _ptr(packed)))

    def store_local(self, cells: bool = True, n_av: int | None = None):
        """Returns ([AoS float32[h][w][9] per local rect] or None, av_vels float32[n_av])."""
        n_av = int(self.params.max_iters if n_av is None else n_av)
        rects = self.local_rects()
        packed = np.zeros(int(self._L.lbm_local_cells(self._h)) * Q, np.float32) if cells else None
        av = np.zeros(max(n_av, 1), np.float32)
        self._check(self._L.lbm_store_local(self._h, _ptr(packed) if cells else None, _ptr(av), n_av))
        return (_per_rect(rects, packed, Q) if cells else None), av[:n_av]

    def fields(self, which=FIELDS):
        """{name: float32[ny][nx]} of the requested macroscopic fields ("ux", "uy",
        "speed", "pressure"), computed on the device from the current lattice
        (lbm_store_fields): the values lio.macroscopic derives from store()'s
        cells, bit for bit.  RCCL: only this rank's rectangle is written."""
        return self._store_fields("store_fields", FIELDS, _select(FIELDS, which, "fields"), self._shape(), np.float32,
                                  table=False)

    def fields_local(self, which=FIELDS):
        """[{name: float32[h][w]}] per local rect (local_rects() order; lbm_store_fields_local)."""
        return self._local("store_fields_local", FIELDS, _select(FIELDS, which, "fields"), table=False)

    def field_stats(self):
        """(mass, max_speed) of this handle's sub-domains (lbm_field_stats): the fp64
        sum of every cell's fp32 density and the largest |u| over fluid cells."""
        mass, umax = ctypes.c_double(), ctypes.c_float()
        self._check(self._L.lbm_field_stats(self._h, ctypes.byref(mass), ctypes.byref(umax)))
        return mass.value, umax.value

    def last_run_seconds(self) -> float:
        s = ctypes.c_double()
        self._check(self._L.lbm_last_run_seconds(self._h, ctypes.byref(s)))
        return s.value

    def total_free_cells(self) -> int:
        return int(self._L.lbm_total_free_cells(self._h))

    def local_rects(self):
        n = ctypes.c_int32()
        self._check(self._L.lbm_local_rects(self._h, None, 0, ctypes.byref(n)))
        rects = (Rect * max(n.value, 1))()
        self._check(self._L.lbm_local_rects(self._h, rects, n.value, ctypes.byref(n)))
        return [(q.x0, q.y0, q.w, q.h) for q in rects[:n.value]]

    def kernel_in_use(self) -> str:
        return {KERNEL_SCALAR: "scalar", KERNEL_VEC4: "vec4", KERNEL_STEP2: "step2", KERNEL_STREAM: "stream",
                KERNEL_RESIDENT: "resident", KERNEL_PIPELINE: "pipeline"}[
            int(self._L.lbm_kernel_in_use(self._h))]

    def steps_per_launch(self) -> int:
        return int(self._L.lbm_steps_per_launch(self._h))

    def run_stats(self):
        """(fused launches, one-step launches) of the last run."""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.lbm_run_stats(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def stream_units(self):
        """[(sub, boundary, x0, y0, w, h, reads_obstacle)] per work unit of the stream
        kernel (lbm_stream_units): per local rect the interior launch's units, then
        the boundary launch's; x0, y0, w, h are the owned cells, sub-domain-local;
        reads_obstacle is the flag the kernel reads (-1: the handle keeps none)."""
        n = ctypes.c_int32()
        self._check(self._L.lbm_stream_units(self._h, None, 0, ctypes.byref(n)))
        buf = (StreamUnit * max(n.value, 1))()
        self._check(self._L.lbm_stream_units(self._h, buf, n.value, ctypes.byref(n)))
        return [(u.sub, u.boundary, u.x0, u.y0, u.w, u.h, u.reads_obstacle) for u in buf[:n.value]]

    def profile_summary(self):
        """[{name, launches, total_ms, min_ms, max_ms}] per launch class (LBM_FLAG_PROFILE handles)."""
        n = ctypes.c_int32()
        self._check(self._L.lbm_profile_summary(self._h, None, 0, ctypes.byref(n)))
        buf = (KernelTime * max(n.value, 1))()
        self._check(self._L.lbm_profile_summary(self._h, buf, n.value, ctypes.byref(n)))
        return [{"name": k.name.decode(), "launches": k.launches, "total_ms": k.total_ms, "min_ms": k.min_ms,
                 "max_ms": k.max_ms} for k in buf[:n.value]]

    def profile_reset(self) -> None:
        self._check(self._L.lbm_profile_reset(self._h))

    def placement(self):
        """(kept pair or -1, [ms per launch of each pair tried]) of the placement probe."""
        kept, tried = ctypes.c_int32(), ctypes.c_int32()
        ms = (ctypes.c_float * 16)()
        self._check(self._L.lbm_placement_probe(self._h, ctypes.byref(kept), ctypes.byref(tried), ms, 16))
        return kept.value, [ms[i] for i in range(min(tried.value, 16))]

    def nonfinite_count(self) -> int:
        """NaN / Inf populations in the current lattice (device scan)."""
        n = ctypes.c_int64()
        self._check(self._L.lbm_nonfinite_count(self._h, ctypes.byref(n)))
        return n.value

    def numerics(self) -> str:
        """'bitwise' (every kernel equals the CPU oracle) or 'tolerance' (LBM_FLAG_TOLERANCE collision)."""
        return "tolerance" if int(self._L.lbm_numerics(self._h)) == 1 else "bitwise"


class Engine3D(_Handle, _WallForces, _Averages, _Gradients, _Stress, _Binned, _Tracers, _Scalar, _Forcing, _Sgs):
    """One lbm3d_handle: the D3Q19 extension engine (include/lbm3d_hip.h)."""

    _PREFIX = "lbm3d_"
    _AVG_FIELDS = AVG_FIELDS3D
    _GRAD_FIELDS = GRAD_FIELDS3D
    _STRESS_FIELDS = STRESS_FIELDS3D
    _BIN_FIELDS = BIN_FIELDS3D
    _TRACER_FIELDS = TRACER_FIELDS3D
    _SCALAR_Q = SCALAR_Q3D
    _SBIN_FIELDS = SBIN_FIELDS3D

    def __init__(self, params, obstacles: np.ndarray, *, parts: int = 1, transport: int = TRANSPORT_LOCAL,
                 rank: int = 0, world: int = 1, devices=None, unique_id: bytes | None = None, flags: int = 0):
        self._L = load_library()
        self.params = Params3D(int(params.nx), int(params.ny), int(params.nz), int(params.max_iters),
                               float(params.density), float(params.accel), float(params.omega))
        obst = np.ascontiguousarray(obstacles, dtype=np.uint8)
        if obst.size != self.params.nx * self.params.ny * self.params.nz:
            raise ValueError("obstacles must have nz*ny*nx entries")
        cfg = self._config(devices, unique_id)
        cfg.parts = int(world if transport == TRANSPORT_RCCL else parts)
        cfg.transport = transport
        cfg.flags = int(flags)  # FLAG_TOLERANCE: the two-step passes use the reciprocal collision
        cfg.rank, cfg.world = int(rank), int(world)
        self._create("create", obst, cfg)

    def _shape(self):
        return (self.params.nz, self.params.ny, self.params.nx)

    # The three chunked runs below keep their own D3Q19 signatures (no accelerate_first, no av_vels),
    # so they stay thin wrappers beside Engine's instead of one declaration on the mixins.
    def gradient_history(self, steps: int, every: int):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and sample
        gradient_stats() after each chunk: a list of (step, sum_w2, sum_s2, max_w, max_div)."""
        return self._stat_history(steps, every, False, self.gradient_stats)[0]

    def strain_history(self, steps: int, every: int):
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and sample
        strain_stats() after each chunk: a list of (step, sum_s2, max_strain, wall_cells,
        sum_wall_strain, max_wall_strain)."""
        return self._stat_history(steps, every, False, self.strain_stats)[0]

    def run_averaged(self, steps: int, every: int) -> None:
        """Advance `steps` steps in run_steps(every) chunks (the remainder last) and
        avg_sample() after each chunk (avg_begin first).  In bitwise mode the lattice
        equals that of one run_steps(steps); in tolerance mode a chunked run differs from
        an unchunked one in the last bits (remainder launches are bitwise)."""
        self._chunks(steps, every, False, False, lambda n, done: self.avg_sample())

    def strain_rate_box(self, x0: int, y0: int, z0: int, nx: int, ny: int, nz: int, which=None):
        """{name: float32[nz][ny][nx]} of the cells [x0, x0+nx) x [y0, y0+ny) x [z0, z0+nz)
        (lbm3d_store_stress_box); a box that is empty or leaves the domain raises LbmError."""
        return self._box("store_stress_box", STRESS_FIELDS3D, _select(STRESS_FIELDS3D, which, "strain-rate fields"),
                         (x0, y0, z0, nx, ny, nz))

    def gradients_box(self, x0: int, y0: int, z0: int, nx: int, ny: int, nz: int, which=None):
        """{name: float32[nz][ny][nx]} of the cells [x0, x0+nx) x [y0, y0+ny) x [z0, z0+nz)
        (lbm3d_store_gradients_box).  The stencils of the box's outer cells still read
        their periodic neighbours; a box that is empty or leaves the domain raises LbmError."""
        return self._box("store_gradients_box", GRAD_FIELDS3D, _select(GRAD_FIELDS3D, which, "gradient fields"),
                         (x0, y0, z0, nx, ny, nz))

    def fields_box(self, x0: int, y0: int, z0: int, nx: int, ny: int, nz: int, which=FIELDS3D):
        """{name: float32[nz][ny][nx]} of the cells [x0, x0+nx) x [y0, y0+ny) x [z0, z0+nz)
        (lbm3d_store_fields_box; a plane is a box of extent 1 along its normal).  No
        periodic wrap: a box that is empty or leaves the domain raises LbmError."""
        return self._box("store_fields_box", FIELDS3D, _select(FIELDS3D, which, "fields"), (x0, y0, z0, nx, ny, nz),
                         table=False)

    def _box(self, name, names, which, extent, table=True):
        box = Box3D(*[int(v) for v in extent])
        shape = (max(box.nz, 0), max(box.ny, 0), max(box.nx, 0))
        return self._store_fields(name, names, which, shape, np.float32, ctypes.byref(box), table=table)

    def init_equilibrium(self) -> None:
        self._check(self._L.lbm3d_init_equilibrium(self._h))

    def load_cells(self, cells: np.ndarray) -> None:
        c = np.ascontiguousarray(cells, dtype=np.float32)
        if c.size != self.params.nx * self.params.ny * self.params.nz * Q3:
            raise ValueError("cells must be AoS float32[nz][ny][nx][19]")
        self._check(self._L.lbm3d_load_cells(self._h, _ptr(c)))

    def run_steps(self, steps: int) -> None:
        self._check(self._L.lbm3d_run_steps(self._h, int(steps)))

    def store(self, cells: bool = True, n_av: int = 0):
        out = np.zeros((self.params.nz, self.params.ny, self.params.nx, Q3), np.float32) if cells else None
        av = np.zeros(max(int(n_av), 1), np.float32)
        self._check(self._L.lbm3d_store(self._h, _ptr(out) if cells else None, _ptr(av), int(n_av)))
        return out, av[:int(n_av)]

    def fields(self, which=FIELDS3D):
        """{name: float32[nz][ny][nx]} of the requested macroscopic fields ("ux", "uy",
        "uz", "speed", "pressure"), computed on the device from the current lattice
        (lbm3d_store_fields): the values lio.macroscopic3d derives from store()'s
        cells, bit for bit.  RCCL: only this rank's planes are written."""
        return self._store_fields("store_fields", FIELDS3D, _select(FIELDS3D, which, "fields"), self._shape(),
                                  np.float32, table=False)

    def field_stats(self):
        """(mass, max_speed) of this handle's slabs (lbm3d_field_stats): the fp64 sum of
        every cell's fp32 density and the largest |u| over fluid cells."""
        mass, umax = ctypes.c_double(), ctypes.c_float()
        self._check(self._L.lbm3d_field_stats(self._h, ctypes.byref(mass), ctypes.byref(umax)))
        return mass.value, umax.value

    def last_run_seconds(self) -> float:
        s = ctypes.c_double()
        self._check(self._L.lbm3d_last_run_seconds(self._h, ctypes.byref(s)))
        return s.value

    def run_stats(self):
        """(three-step passes, two-step passes, one-step launches, pair kernel) of the last
        run_steps (lbm3d_run_stats): one count per pass / step of the whole domain; the last
        entry is 1 when one-step launches use the column-pair kernel, 0 for the one-cell one."""
        v = [ctypes.c_int32() for _ in range(4)]
        self._check(self._L.lbm3d_run_stats(self._h, *[ctypes.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def numerics(self) -> str:
        """'tolerance' when this handle's two- / three-step passes run the reciprocal
        collision (FLAG_TOLERANCE and passes in use), else 'bitwise'.  One-step launches
        are bitwise in both modes."""
        return "tolerance" if int(self._L.lbm3d_numerics(self._h)) == 1 else "bitwise"

    def total_free_cells(self) -> int:
        return int(self._L.lbm3d_total_free_cells(self._h))

    def local_slabs(self):
        n = ctypes.c_int32()
        z0 = (ctypes.c_int32 * 64)()
        nz = (ctypes.c_int32 * 64)()
        self._check(self._L.lbm3d_local_slabs(self._h, z0, nz, 64, ctypes.byref(n)))
        return [(z0[i], nz[i]) for i in range(n.value)]
