/*
 * lbm3d_fields_hip.h -- macroscopic fields, box extracts and lattice
 * statistics of the D3Q19 engine (lbm3d_hip.h), computed on the device from
 * the current lattice.  An additive part of the C ABI of liblbm_hip.so
 * (LBM_ABI_VERSION unchanged): the counterpart of lbm_store_fields /
 * lbm_field_stats (lbm_hip.h) for 3-D, where lbm3d_store moves 76 B per cell
 * to the host and these move 4-20 B.
 *
 * Definition (IEEE fp32, no contraction, correctly rounded divide and sqrt)
 * from a cell's 19 stored populations s[0..18], speed order of lbm3d_hip.h --
 * the expressions the step itself forms from them (oracle/lbm_oracle3d.c
 * cell3d):
 *     rho      = s0 + s1 + ... + s18                       (left to right)
 *     ux       = ((s1+s5+s7+s10+s16) - (s2+s6+s8+s11+s15)) / rho
 *     uy       = ((s3+s5+s8+s12+s18) - (s4+s6+s7+s13+s17)) / rho
 *     uz       = ((s9+s10+s11+s12+s13) - (s14+s15+s16+s17+s18)) / rho
 *     speed    = sqrtf(ux*ux + uy*uy + uz*uz)              (left to right)
 *     pressure = rho * (1.f / 3.f)
 * An obstacle cell gives +0, +0, +0, +0, params.density * (1.f / 3.f) (the
 * convention of lbm_store_fields).  The fields are a pure function of the
 * stored populations: the same bits whatever pass form or numerics mode
 * advanced the lattice, and the bits the same expressions give on the host
 * from lbm3d_store's cells.
 *
 * All three calls block, read the current lattice and change no engine state
 * (a run afterwards continues bit-identically); LBM_E_INVALID for a NULL
 * handle, LBM_E_STATE before lbm3d_load_cells / lbm3d_init_equilibrium.
 */
#ifndef LBM3D_FIELDS_HIP_H
#define LBM3D_FIELDS_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Cells [x0, x0+nx) x [y0, y0+ny) x [z0, z0+nz) of the domain. */
typedef struct lbm3d_box {
    int32_t x0, y0, z0;
    int32_t nx, ny, nz;
} lbm3d_box;

/* Planar float[nz][ny][nx] per field, full domain.  A NULL field is neither
 * computed nor copied (all NULL: nothing is done).  LOCAL transport writes
 * every slab; RCCL writes this rank's planes only and leaves the rest of the
 * arrays untouched, as lbm3d_store does. */
int lbm3d_store_fields(lbm3d_handle *h, float *ux, float *uy, float *uz, float *speed, float *pressure);

/* The same fields for the cells of `box`, packed float[box.nz][box.ny][box.nx].
 * A plane is a box of extent 1 along its normal.  No periodic wrap: a box
 * with a non-positive extent or one that leaves the domain is LBM_E_INVALID.
 * A box may span several slabs; RCCL writes only the part inside this rank's
 * slab.  Only the box's bytes cross to the host, and the device staging is
 * sized by the box. */
int lbm3d_store_fields_box(lbm3d_handle *h, const lbm3d_box *box, float *ux, float *uy, float *uz, float *speed,
                           float *pressure);

/* Over this handle's slabs: *mass = fp64 sum of every cell's fp32 density
 * (obstacle cells included), *max_speed = largest |u| of the fluid cells (0
 * when there are none).  Folded in a fixed order without atomics: two calls
 * on the same lattice return identical bits.  Either pointer may be NULL. */
int lbm3d_field_stats(lbm3d_handle *h, double *mass, float *max_speed);

#ifdef __cplusplus
}
#endif

#endif /* LBM3D_FIELDS_HIP_H */
