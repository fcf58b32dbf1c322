/*
 * lbm_stress_hip.h -- the strain-rate tensor and wall shear of the current
 * lattice from the non-equilibrium second moment of each cell's own
 * populations, derived on the device.  An additive part of the C ABI of
 * liblbm_hip.so (LBM_ABI_VERSION unchanged) for both engines: D2Q9
 * (lbm_hip.h) and D3Q19 (lbm3d_hip.h).
 *
 * In BGK the strain rate is proportional to the second moment of f - f_eq of
 * the cell itself, so no stencil is needed: the value is second-order accurate
 * at a halfway bounce-back wall, where the finite differences of
 * lbm_gradients_hip.h are first order, and nothing crosses a sub-domain
 * border.  The stored lattice is post-collision, and
 * (f - f_eq)_post = (1 - omega) (f - f_eq)_pre, hence with
 * P_ab = sum_k e_ka e_kb f_k
 *
 *     S_ab = -(3 omega / (2 rho (1 - omega))) (P_ab - rho/3 d_ab - rho u_a u_b)
 *
 * The body force both engines fold into the stored populations (the D2Q9 row
 * accelerate, the D3Q19 force on every cell) adds +-w1 / +-w2 pairs that
 * cancel in every second moment.  No step kernel changes.
 *
 * All arithmetic is IEEE fp32 in the written order with no contraction;
 * divide and sqrt are correctly rounded.
 *
 * Definition, D2Q9.  c[k] are the stored populations of the cell in the speed
 * order of lbm_hip.h; rho, ux, uy are exactly lbm_store_fields' values (rho
 * the sequential sum c0 + c1 + ... + c8).
 *
 *     pxx = ((((c1 + c3) + c5) + c6) + c7) + c8
 *     pyy = ((((c2 + c4) + c5) + c6) + c7) + c8
 *     pxy = (c5 + c7) - (c6 + c8)
 *     p   = rho * (1.f / 3.f)
 *     nxx = (pxx - p) - ((rho * ux) * ux)
 *     nyy = (pyy - p) - ((rho * uy) * uy)
 *     nxy = pxy - ((rho * ux) * uy)
 *     k   = coef / rho        coef = (-1.5f * omega) / (1.f - omega), formed once on the host in fp32
 *     sxx = nxx * k   syy = nyy * k   sxy = nxy * k
 *     s2     = ((sxx*sxx) + (syy*syy)) + ((sxy*sxy) * 2.f)          // S:S
 *     strain = sqrtf(s2)
 *
 * An obstacle cell reports +0 in every field.
 *
 * Definition, D3Q19.  Speed order of lbm3d_hip.h; rho, ux, uy, uz are
 * lbm3d_store_fields' values.  The diagonal sums run left to right in
 * ascending speed index:
 *
 *     pxx over speeds 1, 2, 5, 6, 7, 8, 10, 11, 15, 16
 *     pyy over speeds 3, 4, 5, 6, 7, 8, 12, 13, 17, 18
 *     pzz over speeds 9, 10, ..., 18
 *     pxy = (c5 + c6) - (c7 + c8)
 *     pxz = (c10 + c15) - (c11 + c16)
 *     pyz = (c12 + c17) - (c13 + c18)
 *
 * n_ab, k and s_ab as in 2-D, and
 *
 *     s2 = (((sxx*sxx)+(syy*syy))+(szz*szz)) + ((((sxy*sxy)+(sxz*sxz))+(syz*syz)) * 2.f)
 *     strain = sqrtf(s2)
 *
 * Near-wall cells.  A fluid cell is near-wall iff at least one of its 8 (18)
 * lattice neighbours is blocked, neighbours periodic over the full domain: the
 * fluid ends of the links lbm_forces_hip.h sums over.
 *
 * Statistics, over the fluid cells of the handle's local sub-domains / slabs:
 *
 *     sum_s2          = fp64 sum of (double)s2
 *     max_strain      = the largest strain
 *     wall_cells      = number of near-wall cells
 *     sum_wall_strain = fp64 sum of (double)strain over the near-wall cells
 *     max_wall_strain = the largest strain over the near-wall cells
 *
 * The sums are folded lanes -> waves -> blocks in a fixed order with no
 * atomics; the per-block partials are folded by the host in block order,
 * sub-domain after sub-domain (as lbm_gradient_stats).  A repeat call returns
 * identical bits.  The library returns the raw values; with
 * nu = (1 / omega - 1 / 2) / 3 the viscous dissipation is 2 nu * sum_s2, the
 * viscous stress 2 rho nu S, and in simple shear the wall shear stress is
 * rho nu sqrt(2) * strain.
 *
 * Precision floor.  The diagonal terms subtract rho / 3 from sums of that
 * size, so the absolute error of a component is of order 2^-21 * |coef|:
 * about 4e-7 at omega = 1.85, growing without bound as omega -> 1.
 *
 * Contract.  LBM_E_INVALID for a NULL handle.  Before load_cells /
 * init_equilibrium: LBM_E_STATE.  A call with every output NULL returns LBM_OK
 * and launches nothing.  Layout and RCCL rules are those of lbm_store_fields /
 * lbm3d_store_fields(_box); RCCL handles of any world size are accepted (the
 * computation is cell-local), and the statistics cover the local sub-domains.
 * Every call waits for the handle's streams, blocks, and runs on the compute
 * stream; it touches neither lattice nor its ping-pong side, so a run
 * afterwards continues bit-identically.  A handle whose omega gives
 * 1.f - omega == 0.f returns LBM_E_INVALID with an lbm_last_error text that
 * says why: at omega = 1 the post-collision lattice carries no non-equilibrium
 * part.  The near-wall map (one byte per local cell) is built from the
 * full-domain obstacle map at the first statistics call and freed by destroy:
 * a handle that never asks allocates and launches nothing extra.  On an
 * LBM_FLAG_PROFILE handle (D2Q9) the launches are accounted under "neq_strain"
 * and "neq_strain stats".
 */
#ifndef LBM_STRESS_HIP_H
#define LBM_STRESS_HIP_H

#include <stdint.h>

#include "lbm3d_fields_hip.h"
#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* field indices of the arrays of output pointers */
enum {
    LBM_STRESS_SXX = 0,
    LBM_STRESS_SXY = 1,
    LBM_STRESS_SYY = 2,
    LBM_STRESS_STRAIN = 3,
    LBM_STRESS_FIELDS = 4
};

enum {
    LBM3D_STRESS_SXX = 0,
    LBM3D_STRESS_SYY = 1,
    LBM3D_STRESS_SZZ = 2,
    LBM3D_STRESS_SXY = 3,
    LBM3D_STRESS_SXZ = 4,
    LBM3D_STRESS_SYZ = 5,
    LBM3D_STRESS_STRAIN = 6,
    LBM3D_STRESS_FIELDS = 7
};

/* Planar float[ny][nx] per field, each local sub-domain at its rectangle; a
 * NULL entry is neither computed nor staged. */
int lbm_store_stress(lbm_handle *h, float *const out[LBM_STRESS_FIELDS]);

/* The local sub-domains' float[h][w] blocks packed in lbm_local_rects order. */
int lbm_store_stress_local(lbm_handle *h, float *const out[LBM_STRESS_FIELDS]);

/* The five statistics above; a NULL pointer is skipped. */
int lbm_stress_stats(lbm_handle *h, double *sum_s2, float *max_strain, int64_t *wall_cells, double *sum_wall_strain,
                     float *max_wall_strain);

/* D3Q19: planar float[nz][ny][nx] per field (this handle's planes). */
int lbm3d_store_stress(lbm3d_handle *h, float *const out[LBM3D_STRESS_FIELDS]);

/* The cells of `box` into packed float[box.nz][box.ny][box.nx] arrays.  A box
 * that is empty or leaves the domain: LBM_E_INVALID, as lbm3d_store_fields_box. */
int lbm3d_store_stress_box(lbm3d_handle *h, const lbm3d_box *box, float *const out[LBM3D_STRESS_FIELDS]);

int lbm3d_stress_stats(lbm3d_handle *h, double *sum_s2, float *max_strain, int64_t *wall_cells,
                       double *sum_wall_strain, float *max_wall_strain);

#ifdef __cplusplus
}
#endif

#endif /* LBM_STRESS_HIP_H */
