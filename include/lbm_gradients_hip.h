/*
 * lbm_gradients_hip.h -- vorticity, divergence, strain-rate magnitude and the
 * Q criterion (Okubo-Weiss in 2-D) of the current lattice, derived on the
 * device.  An additive part of the C ABI of liblbm_hip.so (LBM_ABI_VERSION
 * unchanged) for both engines: D2Q9 (lbm_hip.h) and D3Q19 (lbm3d_hip.h).
 *
 * These are the quantities that show a vortex street or the vortical
 * structures of a 3-D run; enstrophy and dissipation follow from two sums.
 * All come from the velocity gradient, so they are the first fields that need
 * a cell's neighbours: the engine carries velocities (never populations)
 * across sub-domain and slab borders, and nothing but the requested fields or
 * four numbers crosses to the host.  No step kernel changes.
 *
 * Definition, D2Q9.  The inputs are U = ux and V = uy exactly as
 * lbm_store_fields gives them for the current lattice: IEEE fp32, that
 * header's evaluation order, obstacle cells +0.  Neighbour indices are
 * periodic in the global domain (xe = x + 1 == nx ? 0 : x + 1, likewise xw,
 * yn, ys).  Everything below is IEEE fp32, in the written order, with no
 * contraction:
 *
 *     gxx = (U[y][xe] - U[y][xw]) * 0.5f      gxy = (U[yn][x] - U[ys][x]) * 0.5f
 *     gyx = (V[y][xe] - V[y][xw]) * 0.5f      gyy = (V[yn][x] - V[ys][x]) * 0.5f
 *     vorticity  = gyx - gxy
 *     divergence = gxx + gyy
 *     sxy        = (gxy + gyx) * 0.5f
 *     s2         = ((gxx*gxx) + (gyy*gyy)) + ((sxy*sxy) * 2.f)          // S:S
 *     strain     = sqrtf(s2)
 *     q          = (((gxx*gxx) + (gyy*gyy)) * -0.5f) - (gxy*gyx)        // -tr(G^2)/2 = (W:W - S:S)/2
 *
 * An obstacle cell reports +0 in every output.  A fluid cell next to a wall
 * uses the wall cell's 0 velocity at the cell centre: what a post-processor
 * would do with final_state.dat, and first order at a halfway bounce-back wall
 * (second-order wall-corrected differences are not built; lbm_stress_hip.h
 * gives a strain rate that is second order there, from the cell's own
 * non-equilibrium moments).  With nx == 1 or ny == 1 the two neighbours
 * coincide and the differences are +0.
 *
 * Definition, D3Q19.  The same with nine components
 * g_ab = (u_a[+b] - u_a[-b]) * 0.5f, periodic in x, y and z, from
 * lbm3d_store_fields' ux, uy, uz:
 *
 *     wx = gzy - gyz;  wy = gxz - gzx;  wz = gyx - gxy
 *     vorticity  = sqrtf(((wx*wx) + (wy*wy)) + (wz*wz))
 *     divergence = (gxx + gyy) + gzz
 *     sxy = (gxy+gyx)*0.5f;  sxz = (gxz+gzx)*0.5f;  syz = (gyz+gzy)*0.5f
 *     s2  = (((gxx*gxx)+(gyy*gyy))+(gzz*gzz)) + ((((sxy*sxy)+(sxz*sxz))+(syz*syz)) * 2.f)
 *     strain = sqrtf(s2)
 *     q   = ((((gxx*gxx)+(gyy*gyy))+(gzz*gzz)) * -0.5f) - (((gxy*gyx)+(gxz*gzx))+(gyz*gzy))
 *
 * Statistics, over the fluid cells of the handle's local sub-domains / slabs:
 *
 *     sum_w2  = sum of (double)vorticity * (double)vorticity
 *               (3-D: ((double)wx*wx + (double)wy*wy) + (double)wz*wz)
 *     sum_s2  = sum of (double)s2
 *     max_w   = max |vorticity|         max_div = max |divergence|
 *
 * The sums are fp64, folded lanes -> waves -> blocks in a fixed order with no
 * atomics; the per-block partials are folded by the host in block order,
 * sub-domain after sub-domain (as lbm_field_stats).  A repeat call returns
 * identical bits.  The enstrophy is sum_w2 / 2; the viscous dissipation is
 * 2 nu * sum_s2 with nu = (1 / omega - 1 / 2) / 3 from the handle's omega.  The
 * library returns the raw sums.
 *
 * Gradients of the time means need no entry point: the operator is linear, so
 * the same differences of lbm_avg_store's mean velocities are the mean
 * vorticity.
 *
 * Contract.  LBM_E_INVALID for a NULL handle.  Before load_cells /
 * init_equilibrium: LBM_E_STATE.  A call with every output NULL returns LBM_OK
 * and launches nothing.  Every call waits for the handle's streams, blocks,
 * and runs on the compute stream; it touches neither lattice nor its ping-pong
 * side, so a run afterwards continues bit-identically.  The edge-velocity
 * buffers (two rows and two columns per sub-domain, four planes per slab) are
 * allocated at the first call and freed by destroy: a handle that never asks
 * allocates and launches nothing.  On an LBM_FLAG_PROFILE handle (D2Q9) the
 * launches are accounted under "velocity_gradients" and "velocity_gradients
 * stats" (the edge kernel under "edge_velocities").
 *
 * Not built: an RCCL handle of world size > 1 returns LBM_E_INVALID with an
 * lbm_last_error text that says so -- its neighbours' edges live in other
 * processes, and the exchange could not be tested on a multi-GPU machine
 * (DESIGN.md section 9, item 5).  RCCL world 1, LBM_FLAG_FORCE_EXCHANGE
 * included, works: every neighbour is a local sub-domain.
 */
#ifndef LBM_GRADIENTS_HIP_H
#define LBM_GRADIENTS_HIP_H

#include <stdint.h>

#include "lbm3d_fields_hip.h"
#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* field indices of the arrays of output pointers */
enum {
    LBM_GRAD_VORTICITY = 0,
    LBM_GRAD_DIVERGENCE = 1,
    LBM_GRAD_STRAIN = 2,
    LBM_GRAD_Q = 3,
    LBM_GRAD_FIELDS = 4
};

enum {
    LBM3D_GRAD_WX = 0,
    LBM3D_GRAD_WY = 1,
    LBM3D_GRAD_WZ = 2,
    LBM3D_GRAD_VORTICITY = 3,
    LBM3D_GRAD_DIVERGENCE = 4,
    LBM3D_GRAD_STRAIN = 5,
    LBM3D_GRAD_Q = 6,
    LBM3D_GRAD_FIELDS = 7
};

/* Planar float[ny][nx] per field, each local sub-domain at its rectangle; a
 * NULL entry is neither computed nor staged. */
int lbm_store_gradients(lbm_handle *h, float *const out[LBM_GRAD_FIELDS]);

/* The local sub-domains' float[h][w] blocks packed in lbm_local_rects order. */
int lbm_store_gradients_local(lbm_handle *h, float *const out[LBM_GRAD_FIELDS]);

/* The four statistics above; a NULL pointer is skipped. */
int lbm_gradient_stats(lbm_handle *h, double *sum_w2, double *sum_s2, float *max_w, float *max_div);

/* D3Q19: planar float[nz][ny][nx] per field (this handle's planes). */
int lbm3d_store_gradients(lbm3d_handle *h, float *const out[LBM3D_GRAD_FIELDS]);

/* The cells of `box` into packed float[box.nz][box.ny][box.nx] arrays.  The
 * stencil of a cell on a face of the box still reads its periodic neighbours
 * outside it.  A box that is empty or leaves the domain: LBM_E_INVALID, as
 * lbm3d_store_fields_box. */
int lbm3d_store_gradients_box(lbm3d_handle *h, const lbm3d_box *box, float *const out[LBM3D_GRAD_FIELDS]);

int lbm3d_gradient_stats(lbm3d_handle *h, double *sum_w2, double *sum_s2, float *max_w, float *max_div);

#ifdef __cplusplus
}
#endif

#endif /* LBM_GRADIENTS_HIP_H */
