/*
 * lbm_sgs_hip.h -- a sub-grid model: a local relaxation rate for the BGK
 * collision, as a Smagorinsky eddy viscosity or as a prescribed rate that
 * varies in space (a viscosity sponge).  An additive part of the C ABI of
 * liblbm_hip.so (LBM_ABI_VERSION unchanged) for both engines.  It needs no
 * scalar and no forcing zone and changes no other entry point.
 *
 * The mechanism.  No step kernel changes.  The stored populations are
 * post-collision, c = f + w0 (feq - f) with the handle's omega w0, and the
 * collision conserves the density and the momentum, so feq can be formed again
 * from c and c - feq = (1 - w0) (f - feq).  A cell that should have been
 * relaxed with w_eff instead of w0 is therefore obtained EXACTLY by rescaling
 * its stored non-equilibrium part,
 *
 *     c  <-  c + d (c - feq),     d = (w0 - w_eff) / (1 - w0),
 *
 * and applied after every step this IS a collision with a rate that varies
 * from cell to cell.  It holds wherever nothing was added to a cell's
 * populations after its collision.  The exceptions in these engines are the
 * increments of params.accel != 0, which the step adds after the collision:
 * the D2Q9 inlet acceleration (row ny - 2) and the D3Q19 body force (every
 * fluid cell).  The filter scales those increments too.  Drive a modelled
 * flow with accel = 0 or with forcing zones (lbm_forcing_hip.h), whose kick
 * comes before the step.
 *
 * Model.  mode LBM_SGS_SMAGORINSKY with the coefficient Cs (>= 0), or
 * LBM_SGS_OMEGA with the coefficient w1 in (0, 2), the rate wanted.  The
 * coefficient is one constant or a dense array float[ny][nx]
 * (float[nz][ny][nx]) over the whole domain; a cell with Cs == 0.f, or with
 * w1 == w0, is idle, which gives a wall-damped Cs or a sponge.
 *
 * Definition of one application.  IEEE fp32, every operation rounded
 * separately, as written, no contraction, correctly rounded divide and sqrt.
 * n (finite, > 0) is the number of flow steps the application stands for.
 * Once per application, from w0:
 *
 *     omo = 1.f - w0;   tau0 = 1.f / w0;   nu0 = (tau0 - 0.5f) / 3.f
 *
 * Per cell, D2Q9 (speeds 0 rest, 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW, 8 SE;
 * c_k the stored populations):
 *
 *     rho = 0.f + c0 + c1 + ... + c8                 (sequential)
 *     ux  = (((c1 + c5) + c8) - ((c3 + c6) + c7)) / rho
 *     uy  = (((c2 + c5) + c6) - ((c4 + c7) + c8)) / rho
 *
 * (lbm_store_fields' own), the equilibrium as the collision writes it,
 *
 *     usq = (ux * ux) + (uy * uy);       csq = 1.f - (usq * 1.5f)
 *     l0 = (4.f / 9.f) * rho;   l1 = rho / 9.f;   l2 = rho / 36.f
 *     P(l, v) = l * (((4.5f * v) * ((2.f / 3.f) + v)) + csq)
 *     M(l, v) = l * (((-4.5f * v) * ((2.f / 3.f) - v)) + csq)
 *     us = ux + uy;     ud = (-ux) + uy
 *     e0 = l0 * csq
 *     e1 = P(l1, ux)   e3 = M(l1, ux)   e2 = P(l1, uy)   e4 = M(l1, uy)
 *     e5 = P(l2, us)   e7 = M(l2, us)   e6 = P(l2, ud)   e8 = M(l2, ud)
 *
 * the non-equilibrium part q_k = c_k - e_k and its second moment
 *
 *     pxx = ((((q1 + q3) + q5) + q6) + q7) + q8
 *     pyy = ((((q2 + q4) + q5) + q6) + q7) + q8
 *     pxy = (q5 + q7) - (q6 + q8)
 *     p2  = ((pxx * pxx) + (pyy * pyy)) + ((pxy * pxy) * 2.f)
 *     pim = sqrtf(p2) / fabsf(omo)                   (|Pi| before the collision)
 *
 * Then, SMAGORINSKY:
 *
 *     a   = (25.455844f * n) * (Cs * Cs)             (18 sqrt 2)
 *     tau = 0.5f * (tau0 + sqrtf((tau0 * tau0) + ((a * pim) / rho)))
 *
 * OMEGA:
 *
 *     nu1 = ((1.f / w1) - 0.5f) / 3.f
 *     tau = (3.f * (nu0 + (n * (nu1 - nu0)))) + 0.5f
 *
 * and in both modes
 *
 *     w_eff  = 1.f / tau
 *     d      = (w0 - w_eff) / omo
 *     nu_add = (tau - tau0) / 3.f
 *     idle   = obstacle cell  ||  Cs == 0.f (OMEGA: w1 == w0)  ||  d == 0.f
 *     c_k    = c_k + (d * q_k)        for all nine populations, unless idle
 *
 * An idle cell keeps the bits of all nine populations (the loaded value is
 * selected, no zero is added) and its nu_add counts as 0.f.  D3Q19 (speed order
 * of lbm3d_hip.h; rho = s0 + s1 + ... + s18 sequential; ux, uy, uz as
 * lbm3d_store_fields gives them):
 *
 *     usq = ((ux * ux) + (uy * uy)) + (uz * uz)
 *     l0 = rho / 3.f;   l1 = rho / 18.f;   l2 = rho / 36.f
 *     pairs (P on the first, M on the second speed): l1: (1, 2) ux, (3, 4) uy,
 *     (9, 14) uz;  l2: (5, 6) ux + uy, (7, 8) ux - uy, (10, 15) ux + uz,
 *     (11, 16) (-ux) + uz, (12, 17) uy + uz, (13, 18) (-uy) + uz
 *     pxx = q1 + q2 + q5 + q6 + q7 + q8 + q10 + q11 + q15 + q16     (sequential)
 *     pyy = q3 + q4 + q5 + q6 + q7 + q8 + q12 + q13 + q17 + q18
 *     pzz = q9 + q10 + ... + q18
 *     pxy = (q5 + q6) - (q7 + q8);  pxz = (q10 + q15) - (q11 + q16)
 *     pyz = (q12 + q17) - (q13 + q18)
 *     p2  = (((pxx * pxx) + (pyy * pyy)) + (pzz * pzz))
 *           + ((((pxy * pxy) + (pxz * pxz)) + (pyz * pyz)) * 2.f)
 *
 * and the rest as above, on nineteen populations.  In exact arithmetic an
 * application changes neither the mass nor the momentum of a cell (q has
 * none).  There is NO positivity guard.
 *
 * stats (NULL allowed), double[3]: the number of cells that were not idle, the
 * fp64 sum of their fp32 nu_add and the largest of 0.f and their nu_add
 * (fmaxf).  Folded in a fixed order without atomics: two handles in the same
 * state return identical bits.
 *
 * store_nut writes float[ny][nx] (float[nz][ny][nx]): nu_add of every cell as
 * an application with n = 1 would form it (0.f where the cell would be idle),
 * the eddy viscosity of the current lattice.  The lattice is not touched.  It
 * is meant for a lattice that comes from a step: once an application has
 * rescaled the non-equilibrium part, c - feq is (1 - w_eff) (f - feq) and the
 * result is low by the factor (1 - w_eff) / (1 - w0).
 *
 * Contract.  NULL handle: LBM_E_INVALID.  apply and store_nut before the
 * lattice is loaded: LBM_E_STATE.  LBM_E_INVALID with a message, the model set
 * before unchanged: a mode other than LBM_SGS_*; a coefficient (array or
 * constant) that is not finite, a negative Cs, a w1 outside (0, 2); steps not
 * finite or < 0; 1.f - w0 == 0.f (nothing to rescale: apply and store_nut);
 * in the OMEGA mode a w_eff outside (0, 2) for some cell's w1 (apply).  coef
 * non-NULL: konst is not read.  mode LBM_SGS_OFF frees the model.  steps == 0,
 * or no model set: LBM_OK, no launch, every bit stays (stats and nut zeros).
 * The restrictions are those of lbm_scalar_begin (one device, the whole domain
 * on the handle, at most 16 local parts, no RCCL world > 1); set checks them.
 * apply follows a synchronisation of the handle's streams, launches once per
 * sub-domain (slab) on the compute stream of the first, on the CURRENT side of
 * the flow pair, blocks, and leaves the ghost cells to the engine exactly as
 * lbm_forcing_apply does: a run afterwards continues as from load_cells of the
 * filtered cells.  A handle that never sets a model allocates and launches
 * nothing.  On an LBM_FLAG_PROFILE handle (D2Q9) the launches are accounted
 * under the class "sgs".  lbm_destroy / lbm3d_destroy free the model.
 *
 * Not built: the rate inside the step kernels; dynamic or WALE models; several
 * devices or ranks; regularised or MRT collisions; time means of nu_add.
 */
#ifndef LBM_SGS_HIP_H
#define LBM_SGS_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_SGS_OFF 0
#define LBM_SGS_SMAGORINSKY 1
#define LBM_SGS_OMEGA 2

/* coef NULL: the constant konst; else float[ny][nx] over the domain */
int lbm_sgs_set(lbm_handle *h, int32_t mode, float konst, const float *coef);
int lbm_sgs_apply(lbm_handle *h, float steps, double stats[3]);
int lbm_sgs_store_nut(lbm_handle *h, float *nut);

/* coef: float[nz][ny][nx] */
int lbm3d_sgs_set(lbm3d_handle *h, int32_t mode, float konst, const float *coef);
int lbm3d_sgs_apply(lbm3d_handle *h, float steps, double stats[3]);
int lbm3d_sgs_store_nut(lbm3d_handle *h, float *nut);

/* Host-only restatements (no GPU, no handle), compiled from the same per-cell
 * function as the kernels: one application in place on the AoS cells
 * float[ny][nx][9] (float[nz][ny][nx][19]) of a whole domain with its obstacle
 * map and the omega w0 the cells were collided with.  nut (NULL allowed): the
 * fp32 nu_add of every cell, 0.f where it is idle.  A NULL array, an extent
 * < 1, w0 outside (0, 2) or equal to 1, and what lbm_sgs_set / lbm_sgs_apply
 * refuse: LBM_E_INVALID, nothing written.  steps == 0: LBM_OK, nothing written
 * (nut zeroed). */
int lbm_sgs_filter_ref(int32_t nx, int32_t ny, const uint8_t *obst, float *cells, float omega, int32_t mode,
                       float konst, const float *coef, float steps, float *nut);
int lbm3d_sgs_filter_ref(int32_t nx, int32_t ny, int32_t nz, const uint8_t *obst, float *cells, float omega,
                         int32_t mode, float konst, const float *coef, float steps, float *nut);

#ifdef __cplusplus
}
#endif

#endif /* LBM_SGS_HIP_H */
