/*
 * lbm_forcing_hip.h -- forcing zones: a body force, a linear drag and a
 * velocity target on boxes of cells.  An additive part of the C ABI of
 * liblbm_hip.so (LBM_ABI_VERSION unchanged) for both engines.  It needs no
 * scalar and changes no other entry point.
 *
 * The mechanism is that of lbm_thermal_hip.h: an impulse on the stored
 * populations between runs.  No step kernel changes, and a run afterwards
 * continues from the kicked lattice exactly as if it had been loaded with
 * load_cells.  What the buoyancy does with "force = s (phi - phi_ref) on every
 * cell", a zone does with per-cell coefficients on a box:
 *
 *     lam            (>= 0) the share of the gap to the target velocity closed
 *                    per flow step (a drag towards ut; ut = 0: a porous insert
 *                    or sponge; lam >= 1 / steps: the cell's momentum is SET
 *                    to rho ut -- a fringe, a fan, a penalised body);
 *     utx, uty[, utz]  the target velocity;
 *     fx, fy[, fz]   an acceleration per flow step (the force is rho f, on the
 *                    LOCAL density).
 *
 * Zones.  A handle holds up to LBM_FORCING_MAX_ZONES zones, indexed from 0.  A
 * zone is a box wholly inside the domain (no wrap): x0, y0, w, h (D2Q9) or
 * x0, y0, z0, w, h, d (D3Q19).  Each coefficient is one constant for the zone
 * or a dense array float[h][w] (float[d][h][w]) over the box.  Zones may
 * overlap; they are applied in ascending index order and a later zone sees
 * what an earlier one wrote.
 *
 * Definition of one application.  IEEE fp32, every operation rounded
 * separately, as written, no contraction.  n (finite, > 0) is the number of
 * flow steps the impulse stands for.  Per cell of a zone, D2Q9 (speeds 0 rest,
 * 1 E, 2 N, 3 W, 4 S, 5 NE, 6 NW, 7 SW, 8 SE; c_k the stored populations):
 *
 *     l    = fminf(n * lam, 1.f);    gx = n * fx;    gy = n * fy
 *     idle = obstacle cell  ||  (l == 0.f && gx == 0.f && gy == 0.f)
 *     rho  = c0 + c1 + ... + c8                      (sequential)
 *     jx   = ((c1 + c5) + c8) - ((c3 + c6) + c7)
 *     jy   = ((c2 + c5) + c6) - ((c4 + c7) + c8)
 *     mx   = (l * ((rho * utx) - jx)) + (rho * gx)
 *     my   = (l * ((rho * uty) - jy)) + (rho * gy)
 *
 * and the eight moving populations get the increments of lbm_thermal_hip.h
 * with (jx, jy) there replaced by (mx, my):
 *
 *     ax = mx * (1.f/3.f);      ay = my * (1.f/3.f)
 *     f1 += ax;  f3 -= ax;      f2 += ay;  f4 -= ay
 *     bx = mx * (1.f/12.f);     by = my * (1.f/12.f);   p = bx + by;  q = by - bx
 *     f5 += p;   f7 -= p;       f6 += q;   f8 -= q
 *
 * f0 is not touched.  An idle cell keeps the bits of all nine populations (the
 * loaded value is selected, no zero is added).
 *
 * D3Q19 (speed order of lbm3d_hip.h): rho = s0 + s1 + ... + s18 (sequential),
 *
 *     jx = ((((s1 + s5) + s7) + s10) + s16) - ((((s2 + s6) + s8) + s11) + s15)
 *     jy = ((((s3 + s5) + s8) + s12) + s18) - ((((s4 + s6) + s7) + s13) + s17)
 *     jz = ((((s9 + s10) + s11) + s12) + s13) - ((((s14 + s15) + s16) + s17) + s18)
 *
 * a third component m_z formed like the other two, and the nine pair
 * increments of lbm_thermal_hip.h (a_c = m_c * (1.f/6.f), b_c = m_c * (1.f/12.f)).
 *
 * No division anywhere.  With l = 1 the cell's momentum becomes rho ut (to
 * rounding); with lam = 0 the zone is a pure body force on the local density.
 * In exact arithmetic a zone adds no mass.  There is NO positivity guard, as
 * for the buoyancy: an over-strong force drives populations negative.
 *
 * Impulse.  Optionally an application returns, per zone, the sum over the
 * zone's non-idle cells of (double)mx, (double)my[, (double)mz]: the momentum
 * the zone added, which is minus the drag on a porous body or actuator.  The
 * terms are the fp32 values above; they are folded in fp64 in a fixed order
 * without atomics, so two handles in the same state return identical bits.
 *
 * Contract.  NULL handle: LBM_E_INVALID.  apply before the lattice is loaded:
 * LBM_E_STATE.  LBM_E_INVALID with a message, the zones set before unchanged:
 * a zone index outside 0 .. LBM_FORCING_MAX_ZONES - 1; a box that leaves the
 * domain or a negative extent; a non-finite coefficient (array or constant);
 * a negative lam; steps not finite or < 0.  w == 0 or h == 0 (or d == 0)
 * removes the zone.  steps == 0 or no zone set: LBM_OK, no launch, every bit
 * stays.  The restrictions are those of lbm_scalar_begin (one device, the
 * whole domain on the handle, at most 16 local parts, no RCCL world > 1); they
 * are checked by set_zone.  apply follows a synchronisation of the handle's
 * streams, launches once per zone and intersecting sub-domain (slab) on the
 * compute stream of the first, on the CURRENT side of the flow pair, blocks,
 * and leaves the ghost cells to the engine exactly as the buoyancy does.  A
 * handle that never sets a zone allocates and launches nothing.  On an
 * LBM_FLAG_PROFILE handle (D2Q9) the launches are accounted under the class
 * "forcing".  lbm_destroy / lbm3d_destroy free the zones.
 *
 * Not built: second-order (Guo) forcing; zones on several devices or ranks;
 * coefficients that change without a new set_zone; the kick fused into a step
 * kernel; moving solid walls.
 */
#ifndef LBM_FORCING_HIP_H
#define LBM_FORCING_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LBM_FORCING_MAX_ZONES 8

/* Coefficient order: lam, utx, uty, fx, fy.  coef[i] NULL: the constant
 * konst[i]; else float[h][w] over the box (konst[i] is then not read).  coef
 * itself NULL: all constants.  w == 0 or h == 0: removes the zone. */
int lbm_forcing_set_zone(lbm_handle *h, int32_t zone, int32_t x0, int32_t y0, int32_t w, int32_t ht,
                         const float *const coef[5], const float konst[5]);
int lbm_forcing_clear(lbm_handle *h);
/* the number of zones set and a bit mask of their indices; either may be NULL */
int lbm_forcing_zones(lbm_handle *h, int32_t *n_set, uint32_t *mask);
/* impulse: double[LBM_FORCING_MAX_ZONES][2], rows of unset zones 0; NULL allowed */
int lbm_forcing_apply(lbm_handle *h, float steps, double *impulse);

/* Coefficient order: lam, utx, uty, utz, fx, fy, fz; arrays float[d][h][w]. */
int lbm3d_forcing_set_zone(lbm3d_handle *h, int32_t zone, int32_t x0, int32_t y0, int32_t z0, int32_t w, int32_t ht,
                           int32_t d, const float *const coef[7], const float konst[7]);
int lbm3d_forcing_clear(lbm3d_handle *h);
int lbm3d_forcing_zones(lbm3d_handle *h, int32_t *n_set, uint32_t *mask);
/* impulse: double[LBM_FORCING_MAX_ZONES][3] */
int lbm3d_forcing_apply(lbm3d_handle *h, float steps, double *impulse);

/* Host-only restatements (no GPU, no handle), compiled from the same per-cell
 * function as the kernels: ONE zone applied in place to the AoS cells
 * float[ny][nx][9] (float[nz][ny][nx][19]) of a whole domain with its obstacle
 * map.  terms (NULL allowed): float[h][w][2] (float[d][h][w][3]), the fp32
 * (mx, my[, mz]) of every cell of the box, zeros where the cell is idle.  A
 * NULL array, an extent < 1, a box that leaves the domain or is empty, a
 * non-finite number, a negative lam or steps < 0: LBM_E_INVALID, nothing
 * written.  steps == 0: LBM_OK, nothing written (terms zeroed). */
int lbm_forcing_kick_ref(int32_t nx, int32_t ny, const uint8_t *obst, float *cells, int32_t x0, int32_t y0, int32_t w,
                         int32_t ht, const float *const coef[5], const float konst[5], float steps, float *terms);
int lbm3d_forcing_kick_ref(int32_t nx, int32_t ny, int32_t nz, const uint8_t *obst, float *cells, int32_t x0,
                           int32_t y0, int32_t z0, int32_t w, int32_t ht, int32_t d, const float *const coef[7],
                           const float konst[7], float steps, float *terms);

#ifdef __cplusplus
}
#endif

#endif /* LBM_FORCING_HIP_H */
