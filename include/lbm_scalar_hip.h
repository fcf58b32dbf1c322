/*
 * lbm_scalar_hip.h -- a passive scalar carried with the flow (advection and
 * diffusion of a temperature, a dye, a concentration): a second, small
 * lattice kept on the device beside the flow lattice.  An additive part of
 * the C ABI of liblbm_hip.so (LBM_ABI_VERSION unchanged) for both engines:
 * D2Q9 (lbm_hip.h) carries a D2Q5 scalar, D3Q19 (lbm3d_hip.h) a D3Q7 one.
 *
 * The tracers of lbm_tracers_hip.h follow points through the flow; this is
 * the Eulerian half: a field phi that the current lattice's velocity
 * transports and that diffuses with D = (1 / omega_s - 1/2) / 3 (2-D) or
 * (1 / omega_s - 1/2) / 4 (3-D).  One memory-bound kernel per engine advances
 * it over the FROZEN flow lattice; it reads the flow populations, never
 * writes them.  No step kernel, lattice layout or other entry point changes.
 *
 * Definition.  IEEE fp32, every operation rounded separately, as written, no
 * contraction.
 *
 * 2-D, D2Q5.  Speeds 0 rest, 1 E (+x), 2 N (+y), 3 W, 4 S (the first five of
 * the D2Q9 order); opp = (0, 3, 4, 1, 2).  0 < omega_s < 2.  One step of the
 * populations g[5][ny][nx], periodic in x and y (indices taken modulo the
 * extents):
 *
 *     p0 = g0[y][x]  p1 = g1[y][x-1]  p2 = g2[y-1][x]  p3 = g3[y][x+1]  p4 = g4[y+1][x]
 *     obstacle cell:  out_k = p_opp(k)                 (zero-flux wall: conserves the sum of g)
 *     fluid cell:     phi = (((p0 + p1) + p2) + p3) + p4
 *                     e0 = phi * (1.f/3.f);  t = phi * (1.f/6.f)
 *                     a = t * (3.f * ux);    b = t * (3.f * uy)
 *                     e1 = t + a;  e3 = t - a;  e2 = t + b;  e4 = t - b
 *                     out_k = p_k + omega_s * (e_k - p_k)
 *
 * ux, uy are exactly what lbm_store_fields gives for the cell (0 at an
 * obstacle, where they are not used).  No ghost cell of the flow lattice is
 * read.  The scalar of a cell is phi = (((g0 + g1) + g2) + g3) + g4 of its own
 * stored populations, obstacle cells included.  begin sets g0 = phi0 * (1.f/3.f)
 * and g1..4 = phi0 * (1.f/6.f).
 *
 * Fixed cells: an optional list of distinct (x, y, value).  The listed cells
 * are overwritten with the begin state of `value`, once when the list is set
 * and again after every step (a dye inlet, a heated body).  Any cell may be
 * listed, obstacles included.
 *
 * 3-D, D3Q7.  Speeds 0 rest, 1 +x, 2 -x, 3 +y, 4 -y, 5 +z, 6 -z;
 * opp = (0, 2, 1, 4, 3, 6, 5); p1 = g1[z][y][x-1], p2 = g2[z][y][x+1],
 * p3 = g3[z][y-1][x], p4 = g4[z][y+1][x], p5 = g5[z-1][y][x], p6 = g6[z+1][y][x];
 * phi summed sequentially over speeds 0 to 6; e0 = phi * 0.25f, t = phi * 0.125f,
 * a_c = t * (4.f * u_c), e(+c) = t + a_c, e(-c) = t - a_c; velocities those of
 * lbm3d_store_fields.  begin sets g0 = phi0 * 0.25f, g1..6 = phi0 * 0.125f.
 * Everything else as in 2-D.
 *
 * Every cell has one owner lane and the scalar lattice is global (not split
 * with the flow lattice), so the result does not depend on the decomposition,
 * and the host restatement lbm_scalar_step_ref -- the same per-cell function,
 * compiled for the host -- reproduces it bit for bit.
 *
 * Device memory: two population sets, planar, rows padded to 4 floats:
 * 40 B per cell (2-D), 56 B (3-D), on the device of the handle's sub-domains.
 *
 * Contract.  LBM_E_INVALID for a NULL handle.  Every call but begin and end
 * before begin: LBM_E_STATE; advance before load_cells / init_equilibrium:
 * LBM_E_STATE.  Every call follows a synchronisation of the handle's streams,
 * runs on the compute stream of the first sub-domain, blocks, and touches
 * neither flow lattice, so a run afterwards continues bit-identically.  A
 * handle that never calls begin allocates and launches nothing.  On an
 * LBM_FLAG_PROFILE handle (D2Q9) the launches are accounted under the classes
 * "scalar_step", "scalar_fixed" and "scalar_stats".
 *
 * Not built: scalars on handles whose local sub-domains or slabs lie on more
 * than one device, on RCCL handles of world size > 1, on more than
 * LBM_SCALAR_MAX_PARTS local sub-domains, or on a handle that does not hold
 * the whole domain (begin: LBM_E_INVALID with a message); several scalar
 * steps per launch; caching the velocity across the sub-steps of a frozen
 * lattice; per-cell time accumulators of the scalar (time means at bin
 * resolution, one-cell bins included, are sums of lbm_transport_hip.h's
 * samples).
 *
 * Walls that hold a value or a flux, and the scalar every body hands to the
 * fluid, are lbm_scalar_walls_hip.h: a pass over the wall cells inside advance,
 * after the step and before the fixed list.
 *
 * How much scalar the flow carries -- face fluxes, u phi, Nusselt profiles --
 * is lbm_transport_hip.h: binned sums of the scalar's transport terms.
 *
 * Feedback on the flow: lbm_thermal_hip.h (included below) adds the Boussinesq
 * buoyancy calls lbm_scalar_buoyancy / lbm3d_scalar_buoyancy, the one place
 * where a scalar call writes the flow lattice.
 */
#ifndef LBM_SCALAR_HIP_H
#define LBM_SCALAR_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* most local sub-domains / slabs of a handle that carries a scalar */
enum { LBM_SCALAR_MAX_PARTS = 16 };

/* Allocates the scalar lattice and sets it to the begin state of phi0
 * (float[ny][nx]; NULL: zeros); the fixed list is empty and the step count 0.
 * A second call replaces the state.  omega_s not finite or outside (0, 2):
 * LBM_E_INVALID, and the previous state (if any) is kept. */
int lbm_scalar_begin(lbm_handle *h, float omega_s, const float *phi0);

/* Replaces the fixed list by n distinct cells and applies it once.  n = 0
 * clears the list (the arrays may be NULL).  n < 0, a NULL array with n > 0,
 * a cell outside the domain or listed twice: LBM_E_INVALID, and the old list
 * stays. */
int lbm_scalar_set_fixed(lbm_handle *h, int64_t n, const int32_t *x, const int32_t *y, const float *value);

/* `steps` scalar steps over the current, frozen lattice (one step launch per
 * local sub-domain and step, then the fixed list).  steps < 0: LBM_E_INVALID;
 * steps = 0: LBM_OK, no launch. */
int lbm_scalar_advance(lbm_handle *h, int32_t steps);

/* The steps advanced since begin. */
int lbm_scalar_steps(lbm_handle *h, int64_t *n);

/* phi (float[ny][nx]) and the populations (planar float[5][ny][nx]); either
 * may be NULL. */
int lbm_scalar_store(lbm_handle *h, float *phi, float *g);

/* total: the fp64 sum of every cell's fp32 phi, folded in a fixed order (two
 * calls give identical bits); min, max: over the fluid cells (+Inf, -Inf when
 * there is none).  NULL entries are skipped; all NULL launches nothing.
 * Non-finite scalars: the extremes are folded with fmaxf, which drops a NaN
 * operand, so a NaN phi of a fluid cell is left out of min and max (all fluid
 * cells NaN: +Inf, -Inf, as with none) while +-Inf take part as values; the
 * sum is plain IEEE addition, so total is NaN as soon as any cell, fluid or
 * blocked, holds a NaN phi or cells hold infinities of both signs. */
int lbm_scalar_stats(lbm_handle *h, double *total, float *min, float *max);

/* Frees the state (lbm_destroy frees it too).  LBM_OK on a handle without one. */
int lbm_scalar_end(lbm_handle *h);

/* D3Q19 twins: phi0 and phi float[nz][ny][nx], g planar float[7][nz][ny][nx]. */
int lbm3d_scalar_begin(lbm3d_handle *h, float omega_s, const float *phi0);
int lbm3d_scalar_set_fixed(lbm3d_handle *h, int64_t n, const int32_t *x, const int32_t *y, const int32_t *z,
                           const float *value);
int lbm3d_scalar_advance(lbm3d_handle *h, int32_t steps);
int lbm3d_scalar_steps(lbm3d_handle *h, int64_t *n);
int lbm3d_scalar_store(lbm3d_handle *h, float *phi, float *g);
int lbm3d_scalar_stats(lbm3d_handle *h, double *total, float *min, float *max);
int lbm3d_scalar_end(lbm3d_handle *h);

/* Host-only restatements (no GPU, no handle): one step of the definition
 * above from g_in to g_out (planar, unpadded; they must not overlap) over the
 * planar velocity fields lbm_store_fields writes and the obstacle map
 * uint8[ny][nx] (uint8[nz][ny][nx]), compiled from the same per-cell function
 * as the kernels.  A NULL array, an extent < 1 or a bad omega_s:
 * LBM_E_INVALID, nothing written. */
int lbm_scalar_step_ref(int32_t nx, int32_t ny, float omega_s, const float *ux, const float *uy,
                        const uint8_t *obst, const float *g_in, float *g_out);
int lbm3d_scalar_step_ref(int32_t nx, int32_t ny, int32_t nz, float omega_s, const float *ux, const float *uy,
                          const float *uz, const uint8_t *obst, const float *g_in, float *g_out);

#ifdef __cplusplus
}
#endif

#include "lbm_thermal_hip.h"

#endif /* LBM_SCALAR_HIP_H */
