/*
 * lbm_tracers_hip.h -- Lagrangian tracers and point probes: a set of points
 * kept on the device, at which the current lattice is interpolated.  An
 * additive part of the C ABI of liblbm_hip.so (LBM_ABI_VERSION unchanged) for
 * both engines: D2Q9 (lbm_hip.h) and D3Q19 (lbm3d_hip.h).
 *
 * Pathlines, streaklines and residence times follow fluid parcels through the
 * flow; a time series of the velocity at a handful of points gives a shedding
 * frequency.  Both are one capability -- a probe is a point that is never
 * advanced -- and neither needs a field on the host: lbm_tracer_begin copies
 * the points to the device, lbm_tracer_advance moves them with the velocity
 * interpolated from the current lattice in one gather kernel of O(points)
 * work, lbm_tracer_sample interpolates velocity and pressure at them.  No step
 * kernel changes.
 *
 * Definition.
 *
 * Coordinates are in cell units, fp64.  The centre of cell (i, j[, k]) is the
 * point (i, j[, k]).  The domain is periodic: 0 <= x < nx, 0 <= y < ny
 * (0 <= z < nz).  (fp32 at x ~ 8192 has an ulp of 2^-11, the order of one
 * step's displacement in slow regions: hence fp64.)
 *
 * The values at a cell are exactly what lbm_store_fields / lbm3d_store_fields
 * give for it: ux, uy (uz) and pressure, in IEEE fp32 and the evaluation order
 * those headers state, with their obstacle-cell convention 0, 0, (0,)
 * density * (1.f / 3.f), widened to double.  No ghost cell is ever read: the
 * periodic neighbour of a border cell is taken from the interior of the
 * sub-domain or slab that owns it.
 *
 * Interpolation, every operation in fp64, as written, without contraction:
 *
 *     i0 = (int)floor(x)          tx = x - (double)i0
 *     i1 = (i0 + 1 == nx) ? 0 : i0 + 1            likewise j0, j1, ty (k0, k1, tz)
 *     lerp(a, b, t) = a + t * (b - a)
 *     v  = lerp(lerp(v[j0][i0], v[j0][i1], tx), lerp(v[j1][i0], v[j1][i1], tx), ty)
 *
 * and in 3-D along x first, then y, then z:
 *
 *     v = lerp(lerp(lerp(v000, v100, tx), lerp(v010, v110, tx), ty),
 *              lerp(lerp(v001, v101, tx), lerp(v011, v111, tx), ty), tz)
 *
 * (vXYZ: X, Y, Z select i0/i1, j0/j1, k0/k1).  At a cell centre this is the
 * cell's own value, exactly.
 *
 *     wrap(v, n):  r = v - n * floor(v / n);  if (!(r >= 0.0 && r < n)) r = 0.0;
 *
 * with n as double.  The last clause also catches NaN and +-Inf, so a stored
 * position is always a valid index, whatever the lattice holds; the kernels
 * rely on this invariant alone for their index safety.
 *
 * Advance by dt (a double: the lattice steps run since the last advance; the
 * field is frozen at the current lattice), per coordinate c with extent n_c:
 *
 *     LBM_TRACER_EULER:  c' = wrap(c + dt * u_c(p), n_c)
 *     LBM_TRACER_HEUN:   k1 = u(p);  p*_c = wrap(c + dt * k1_c, n_c);  k2 = u(p*)
 *                        c' = wrap(c + (0.5 * dt) * (k1_c + k2_c), n_c)
 *
 * The blocked flag of a point is 1 when its nearest cell is an obstacle, else
 * 0; the nearest cell is (int)floor(x + 0.5), taken to 0 when it equals nx,
 * likewise for y (and z).
 *
 * Every point has one owner lane and no value is reduced across points: the
 * result does not depend on the decomposition, and a host restatement of the
 * definition reproduces it bit for bit (lbm_tracer_advance_ref /
 * lbm_tracer_sample_ref below compile the same per-point functions for the
 * host).
 *
 * Contract.  LBM_E_INVALID for a NULL handle.  advance, sample or store
 * before begin: LBM_E_STATE; advance or sample before load_cells /
 * init_equilibrium: LBM_E_STATE.  Every call follows a synchronisation of the
 * handle's streams, runs on the compute stream, blocks, and touches neither
 * lattice of the pair, so a run afterwards continues bit-identically.  A
 * handle that never calls begin allocates and launches nothing.  On an
 * LBM_FLAG_PROFILE handle (D2Q9) the advance launch is accounted under the
 * class "advance_tracers", the sample launch under "sample_tracers".
 *
 * Not built: point sets on handles whose local sub-domains or slabs lie on
 * more than one device, on RCCL handles of world size > 1, or on more than
 * LBM_TRACER_MAX_PARTS local sub-domains (begin: LBM_E_INVALID with a
 * message); appending points to a live set; inertial particles; wall
 * reflection.
 */
#ifndef LBM_TRACERS_HIP_H
#define LBM_TRACERS_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* integration schemes of advance */
enum { LBM_TRACER_EULER = 0, LBM_TRACER_HEUN = 1 };

/* most local sub-domains / slabs of a handle that takes a point set */
enum { LBM_TRACER_MAX_PARTS = 16 };

/* Copies n >= 1 seeds to the device of the handle's sub-domains; a second
 * call replaces the set.  n < 1, a NULL array, or any seed that is not finite
 * or lies outside [0, nx) x [0, ny): LBM_E_INVALID, and the previous set (if
 * any) is kept.  Device memory: 16 B per point (24 B in 3-D). */
int lbm_tracer_begin(lbm_handle *h, int64_t n, const double *x, const double *y);

/* The number of points (0 when there is no set). */
int lbm_tracer_count(lbm_handle *h, int64_t *n);

/* Moves every point by dt steps of the current lattice's velocity (one
 * launch).  dt not finite, or an unknown scheme: LBM_E_INVALID. */
int lbm_tracer_advance(lbm_handle *h, double dt, int32_t scheme);

/* The interpolated ux, uy and pressure at the current positions, double[n]
 * each.  A NULL array is neither computed nor copied; all NULL returns LBM_OK
 * and launches nothing. */
int lbm_tracer_sample(lbm_handle *h, double *ux, double *uy, double *pressure);

/* The current positions (double[n] each) and blocked flags (uint8_t[n]).  A
 * NULL array is skipped. */
int lbm_tracer_store(lbm_handle *h, double *x, double *y, uint8_t *blocked);

/* Frees the set (lbm_destroy frees it too).  LBM_OK on a handle without one. */
int lbm_tracer_end(lbm_handle *h);

/* D3Q19 twins: seeds in [0, nx) x [0, ny) x [0, nz). */
int lbm3d_tracer_begin(lbm3d_handle *h, int64_t n, const double *x, const double *y, const double *z);
int lbm3d_tracer_count(lbm3d_handle *h, int64_t *n);
int lbm3d_tracer_advance(lbm3d_handle *h, double dt, int32_t scheme);
int lbm3d_tracer_sample(lbm3d_handle *h, double *ux, double *uy, double *uz, double *pressure);
int lbm3d_tracer_store(lbm3d_handle *h, double *x, double *y, double *z, uint8_t *blocked);
int lbm3d_tracer_end(lbm3d_handle *h);

/* Host-only restatements (no GPU, no handle): the definition above over
 * planar fp32 fields float[ny][nx] (float[nz][ny][nx]) -- the layout
 * lbm_store_fields writes -- compiled from the same per-point functions as the
 * kernels.  advance_ref moves x, y (z) in place; sample_ref writes out_*[n]
 * (a NULL output is skipped, and so may its field be).  Positions must satisfy
 * the invariant 0 <= c < n_c (LBM_E_INVALID otherwise, nothing written). */
int lbm_tracer_advance_ref(int32_t nx, int32_t ny, const float *ux, const float *uy, int64_t n, double *x, double *y,
                           double dt, int32_t scheme);
int lbm_tracer_sample_ref(int32_t nx, int32_t ny, const float *ux, const float *uy, const float *pressure, int64_t n,
                          const double *x, const double *y, double *out_ux, double *out_uy, double *out_p);
int lbm3d_tracer_advance_ref(int32_t nx, int32_t ny, int32_t nz, const float *ux, const float *uy, const float *uz,
                             int64_t n, double *x, double *y, double *z, double dt, int32_t scheme);
int lbm3d_tracer_sample_ref(int32_t nx, int32_t ny, int32_t nz, const float *ux, const float *uy, const float *uz,
                            const float *pressure, int64_t n, const double *x, const double *y, const double *z,
                            double *out_ux, double *out_uy, double *out_uz, double *out_p);

#ifdef __cplusplus
}
#endif

#endif /* LBM_TRACERS_HIP_H */
