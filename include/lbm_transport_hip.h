/*
 * lbm_transport_hip.h -- how much scalar the flow carries: sums of the passive
 * scalar's per-cell transport terms over rectangular bins, formed on the
 * device (heat-flux and Nusselt profiles, plane fluxes, scalar totals and
 * variances).  An additive part of the C ABI of liblbm_hip.so
 * (LBM_ABI_VERSION unchanged) for both engines: D2Q9 + D2Q5 and D3Q19 + D3Q7
 * (lbm_scalar_hip.h).  Only the bin arrays cross to the host.  No step kernel
 * and no other entry point changes.
 *
 * The flux through a face.  The scalar step streams g_k to the neighbour
 * along speed k, so the amount of scalar that crosses the face between cell x
 * and cell x + 1 in the next step is exactly g1[y][x] - g3[y][x+1]: advection
 * and diffusion together, zero-flux walls included; no model and no gradient
 * stencil.  With indices modulo the extents (periodic):
 *
 *     2-D   FX[y][x] = g1[y][x] - g3[y][x+1]      FY[y][x] = g2[y][x] - g4[y+1][x]
 *     3-D   FX = g1[x] - g2[x+1]    FY = g3[y] - g4[y+1]    FZ = g5[z] - g6[z+1]
 *
 * each one fp32 subtraction of stored populations, taken for EVERY cell,
 * obstacles included (obstacle cells hold scalar and reflect it).  A face
 * belongs to the cell on its low side.  For every cell that is not in the
 * fixed list the budget
 *
 *     phi_after_step(x, y) - phi(x, y) = FX[y][x-1] - FX[y][x] + FY[y-1][x] - FY[y][x]
 *
 * holds up to fp32 rounding, so in a steady state the sum of FY over a
 * horizontal plane is the same for every plane between a hot and a cold row.
 *
 * Terms per cell, each widened to fp64 before any product or sum:
 *
 *     PHI      (double)phi                       fluid cells
 *     PHIPHI   (double)phi * (double)phi         fluid cells
 *     U?PHI    (double)u_c * (double)phi         fluid cells
 *     F?       (double)F_c                       all cells
 *
 * phi is lbm_scalar_hip.h's sequential fp32 sum of the cell's own stored g;
 * u_c is exactly what lbm_store_fields / lbm3d_store_fields give (the same
 * device expressions).  Every product is exact in fp64.
 *
 * Bins, determinism, precision: as lbm_binned_hip.h states them.  Bins tile
 * the global domain from cell 0 and the last bin along an axis may be ragged;
 * out[f] is planar double[nby][nbx] (3-D: double[nbz][nby][nbx]) with
 * nb? = LBM_BIN_COUNT(n?, b?).  Sums start from +0.0, there are no atomics and
 * the fold order is fixed by the geometry: two calls return identical bits, a
 * one-cell bin is exact, and a bin of n contributing cells lies within
 * 2 (n - 1) 2^-53 sum|term| of the exactly rounded sum.  The fluid cells per
 * bin are lbm_bin_fluid_cells / lbm3d_bin_fluid_cells, unchanged.
 *
 * Time means.  The operator is linear in time: the time mean of any bin
 * array is the sum of its samples on the host divided by their number.  No
 * per-cell accumulator is added; time averages of the scalar exist at bin
 * resolution (one-cell bins included) through repeated calls.
 *
 * Contract.  The rules follow lbm_store_binned and lbm_scalar_hip.h.  A NULL
 * handle, or a bin size outside 1..n along its axis: LBM_E_INVALID.  Before
 * lbm_scalar_begin, or before load_cells / init_equilibrium: LBM_E_STATE.  A
 * NULL entry of `out` is neither computed, staged nor copied; a call with
 * every entry NULL returns LBM_OK and launches nothing.  With no U?PHI entry
 * requested the flow lattice is not read at all, and with no PHI / PHIPHI
 * entry either only the planes the requested faces need are read.  Every call
 * follows a synchronisation of the handle's streams, runs on the compute
 * stream of the first sub-domain (slab), blocks, and writes neither the flow
 * lattice nor the scalar lattice: a run or an advance afterwards continues
 * bit-identically.  A handle that never calls these allocates and launches
 * nothing new.  On an LBM_FLAG_PROFILE handle (D2Q9) the launches are
 * accounted under the classes "scalar_binned" and "scalar_binned fold".
 *
 * Not built: per-cell fp32 flux fields to the host (one-cell bins give them);
 * a diffusive-only flux (total less convective, at bin level); the wall heat
 * flux per body; fusing the sums into the scalar step.
 */
#ifndef LBM_TRANSPORT_HIP_H
#define LBM_TRANSPORT_HIP_H

#include <stdint.h>

#include "lbm_binned_hip.h"
#include "lbm_scalar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* field indices of the arrays of output pointers */
enum {
    LBM_SBIN_PHI = 0,
    LBM_SBIN_PHIPHI = 1,
    LBM_SBIN_UXPHI = 2,
    LBM_SBIN_UYPHI = 3,
    LBM_SBIN_FX = 4,
    LBM_SBIN_FY = 5,
    LBM_SBIN_FIELDS = 6
};

enum {
    LBM3D_SBIN_PHI = 0,
    LBM3D_SBIN_PHIPHI = 1,
    LBM3D_SBIN_UXPHI = 2,
    LBM3D_SBIN_UYPHI = 3,
    LBM3D_SBIN_UZPHI = 4,
    LBM3D_SBIN_FX = 5,
    LBM3D_SBIN_FY = 6,
    LBM3D_SBIN_FZ = 7,
    LBM3D_SBIN_FIELDS = 8
};

/* The binned transport sums of the current lattice and scalar: out[f] is double[nby][nbx] or NULL. */
int lbm_scalar_store_binned(lbm_handle *h, int32_t bw, int32_t bh, double *const out[LBM_SBIN_FIELDS]);

/* D3Q19 + D3Q7: out[f] is double[nbz][nby][nbx] or NULL. */
int lbm3d_scalar_store_binned(lbm3d_handle *h, int32_t bw, int32_t bh, int32_t bd,
                              double *const out[LBM3D_SBIN_FIELDS]);

/* Host-only restatements (no GPU, no handle): the per-cell terms, planar double[LBM_SBIN_FIELDS][ny][nx]
 * (double[LBM3D_SBIN_FIELDS][nz][ny][nx]), from the planar velocity fields lbm_store_fields writes, the
 * obstacle map and the planar unpadded populations g -- the kernels' per-cell function compiled for the
 * host.  A NULL array or an extent < 1: LBM_E_INVALID, nothing written. */
int lbm_scalar_terms_ref(int32_t nx, int32_t ny, const float *ux, const float *uy, const uint8_t *obst,
                         const float *g, double *terms);
int lbm3d_scalar_terms_ref(int32_t nx, int32_t ny, int32_t nz, const float *ux, const float *uy, const float *uz,
                           const uint8_t *obst, const float *g, double *terms);

#ifdef __cplusplus
}
#endif

#endif /* LBM_TRANSPORT_HIP_H */
