/*
 * lbm_binned_hip.h -- sums of per-cell quantities of the current lattice over
 * the cells of rectangular bins, formed on the device: velocity profiles
 * (bins nx x 1), section fluxes (1 x ny), reduced-resolution fields (k x k) and
 * domain totals (nx x ny).  An additive part of the C ABI of liblbm_hip.so
 * (LBM_ABI_VERSION unchanged) for both engines: D2Q9 (lbm_hip.h) and D3Q19
 * (lbm3d_hip.h).  Only the bin arrays cross to the host.  No step kernel
 * changes.
 *
 * Bins.  Bins tile the full domain from cell (0, 0[, 0]) in global
 * coordinates: bin (bx, by) covers [bx*bw, min(nx, (bx+1)*bw)) x
 * [by*bh, min(ny, (by+1)*bh)), in 3-D also [bz*bd, min(nz, (bz+1)*bd)); the
 * last bin along an axis may be ragged.  Each output is planar
 * double[nby][nbx], in 3-D double[nbz][nby][nbx], with
 * nb? = LBM_BIN_COUNT(n?, b?).
 *
 * Definition.  For every fluid cell take ux, uy[, uz], speed exactly as
 * lbm_store_fields / lbm3d_store_fields give them (the same device
 * expressions); rho is that header's sequential fp32 density (D2Q9:
 * c0 + c1 + ... + c8; D3Q19: likewise over the 19 speeds) and jx, jy[, jz] are
 * the fp32 numerators those headers divide by rho, in D2Q9
 *
 *     jx = ((c1 + c5) + c8) - ((c3 + c6) + c7)
 *     jy = ((c2 + c5) + c6) - ((c4 + c7) + c8)
 *
 * and in D3Q19 the five-term sums of lbm3d_fields_hip.h.  A bin's entry is the
 * fp64 sum over its fluid cells of (double)q for q = rho, jx, jy[, jz], ux,
 * uy[, uz], speed, and of (double)a * (double)b for the products (each product
 * is exact in fp64).  Every sum starts from +0.0, so a sum of value zero is
 * +0.0 whatever the signs of its zero terms.  Obstacle cells contribute to
 * nothing; a bin with no fluid cell holds +0.0.  lbm_bin_fluid_cells gives the
 * fluid cells per bin; means are sum / count, and that division is the
 * caller's.  The operator is linear: sums of binned samples over time are the
 * binned sums of the time sums.
 *
 * Determinism and precision.  No floating-point atomics: every sum is folded
 * in an order fixed by the geometry of the grid, the bins and the
 * decomposition, so two calls on the same lattice return identical bits.  The
 * order itself is not part of the contract and differs between
 * decompositions.  A one-cell bin is therefore exact, and a bin of n fluid
 * cells lies within
 *
 *     2 (n - 1) 2^-53 sum|term|
 *
 * of the exactly rounded sum (any order of n fp64 additions, plus the rounding
 * of the exact sum itself).
 *
 * Contract.  The rules follow lbm_store_fields.  A NULL handle, or a bin size
 * outside 1..n along its axis: LBM_E_INVALID.  lbm_store_binned before
 * load_cells / init_equilibrium: LBM_E_STATE (the counts need no lattice).  A
 * NULL entry of `out` is neither staged nor copied; a call with every entry
 * NULL (or a NULL `count`) returns LBM_OK and does no work.  Every call waits
 * for the handle's streams, blocks, runs on the compute stream and touches
 * neither lattice nor its ping-pong side: a run afterwards continues
 * bit-identically.  LOCAL handles write full-domain bins; the partial sums of
 * a bin that spans several sub-domains or slabs are added on the host in
 * sub-domain order.  The kernel is cell-local, so RCCL handles of any world
 * size are accepted: they return this rank's partial sums and counts over the
 * full bin grid (bins the rank does not touch hold zeros) and the caller
 * all-reduces them.  The counts come from the obstacle map with no launch.
 *
 * Staging.  Per sub-domain (slab) and requested field the device holds, until
 * the call returns, 8 B x chunks x (waves + bins along x - 1) [x ny in 3-D] of
 * partial sums and 8 B per local bin, where a wave is 256 (3-D: 64) columns
 * and a chunk at most 32 rows (planes) of one bin: at most
 * 8 B x ceil(n_walked / min(b, 32) + bins) x (nx / 256 + nbx) per field in
 * 2-D, about 2.3 B per cell for the nine fields at bins 1 x ny and less for
 * every wider bin.
 *
 * On an LBM_FLAG_PROFILE handle (D2Q9) the launches are accounted under
 * "binned_sums" and "binned_sums fold".
 */
#ifndef LBM_BINNED_HIP_H
#define LBM_BINNED_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* field indices of the arrays of output pointers */
enum {
    LBM_BIN_RHO = 0,
    LBM_BIN_JX = 1,
    LBM_BIN_JY = 2,
    LBM_BIN_UX = 3,
    LBM_BIN_UY = 4,
    LBM_BIN_SPEED = 5,
    LBM_BIN_UXUX = 6,
    LBM_BIN_UXUY = 7,
    LBM_BIN_UYUY = 8,
    LBM_BIN_FIELDS = 9
};

enum {
    LBM3D_BIN_RHO = 0,
    LBM3D_BIN_JX = 1,
    LBM3D_BIN_JY = 2,
    LBM3D_BIN_JZ = 3,
    LBM3D_BIN_UX = 4,
    LBM3D_BIN_UY = 5,
    LBM3D_BIN_UZ = 6,
    LBM3D_BIN_SPEED = 7,
    LBM3D_BIN_UXUX = 8,
    LBM3D_BIN_UXUY = 9,
    LBM3D_BIN_UXUZ = 10,
    LBM3D_BIN_UYUY = 11,
    LBM3D_BIN_UYUZ = 12,
    LBM3D_BIN_UZUZ = 13,
    LBM3D_BIN_FIELDS = 14
};

/* bins along an axis of n cells cut into bins of b */
#define LBM_BIN_COUNT(n, b) (((n) + (b) - 1) / (b))

/* The binned sums of the current lattice: out[f] is double[nby][nbx] or NULL. */
int lbm_store_binned(lbm_handle *h, int32_t bw, int32_t bh, double *const out[LBM_BIN_FIELDS]);

/* Fluid cells per bin of this handle's sub-domains: int64[nby][nbx]. */
int lbm_bin_fluid_cells(lbm_handle *h, int32_t bw, int32_t bh, int64_t *count);

/* D3Q19: out[f] is double[nbz][nby][nbx] or NULL. */
int lbm3d_store_binned(lbm3d_handle *h, int32_t bw, int32_t bh, int32_t bd, double *const out[LBM3D_BIN_FIELDS]);

/* Fluid cells per bin of this handle's slabs: int64[nbz][nby][nbx]. */
int lbm3d_bin_fluid_cells(lbm3d_handle *h, int32_t bw, int32_t bh, int32_t bd, int64_t *count);

#ifdef __cplusplus
}
#endif

#endif /* LBM_BINNED_HIP_H */
