/*
 * lbm_averages_hip.h -- time-averaged flow fields and Reynolds stresses,
 * accumulated on the device next to the lattice.  An additive part of the C
 * ABI of liblbm_hip.so (LBM_ABI_VERSION unchanged) for both engines: D2Q9
 * (lbm_hip.h) and D3Q19 (lbm3d_hip.h).
 *
 * An unsteady flow is described by its mean and its fluctuation: the
 * time-averaged velocity and pressure, the Reynolds stresses <u_a' u_b'> and
 * the pressure variance.  lbm_avg_begin allocates one fp64 sum per selected
 * field and cell beside the lattice; lbm_avg_sample adds the current lattice
 * to the sums in one memory-bound kernel; nothing crosses to the host until
 * lbm_avg_store / lbm_avg_store_sums.  No step kernel changes.
 *
 * Definition.  A sample of a cell is exactly the value lbm_store_fields /
 * lbm3d_store_fields gives for that cell: ux, uy (and uz) and pressure, in
 * IEEE fp32 and the evaluation order those headers state, with their
 * obstacle-cell convention 0, 0, (0,) density * (1.f / 3.f), whatever kernel
 * or numerics mode advanced the lattice.  Per cell and sample, in fp64, as
 * written and without contraction:
 *
 *     S_a  += (double)a                  a in {ux, uy, (uz,) p}
 *     S_ab += (double)a * (double)b      the velocity pairs listed below, and p * p
 *
 * With n the sample count, lbm_avg_store writes
 *
 *     mean_a = (float)(S_a / (double)n)
 *     c_ab   = (float)(S_ab / (double)n - (S_a / (double)n) * (S_b / (double)n))
 *
 * every operation in fp64 in that order, one rounding to fp32 at the end.
 * The order of samples in time is the only order there is: no reduction
 * across cells, no atomics.  Two identical sequences give identical bits, and
 * a host restatement of the definition reproduces them exactly.
 *
 * Contract.  LBM_E_INVALID for a NULL handle.  sample, store and store_sums
 * before begin: LBM_E_STATE; sample before load_cells / init_equilibrium:
 * LBM_E_STATE; store with zero samples: LBM_E_STATE (store_sums with zero
 * samples writes zeros).  A non-NULL second-moment entry on a handle begun
 * with LBM_AVG_MEAN only: LBM_E_INVALID, and nothing is written.  store or
 * store_sums with every entry NULL returns LBM_OK and does no work.  Every
 * call blocks; it runs on the compute stream and touches neither lattice nor
 * its ping-pong side, so a run afterwards continues bit-identically.  A handle
 * that never calls begin allocates and launches nothing.  On an
 * LBM_FLAG_PROFILE handle (D2Q9) the sample launch is accounted under the
 * class "accumulate_moments", the derive launch under "moment_means".
 */
#ifndef LBM_AVERAGES_HIP_H
#define LBM_AVERAGES_HIP_H

#include <stdint.h>

#include "lbm3d_hip.h"
#include "lbm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* field indices of the arrays of output pointers */
enum {
    LBM_AVG_UX = 0,
    LBM_AVG_UY = 1,
    LBM_AVG_P = 2,
    LBM_AVG_UXUX = 3,
    LBM_AVG_UXUY = 4,
    LBM_AVG_UYUY = 5,
    LBM_AVG_PP = 6,
    LBM_AVG_FIELDS = 7
};

enum {
    LBM3D_AVG_UX = 0,
    LBM3D_AVG_UY = 1,
    LBM3D_AVG_UZ = 2,
    LBM3D_AVG_P = 3,
    LBM3D_AVG_UXUX = 4,
    LBM3D_AVG_UXUY = 5,
    LBM3D_AVG_UXUZ = 6,
    LBM3D_AVG_UYUY = 7,
    LBM3D_AVG_UYUZ = 8,
    LBM3D_AVG_UZUZ = 9,
    LBM3D_AVG_PP = 10,
    LBM3D_AVG_FIELDS = 11
};

/* moments flags of begin: LBM_AVG_MEAN selects the first moments (ux, uy,
 * (uz,) p), LBM_AVG_SECOND the products and is valid only together with
 * LBM_AVG_MEAN.  begin accepts 1 or 3. */
enum { LBM_AVG_MEAN = 1, LBM_AVG_SECOND = 2 };

/* Allocates one zeroed fp64 accumulator per selected field and cell, for every
 * local sub-domain, on that sub-domain's device.  Calling it again re-zeroes
 * the accumulators (and re-allocates them if `moments` changed).  moments
 * other than 1 or 3: LBM_E_INVALID.  Allocation failure: LBM_E_NOMEM; the
 * handle stays usable and is not averaging.
 *
 * Device memory: 8 B x fields x roundup(w, 4) x h per sub-domain (fields = 3 /
 * 7 for D2Q9, 4 / 11 for D3Q19).  With LBM_AVG_MEAN | LBM_AVG_SECOND that is
 * 3.8 GB at 8192^2 and 11.8 GB at 512^3. */
int lbm_avg_begin(lbm_handle *h, int32_t moments);

/* Adds the current lattice to the sums and increments the sample count. */
int lbm_avg_sample(lbm_handle *h);

/* The sample count (0 on a handle that is not averaging). */
int lbm_avg_samples(lbm_handle *h, int64_t *n);

/* The raw fp64 sums, planar double[ny][nx] per field, full domain.  A NULL
 * entry is skipped.  RCCL: this rank's rectangle only, as lbm_store_fields. */
int lbm_avg_store_sums(lbm_handle *h, double *const out[LBM_AVG_FIELDS]);

/* fp32 means (first moments) and central second moments, formed on the device
 * from the sums (definition above).  Layout rules of lbm_avg_store_sums, in
 * float. */
int lbm_avg_store(lbm_handle *h, float *const out[LBM_AVG_FIELDS]);

/* Frees the accumulators (lbm_destroy frees them too).  LBM_OK on a handle
 * that is not averaging. */
int lbm_avg_end(lbm_handle *h);

/* D3Q19 twins: planar [nz][ny][nx] arrays, LBM3D_AVG_FIELDS entries; RCCL:
 * this rank's planes only. */
int lbm3d_avg_begin(lbm3d_handle *h, int32_t moments);
int lbm3d_avg_sample(lbm3d_handle *h);
int lbm3d_avg_samples(lbm3d_handle *h, int64_t *n);
int lbm3d_avg_store_sums(lbm3d_handle *h, double *const out[LBM3D_AVG_FIELDS]);
int lbm3d_avg_store(lbm3d_handle *h, float *const out[LBM3D_AVG_FIELDS]);
int lbm3d_avg_end(lbm3d_handle *h);

#ifdef __cplusplus
}
#endif

#endif /* LBM_AVERAGES_HIP_H */
