// lbm_gradients.hpp -- what the velocity-gradient kernels of both engines share
// (lbm_gradients.hip, lbm3d_gradients.hip; include/lbm_gradients_hip.h): the
// per-cell expressions of the definition and the argument blocks of the kernels.
//
// Arithmetic: IEEE fp32 in the order the header writes, no contraction
// (-ffp-contract=off), correctly rounded sqrt (hipcc default).  The inputs are
// the velocities cell_macro / cell3_macro give, so they are lbm_store_fields'
// own by construction.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lbm_views.hpp"

namespace lbm {
namespace grad {

// ---- D2Q9 ----

// a wave owns GR_OWN_Q lane quads (GR_STRIP columns) of a strip and GR_SEG rows
// of a segment; lanes 0 and 63 and one row each side only supply neighbours
constexpr int GR_OWN_Q = 62;
constexpr int GR_STRIP = 4 * GR_OWN_Q;  // 248 owned columns of the 256 a wave reads
constexpr int GR_SEG = 32;              // owned rows of the 34 a wave reads

struct Grad2 {
    float vorticity, divergence, strain, q, s2;
};

// e / w / n / s: the velocity at the east / west / north / south neighbour
__device__ __forceinline__ Grad2 gradients2(float ue, float uw, float un, float us, float ve, float vw, float vn,
                                            float vs) {
    const float gxx = (ue - uw) * 0.5f, gxy = (un - us) * 0.5f;
    const float gyx = (ve - vw) * 0.5f, gyy = (vn - vs) * 0.5f;
    Grad2 g;
    g.vorticity = gyx - gxy;
    g.divergence = gxx + gyy;
    const float sxy = (gxy + gyx) * 0.5f;
    g.s2 = ((gxx * gxx) + (gyy * gyy)) + ((sxy * sxy) * 2.f);
    g.strain = sqrtf(g.s2);
    g.q = (((gxx * gxx) + (gyy * gyy)) * -0.5f) - (gxy * gyx);
    return g;
}

// Edge velocities of one sub-domain: for side d = E, N, W, S (Dir order) the
// planar pair [2][len(d)] (ux then uy; len = h for E / W, w for N / S) at
// float offset edge_off(d).  `out` holds this sub-domain's own outermost
// column / row of side d, `in` what lies across side d: out[OPP(d)] of nb[d].
struct EdgeLayout {
    int w, h;
    __host__ __device__ int len(int d) const { return (d & 1) ? w : h; }
    __host__ __device__ long long off(int d) const {
        return d == 0 ? 0 : d == 1 ? 2LL * h : d == 2 ? 2LL * h + 2LL * w : 4LL * h + 2LL * w;
    }
    __host__ __device__ long long total() const { return 4LL * h + 4LL * w; }
};

struct GradArgs : LatticeView {
    const float *in;       // edge velocities across the four sides (EdgeLayout)
    float *edge_out;       // edge kernel: this sub-domain's own edges (EdgeLayout)
    float *out[4];         // LBM_GRAD_* staging arrays float[h][sp]; a null array is not stored
    int strips, segs;      // work items: strips x segs waves
    double *sum_part;      // stats: [2][blocks] fp64 partial sums (w2, then s2)
    float *max_part;       // stats: [2][blocks] partial maxima (|vorticity|, then |divergence|)
};

// ---- D3Q19 ----

constexpr int G3X = 16, G3Y = 16;   // block: 16 lane quads (64 cells) along x by 16 rows, all owned
constexpr int G3W = 4 * G3X;
constexpr int G3_SEG = 32;          // owned planes of the G3_SEG + 2 a block walks

struct Grad3 {
    float wx, wy, wz, vorticity, divergence, strain, q, s2;
};

// px / mx: the velocity (ux, uy, uz) at the +x / -x neighbour; py / my, pz / mz likewise
__device__ __forceinline__ Grad3 gradients3(const float (&px)[3], const float (&mx)[3], const float (&py)[3],
                                            const float (&my)[3], const float (&pz)[3], const float (&mz)[3]) {
    const float gxx = (px[0] - mx[0]) * 0.5f, gxy = (py[0] - my[0]) * 0.5f, gxz = (pz[0] - mz[0]) * 0.5f;
    const float gyx = (px[1] - mx[1]) * 0.5f, gyy = (py[1] - my[1]) * 0.5f, gyz = (pz[1] - mz[1]) * 0.5f;
    const float gzx = (px[2] - mx[2]) * 0.5f, gzy = (py[2] - my[2]) * 0.5f, gzz = (pz[2] - mz[2]) * 0.5f;
    Grad3 g;
    g.wx = gzy - gyz;
    g.wy = gxz - gzx;
    g.wz = gyx - gxy;
    g.vorticity = sqrtf(((g.wx * g.wx) + (g.wy * g.wy)) + (g.wz * g.wz));
    g.divergence = (gxx + gyy) + gzz;
    const float sxy = (gxy + gyx) * 0.5f, sxz = (gxz + gzx) * 0.5f, syz = (gyz + gzy) * 0.5f;
    g.s2 = (((gxx * gxx) + (gyy * gyy)) + (gzz * gzz)) + ((((sxy * sxy) + (sxz * sxz)) + (syz * syz)) * 2.f);
    g.strain = sqrtf(g.s2);
    g.q = ((((gxx * gxx) + (gyy * gyy)) + (gzz * gzz)) * -0.5f) - (((gxy * gyx) + (gxz * gzx)) + (gyz * gzy));
    return g;
}

// the view with quad = (x0 % 4 == 0) and sp = roundup(bx, 4) whatever the box width
struct Grad3Args : Box3View {
    int nzs;               // planes of the slab
    // velocities of the planes beyond the slab: below (z = -1) and above (z = nzs),
    // planar [3][ny][hp] each (ux, uy, uz)
    const float *below, *above;
    int hp;                // row pitch of the two planes
    float *out[7];         // LBM3D_GRAD_* staging arrays float[bz][by][sp]; a null array is not stored
    double *sum_part;      // stats: [2][blocks]
    float *max_part;       // stats: [2][blocks]
};

}  // namespace grad
}  // namespace lbm
