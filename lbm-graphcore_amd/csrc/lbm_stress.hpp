// lbm_stress.hpp -- what the non-equilibrium strain-rate kernels of both
// engines share (lbm_stress.hip, lbm3d_stress.hip; include/lbm_stress_hip.h):
// the per-cell expression of the definition, the argument blocks of the
// kernels, the work-unit sizes and the cell classes of the near-wall map.
//
// Arithmetic: IEEE fp32 in the order the header writes, no contraction
// (-ffp-contract=off), correctly rounded divide and sqrt (hipcc default).
// rho and the velocities are cell_macro's / cell3_macro's, so they are
// lbm_store_fields' own by construction.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lbm3d_cell_macro.hpp"
#include "lbm_cell_macro.hpp"
#include "lbm_views.hpp"

namespace lbm {
namespace stress {

// cell classes of the statistics' map (one byte per cell, built at the first
// statistics call): an obstacle, a fluid cell with no blocked lattice
// neighbour, a fluid cell with at least one
enum : uint8_t { CLS_FLUID = 0, CLS_BLOCKED = 1, CLS_NEAR_WALL = 2 };

// ---- D2Q9 ----

// a lane takes ST_ITER quads (four consecutive cells of a row) a block apart:
// a block of ST_BLOCK lanes owns ST_BLOCK * ST_ITER consecutive quads of the
// row-major quad order
constexpr int ST_BLOCK = 256;
constexpr int ST_ITER = 8;
constexpr int ST_BLOCK_QUADS = ST_BLOCK * ST_ITER;

struct Strain2 {
    float sxx, sxy, syy, strain, s2;
};

// coef = (-1.5f * omega) / (1.f - omega), formed once on the host in fp32 (neq_strain_coef, lbm_diag_host.hpp)
__device__ __forceinline__ Strain2 neq_strain2(const float (&c)[9], bool blocked, float coef) {
    Strain2 s{0.f, 0.f, 0.f, 0.f, 0.f};
    if (blocked) return s;
    float rho;
    const CellMacro m = cell_macro<true, false>(c, false, 0.f, rho);
    const float pxx = ((((c[1] + c[3]) + c[5]) + c[6]) + c[7]) + c[8];
    const float pyy = ((((c[2] + c[4]) + c[5]) + c[6]) + c[7]) + c[8];
    const float pxy = (c[5] + c[7]) - (c[6] + c[8]);
    const float p = rho * (1.f / 3.f);
    const float nxx = (pxx - p) - ((rho * m.ux) * m.ux);
    const float nyy = (pyy - p) - ((rho * m.uy) * m.uy);
    const float nxy = pxy - ((rho * m.ux) * m.uy);
    const float k = coef / rho;
    s.sxx = nxx * k;
    s.syy = nyy * k;
    s.sxy = nxy * k;
    s.s2 = ((s.sxx * s.sxx) + (s.syy * s.syy)) + ((s.sxy * s.sxy) * 2.f);
    s.strain = sqrtf(s.s2);
    return s;
}

// obst: the obstacle map (store), or the class map CLS_* (stats)
struct StressArgs : LatticeView {
    float coef;            // neq_strain_coef(omega)
    float *out[4];         // LBM_STRESS_* staging arrays float[h][sp]; a null array is not stored
    double *sum_part;      // stats: [2][blocks] fp64 partial sums (s2, then near-wall strain)
    float *max_part;       // stats: [2][blocks] partial maxima (strain, then near-wall strain)
};

// ---- D3Q19 ----

// block: 64 lanes along x (one wave) by S3Y rows, walking S3Z consecutive planes
constexpr int S3X = 64, S3Y = 4, S3Z = 8;

struct Strain3 {
    float sxx, syy, szz, sxy, sxz, syz, strain, s2;
};

__device__ __forceinline__ Strain3 neq_strain3(const float (&c)[19], bool blocked, float coef) {
    Strain3 s{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (blocked) return s;
    float rho;
    const Cell3Macro m = cell3_macro<true, false>(c, false, 0.f, rho);
    const float pxx = ((((((((c[1] + c[2]) + c[5]) + c[6]) + c[7]) + c[8]) + c[10]) + c[11]) + c[15]) + c[16];
    const float pyy = ((((((((c[3] + c[4]) + c[5]) + c[6]) + c[7]) + c[8]) + c[12]) + c[13]) + c[17]) + c[18];
    const float pzz = ((((((((c[9] + c[10]) + c[11]) + c[12]) + c[13]) + c[14]) + c[15]) + c[16]) + c[17]) + c[18];
    const float pxy = (c[5] + c[6]) - (c[7] + c[8]);
    const float pxz = (c[10] + c[15]) - (c[11] + c[16]);
    const float pyz = (c[12] + c[17]) - (c[13] + c[18]);
    const float p = rho * (1.f / 3.f);
    const float nxx = (pxx - p) - ((rho * m.ux) * m.ux);
    const float nyy = (pyy - p) - ((rho * m.uy) * m.uy);
    const float nzz = (pzz - p) - ((rho * m.uz) * m.uz);
    const float nxy = pxy - ((rho * m.ux) * m.uy);
    const float nxz = pxz - ((rho * m.ux) * m.uz);
    const float nyz = pyz - ((rho * m.uy) * m.uz);
    const float k = coef / rho;
    s.sxx = nxx * k;
    s.syy = nyy * k;
    s.szz = nzz * k;
    s.sxy = nxy * k;
    s.sxz = nxz * k;
    s.syz = nyz * k;
    s.s2 = (((s.sxx * s.sxx) + (s.syy * s.syy)) + (s.szz * s.szz)) +
           ((((s.sxy * s.sxy) + (s.sxz * s.sxz)) + (s.syz * s.syz)) * 2.f);
    s.strain = sqrtf(s.s2);
    return s;
}

// obst: the obstacle map (store), or the class map CLS_* (stats)
struct Stress3Args : Box3View {
    float coef;            // neq_strain_coef(omega)
    float *out[7];         // LBM3D_STRESS_* staging arrays float[bz][by][sp]; a null array is not stored
    double *sum_part;      // stats: [2][blocks]
    float *max_part;       // stats: [2][blocks]
};

}  // namespace stress
}  // namespace lbm
