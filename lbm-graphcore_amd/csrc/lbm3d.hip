// lbm3d.hip -- kernels of the D3Q19-BGK engine (include/lbm3d_hip.h) and their
// launch_* wrappers (lbm3d_engine.hpp): BASELINE config 5, SURVEY 8f rank 4.
// The reference has no 3-D code; this is the 3-D analogue
// of its fused D2Q9 step (main/LastChance.cpp:192-266) on the same machinery
// as the D2Q9 engine: SoA lattice pair, one fused pull-stream / bounce-back /
// BGK / body-force / |u| kernel, device-side per-step |u| partials, slab
// decomposition with halos over RCCL (or device copies), boundary planes on a
// high-priority stream so the exchange overlaps the interior (the host side
// is in lbm3d_engine.hip).
//
// Layout per slab of nzs planes: f[z + 2][k][y][px] for -2 <= z <= nzs + 1 (two
// ghost planes below and above: the one-step kernels read the inner ones, the
// two-step kernel both); speeds ordered so that the five that cross
// the top face (c_z = +1: 9..13) and the five that cross the bottom face
// (c_z = -1: 14..18) are each ONE contiguous block of a plane -- the halo
// message of a face is a single contiguous range of the lattice, sent and
// received in place (no pack / unpack kernels).  x and y wrap in-kernel.
//
// Bandwidth-bound: 152 algorithmic bytes per cell update (19 fp32 loads + 19
// stores); no MFMA.  Arithmetic in IEEE fp32 evaluated in the order of
// oracle/lbm_oracle3d.c (-ffp-contract=off, correctly rounded / and sqrt), so
// the lattice is bitwise equal to the CPU restatement.
//
// Every kernel is built from the same pieces, each written once: the cell
// (rebound3 for an obstacle; cell3d, or cell3dt in tolerance mode, for fluid),
// the block fold of |u| (fold_levels) and, for the two- and three-step
// passes, a level's LDS publish, pull gather and reload (publish3, gather3,
// reload3).  The kernels differ in how they pull and in how many steps a pass
// over the lattice makes: step3d (one cell per lane), step3d_pair (a column
// pair per lane), step3d_two and step3d_three (two and three steps per pass).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "lbm3d_engine.hpp"
#include "lbm_packed.hpp"

#ifndef LBM3D_XCD_REMAP
#define LBM3D_XCD_REMAP 1  // 0: the hardware's block order (A/B builds only)
#endif

namespace lbm {

constexpr int B3X = 64, B3Y = 4;  // block: 64 x-columns (one wave) x 4 rows
static_assert(B3X == 64, "the one-step kernels fold a row as one wave");

// bounce-back of an obstacle cell: out_k = s_opp(k)
__device__ __forceinline__ void rebound3(const float (&s)[Q3], float (&o)[Q3]) {
    o[0] = s[0];
    o[1] = s[2];
    o[2] = s[1];
    o[3] = s[4];
    o[4] = s[3];
    o[5] = s[6];
    o[6] = s[5];
    o[7] = s[8];
    o[8] = s[7];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        o[9 + i] = s[14 + i];
        o[14 + i] = s[9 + i];
    }
}

// One D3Q19 cell: pulled populations s -> outputs o (the order of
// oracle/lbm_oracle3d.c cell3d); returns |u| (0 for an obstacle).  |u| feeds
// av_vels only: by v_sqrt_f32 (<= 1 ulp, as lbm_packed.hpp sqrt_av), or
// (IEEE_ROOT, the one-cell kernel) correctly rounded.
template <bool IEEE_ROOT = false>
__device__ __forceinline__ float cell3d(const float (&s)[Q3], float (&o)[Q3], bool ob, float omega, float omo,
                                        float w1, float w2) {
    if (ob) {
        rebound3(s, o);
        return 0.f;
    }
    const float rho = s[0] + s[1] + s[2] + s[3] + s[4] + s[5] + s[6] + s[7] + s[8] + s[9] + s[10] + s[11] + s[12] +
                      s[13] + s[14] + s[15] + s[16] + s[17] + s[18];
    // correctly rounded divisions for every input (lbm_packed.hpp header):
    // the velocity components by the compiler's IEEE sequence; x/3 by the
    // short sequence (exhaustively exact for every float x); x/18 and x/36
    // by it for x >= 2^-120 (exhaustive: exact from 2^-125 / 2^-124 up), by
    // IEEE division in a wave holding a smaller density (never in physical states)
    auto cdiv = [](float x, float d, float y) {
        const float q = x * y;
        return __builtin_fmaf(__builtin_fmaf(-d, q, x), y, q);
    };
    const float ux = ((s[1] + s[5] + s[7] + s[10] + s[16]) - (s[2] + s[6] + s[8] + s[11] + s[15])) / rho;
    const float uy = ((s[3] + s[5] + s[8] + s[12] + s[18]) - (s[4] + s[6] + s[7] + s[13] + s[17])) / rho;
    const float uz = ((s[9] + s[10] + s[11] + s[12] + s[13]) - (s[14] + s[15] + s[16] + s[17] + s[18])) / rho;
    const float usq = ux * ux + uy * uy + uz * uz;
    const float c = 1.00f - usq * 1.50f;
    const float ld0 = cdiv(rho, 3.00f, 1.00f / 3.00f) * omega;
    float r18 = cdiv(rho, 18.00f, 1.00f / 18.00f), r36 = cdiv(rho, 36.00f, 1.00f / 36.00f);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(!(rho >= 0x1p-120f)) != 0, 0)) {
        r18 = rho / 18.00f;
        r36 = rho / 36.00f;
    }
    const float ld1 = r18 * omega;
    const float ld2 = r36 * omega;
    const float pxy = ux + uy, mxy = ux - uy, pxz = ux + uz, mxz = -ux + uz, pyz = uy + uz, myz = -uy + uz;
    const float e[Q3] = {0.f, ux, -ux, uy, -uy, pxy, -pxy, mxy, -mxy, uz, pxz, mxz, pyz, myz,
                         -uz, -pxz, -mxz, -pyz, -myz};
    o[0] = s[0] * omo + ld0 * c;
#pragma unroll
    for (int k = 1; k < Q3; ++k) {
        const float ld = (k <= 4 || k == 9 || k == 14) ? ld1 : ld2;
        o[k] = s[k] * omo + ld * ((4.50f * e[k]) * (2.00f / 3.00f + e[k]) + c);
    }
    o[1] = o[1] + w1;
    o[2] = o[2] - w1;
    o[5] = o[5] + w2;
    o[6] = o[6] - w2;
    o[7] = o[7] + w2;
    o[8] = o[8] - w2;
    o[10] = o[10] + w2;
    o[11] = o[11] - w2;
    o[15] = o[15] - w2;
    o[16] = o[16] + w2;
    return IEEE_ROOT ? sqrtf(usq) : __builtin_amdgcn_sqrtf(usq);
}

// LBM_FLAG_TOLERANCE form of cell3d (the 2-D collide2t's reassociation in
// 3-D): one reciprocal of rho (v_rcp_f32, 1 ulp, no Newton step) for the velocity,
// carried scaled (v = 3u), rho * (omega / 3 | 18 | 36), and per pair of
// opposite speeds out_k = fma(s_k, 1 - omega, P) +- Q with P = ld (v^2 / 2 +
// c), c = 1 - |v|^2 / 6, Q = ld v (+ the body-force weight of the pair, which
// enters the two outputs with opposite signs).  Not bitwise equal to
// oracle/lbm_oracle3d.c; checked against it within a stated tolerance
// (tests/test_d3q19.py test_d3q19_tolerance_*).  k = {1 - omega, omega/3,
// omega/18, omega/36}.
__device__ __forceinline__ float cell3dt(const float (&s)[Q3], float (&o)[Q3], bool ob, float omo, float k0, float k1,
                                         float k2, float w1, float w2) {
    if (ob) {
        rebound3(s, o);
        return 0.f;
    }
    const float ax = s[1] + s[5] + s[7] + s[10] + s[16], bx = s[2] + s[6] + s[8] + s[11] + s[15];
    const float ay = s[3] + s[5] + s[8] + s[12] + s[18], by = s[4] + s[6] + s[7] + s[13] + s[17];
    const float az = s[9] + s[10] + s[11] + s[12] + s[13], bz = s[14] + s[15] + s[16] + s[17] + s[18];
    // ax + bx holds speeds 1, 2, 5-8, 10, 11, 15, 16; the rest of the 19 here
    const float rho = ((s[0] + (s[3] + s[4])) + (ax + bx)) + ((s[9] + s[12] + s[13]) + (s[14] + s[17] + s[18]));
    const float r = __builtin_amdgcn_rcpf(rho);
    const float r3 = r * 3.00f;
    const float vx = (ax - bx) * r3, vy = (ay - by) * r3, vz = (az - bz) * r3;  // 3 u
    const float h = __builtin_fmaf(vx, vx, __builtin_fmaf(vy, vy, vz * vz));   // 9 |u|^2
    const float c = __builtin_fmaf(h, -1.00f / 6.00f, 1.00f);
    const float ld1 = rho * k1, ld2 = rho * k2;
    o[0] = __builtin_fmaf(s[0], omo, (rho * k0) * c);
    // q: the pair's +- term, w: its body-force weight (+w on kp, -w on km)
    auto pair = [&](int kp, int km, float v, float ld, float w) {
        const float p = ld * __builtin_fmaf(v * v, 0.50f, c), q = __builtin_fmaf(ld, v, w);
        o[kp] = __builtin_fmaf(s[kp], omo, p) + q;
        o[km] = __builtin_fmaf(s[km], omo, p) - q;
    };
    auto pair0 = [&](int kp, int km, float v, float ld) {  // no body force on this pair
        const float p = ld * __builtin_fmaf(v * v, 0.50f, c);
        o[kp] = __builtin_fmaf(ld, v, __builtin_fmaf(s[kp], omo, p));
        o[km] = __builtin_fmaf(-ld, v, __builtin_fmaf(s[km], omo, p));
    };
    pair(1, 2, vx, ld1, w1);
    pair0(3, 4, vy, ld1);
    pair0(9, 14, vz, ld1);
    pair(5, 6, vx + vy, ld2, w2);
    pair(7, 8, vx - vy, ld2, w2);
    pair(10, 15, vx + vz, ld2, w2);
    pair(11, 16, vz - vx, ld2, -w2);
    pair0(12, 17, vy + vz, ld2);
    pair0(13, 18, vz - vy, ld2);
    return __builtin_amdgcn_sqrtf(h) * (1.00f / 3.00f);  // |u|, av_vels only
}

// Block sums of the per-thread u[0 .. N) of a block of NW waves, in a fixed
// order: lanes by __shfl_down 32..1, then the waves in row order by thread 0,
// which writes level l's sum to partials[l * nblocks + blk].  lane / w: the
// thread's lane and wave (row).  Every thread of the block must reach it (it
// holds a barrier).
template <int N, int NW>
__device__ __forceinline__ void fold_levels(float (&u)[N], float (&red)[N][NW], int lane, int w, float *partials,
                                            int nblocks, long long blk) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int l = 0; l < N; ++l) u[l] += __shfl_down(u[l], off, 64);
    }
    if (lane == 0) {
#pragma unroll
        for (int l = 0; l < N; ++l) red[l][w] = u[l];
    }
    __syncthreads();
    if (lane == 0 && w == 0) {
#pragma unroll
        for (int l = 0; l < N; ++l) {
            float b = red[l][0];
#pragma unroll
            for (int i = 1; i < NW; ++i) b += red[l][i];
            partials[l * nblocks + blk] = b;
        }
    }
}

// the one-step kernels' fold: one level, the block's partial at its grid index
__device__ __forceinline__ void fold_block3(float usum, float (&red)[1][B3Y], float *partials) {
    float u[1] = {usum};
    fold_levels(u, red, threadIdx.x, threadIdx.y, partials, 0,
                ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
}

// One cell per lane, one plane per block: the kernel of odd nx (LBM3D_PAIR=0
// forces it).  Same cell3d arithmetic as every other kernel; its |u| keeps
// the correctly rounded root.
__global__ __launch_bounds__(B3X * B3Y) void step3d(Step3Args a) {
    __shared__ float red[1][B3Y];
    const int x = blockIdx.x * B3X + threadIdx.x;
    const int y = blockIdx.y * B3Y + threadIdx.y;
    const int z = a.z0 + blockIdx.z;
    float usum = 0.f;
    if (x < a.nx && y < a.ny) {
        const int xw = x == 0 ? a.nx - 1 : x - 1, xe = x == a.nx - 1 ? 0 : x + 1;
        const int ys = y == 0 ? a.ny - 1 : y - 1, yn = y == a.ny - 1 ? 0 : y + 1;
        const long long PL = a.PL, KS = a.KS;
        const int px = a.px;
        // pulled populations s_k = f_k(x - cx, y - cy, z - cz)
        const float *p0 = a.fin + (long long)z * PL;  // plane z
        const float *pm = p0 - PL;                     // plane z-1 (c_z = +1 pulls from below)
        const float *pp = p0 + PL;                     // plane z+1
        const long long ry = (long long)y * px, rs = (long long)ys * px, rn = (long long)yn * px;
        float s[Q3];
        s[0] = p0[0 * KS + ry + x];
        s[1] = p0[1 * KS + ry + xw];
        s[2] = p0[2 * KS + ry + xe];
        s[3] = p0[3 * KS + rs + x];
        s[4] = p0[4 * KS + rn + x];
        s[5] = p0[5 * KS + rs + xw];
        s[6] = p0[6 * KS + rn + xe];
        s[7] = p0[7 * KS + rn + xw];
        s[8] = p0[8 * KS + rs + xe];
        s[9] = pm[9 * KS + ry + x];
        s[10] = pm[10 * KS + ry + xw];
        s[11] = pm[11 * KS + ry + xe];
        s[12] = pm[12 * KS + rs + x];
        s[13] = pm[13 * KS + rn + x];
        s[14] = pp[14 * KS + ry + x];
        s[15] = pp[15 * KS + ry + xe];
        s[16] = pp[16 * KS + ry + xw];
        s[17] = pp[17 * KS + rn + x];
        s[18] = pp[18 * KS + rs + x];
        float o[Q3];
        const bool ob = a.obst[((long long)blockIdx.z * a.ny + y) * a.nx + x] != 0;
        usum = cell3d<true>(s, o, ob, a.omega, a.omo, a.w1, a.w2);
        float *d = a.fout + (long long)z * PL + ry + x;
#pragma unroll
        for (int k = 0; k < Q3; ++k) d[k * KS] = o[k];
    }
    fold_block3(usum, red, a.partials);
}

// Two cells per lane (a column pair, nx even): every load and store is a
// float2 (512 B per wave instruction instead of 256); the x-shifted pulls
// take the neighbour column from the adjacent lane by DPP, and the first /
// last pair of a wave (or of a row, with the periodic wrap) loads it
// directly.  Each block walks ZB planes, so the per-step |u| partials are
// ZB times fewer.  Bitwise equal to step3d (same cell3d arithmetic).
template <int ZB, bool NT>
__global__ __launch_bounds__(B3X * B3Y) void step3d_pair(Step3Args a, int planes) {
    __shared__ float red[1][B3Y];
    const int lane = threadIdx.x;
    const int xa = blockIdx.x * (2 * B3X) + 2 * lane;
    const int y = blockIdx.y * B3Y + threadIdx.y;
    const bool active = xa < a.nx && y < a.ny;
    float usum = 0.f;
    const long long PL = a.PL, KS = a.KS;
    const int px = a.px, nx = a.nx;
    const int yc = min(y, a.ny - 1);  // inactive rows read a valid row
    const int ys = yc == 0 ? a.ny - 1 : yc - 1, yn = yc + 1 >= a.ny ? 0 : yc + 1;
    const long long ry = (long long)yc * px, rs = (long long)ys * px, rn = (long long)yn * px;
    const int xc = min(xa, nx - 2);  // clamped pair base for inactive lanes
    const bool first = lane == 0 || xa == 0;
    const bool last = lane == B3X - 1 || xa + 2 >= nx;
    const int xl = xa == 0 ? nx - 1 : xa - 1;   // column left of the pair (periodic)
    const int xr = xa + 2 >= nx ? 0 : xa + 2;   // column right of the pair
    const int zb0 = blockIdx.z * ZB;
    for (int zi = 0; zi < ZB; ++zi) {
        const int zl = zb0 + zi;
        if (zl >= planes) break;
        const int z = a.z0 + zl;
        const float *p0 = a.fin + (long long)z * PL;
        const float *pm = p0 - PL, *pp = p0 + PL;
        auto L2 = [&](const float *base, int k, long long row) {
            return *reinterpret_cast<const f2 *>(base + k * KS + row + xc);
        };
        f2 s2[Q3];
        s2[0] = L2(p0, 0, ry);
        s2[1] = left2(L2(p0, 1, ry));
        s2[2] = right2(L2(p0, 2, ry));
        s2[3] = L2(p0, 3, rs);
        s2[4] = L2(p0, 4, rn);
        s2[5] = left2(L2(p0, 5, rs));
        s2[6] = right2(L2(p0, 6, rn));
        s2[7] = left2(L2(p0, 7, rn));
        s2[8] = right2(L2(p0, 8, rs));
        s2[9] = L2(pm, 9, ry);
        s2[10] = left2(L2(pm, 10, ry));
        s2[11] = right2(L2(pm, 11, ry));
        s2[12] = L2(pm, 12, rs);
        s2[13] = L2(pm, 13, rn);
        s2[14] = L2(pp, 14, ry);
        s2[15] = right2(L2(pp, 15, ry));
        s2[16] = left2(L2(pp, 16, ry));
        s2[17] = L2(pp, 17, rn);
        s2[18] = L2(pp, 18, rs);
        if (first && active) {  // pulls from x - 1: speeds 1, 5, 7, 10, 16
            s2[1].x = p0[1 * KS + ry + xl];
            s2[5].x = p0[5 * KS + rs + xl];
            s2[7].x = p0[7 * KS + rn + xl];
            s2[10].x = pm[10 * KS + ry + xl];
            s2[16].x = pp[16 * KS + ry + xl];
        }
        if (last && active) {   // pulls from x + 1: speeds 2, 6, 8, 11, 15
            s2[2].y = p0[2 * KS + ry + xr];
            s2[6].y = p0[6 * KS + rn + xr];
            s2[8].y = p0[8 * KS + rs + xr];
            s2[11].y = pm[11 * KS + ry + xr];
            s2[15].y = pp[15 * KS + ry + xr];
        }
        if (active) {
            const uint16_t ob2 = *reinterpret_cast<const uint16_t *>(a.obst + ((long long)zl * a.ny + y) * nx + xa);
            float sa[Q3], sb[Q3], oa[Q3], obv[Q3];
#pragma unroll
            for (int k = 0; k < Q3; ++k) {
                sa[k] = s2[k].x;
                sb[k] = s2[k].y;
            }
            usum += cell3d(sa, oa, (ob2 & 0xffu) != 0, a.omega, a.omo, a.w1, a.w2);
            usum += cell3d(sb, obv, (ob2 >> 8) != 0, a.omega, a.omo, a.w1, a.w2);
            float *d = a.fout + (long long)z * PL + ry + xa;
#pragma unroll
            for (int k = 0; k < Q3; ++k) {
                if (NT)
                    __builtin_nontemporal_store(f2{oa[k], obv[k]}, reinterpret_cast<f2 *>(d + k * KS));
                else
                    *reinterpret_cast<f2 *>(d + k * KS) = f2{oa[k], obv[k]};
            }
        }
    }
    fold_block3(usum, red, a.partials);
}

// ---------------------------------------------------------------------------
// Two time steps per pass over the lattice (one slab, z periodic): 2.5-D
// temporal blocking.  A block of 64 columns (one wave, one column per lane) x
// 12 rows (one wave per row) walks a segment of z planes; as input plane j
// arrives (step t, 19 coalesced loads per lane), level 1 computes plane j-1 at
// t+1 and level 2 computes plane j-2 at t+2 from level 1's planes, so the
// lattice crosses HBM once per two steps.  Owned outputs: the inner 60 x 8
// cells (a two-cell ring in x and y is recomputed).
// Pulls, per level, for the centre plane z (input plane z+1 just arrived):
//   own row, x +- 1 by DPP:   speeds 0,1,2 of plane z, 9,10,11 of plane z-1
//                             (registers kept from earlier iterations),
//                             14,15,16 of plane z+1;
//   rows y +- 1 through LDS:  3..8 of plane z (one slot set, read into
//                             registers the iteration plane z arrives),
//                             12,13 of plane z-1 (ring of 3), 17,18 of z+1.
// Two barriers per iteration (one per level) order every slot's writes and
// reads (each slot is rewritten only after the barrier that follows its last
// read).  Algorithmic traffic per cell update: (19 loads x 64 x 12 / (60 x 8)
// + 19 stores) x 4 B / 2 = 98.8 B instead of 152.  Same cell3d arithmetic:
// bitwise equal to the one-step kernels.
// ---------------------------------------------------------------------------
// The block of both passes: 64 columns x 12 rows (waves).  A level's LDS is 14
// plane slots of 64 x 12 floats = 42 KB: two levels 84 KB, three 126 KB (one
// block per CU, three waves per SIMD).  Blocks of 14-16 rows, a dead-row skip
// in the two-step pass and two prefetched planes were measured and removed
// (profiles/r02/d3q19/ab_two_th_skip_pd.log, profiles/r03/d3q19/ab_pd.log).
constexpr int T3W = 64;             // columns (lanes) per block
constexpr int T3TH = 12;            // rows (waves) per block
constexpr int T3C = T3W * T3TH;     // cells per plane slot
// Z (speeds 3..8 of the newest plane) is single-buffered: each thread reads
// its six y +- 1 pulls right after the barrier that publishes them and keeps
// them in registers (zr) until the next iteration, when that plane is the
// centre plane -- 14 slots per level instead of 20.
constexpr int T3LDS = (2 + 6 + 3 * 2) * T3C;         // floats per level: M[2], Z[6], P[3][2]
constexpr int T3OX = T3W - 4, T3OY = T3TH - 4;       // owned columns / rows of the two-step pass
constexpr int T3OX3 = T3W - 6, T3OY3 = T3TH - 6;     // ... of the three-step pass

// XCD-aware block order for the multi-step passes (as the 2-D stream
// kernel's xcd_remap, lbm_device.hpp): the hardware deals workgroups to the
// eight XCDs round robin, so consecutive blocks -- x neighbours, whose
// windows overlap by six columns, and y neighbours, overlapping by six rows
// -- landed on different XCDs and read their shared cells from HBM twice.
// Here each XCD takes one contiguous range of (x fastest, then y, then z)
// blocks, so neighbours run side by side on one XCD and the overlap comes
// from its L2.  Blocks keep their logical index for the |u| partials.
struct Blk3 {
    int x, y, z;
};
__device__ __forceinline__ Blk3 blk3_remap() {
    const int nb = gridDim.x * gridDim.y * gridDim.z;
    const int lin = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
    const int l = LBM3D_XCD_REMAP ? xcd_remap(lin, nb) : lin;
    const int yz = l / gridDim.x;
    return Blk3{l - yz * (int)gridDim.x, yz % (int)gridDim.y, yz / (int)gridDim.y};
}

// per-thread LDS offsets (floats) of a level's slots, loop-invariant; the
// neighbours of the block's edge rows and lanes are clamped (those cells are
// in the recomputed ring, never owned)
struct Lds3 {
    int c, ym, yp, ymxm, ypxp, ypxm, ymxp;  // own cell; y-1; y+1; (y-1,x-1); (y+1,x+1); (y+1,x-1); (y-1,x+1)
};
__device__ __forceinline__ Lds3 lds3_offsets(int lane, int wy) {
    const int wm = max(wy - 1, 0) * T3W, wp = min(wy + 1, T3TH - 1) * T3W;
    const int lm = max(lane - 1, 0), lp = min(lane + 1, T3W - 1);
    return Lds3{wy * T3W + lane, wm + lane, wp + lane, wm + lm, wp + lp, wp + lm, wm + lp};
}

// A level's three steps around its barrier, for input plane jz (in) and
// centre plane jz - 1.  The level's LDS: M (speeds 17, 18 of plane jz), Z
// (3..8 of plane jz), P (12, 13 of planes jz, jz - 1, jz - 2, a ring of three
// slot pairs).  publish3 before the barrier: the thread's own cell of plane
// jz, P-ring slot pin.
__device__ __forceinline__ void publish3(float *lds, const float (&in)[Q3], int pin, const Lds3 &d) {
    float *M = lds, *Z = lds + 2 * T3C, *P = lds + 8 * T3C;
    M[d.c] = in[17];
    M[T3C + d.c] = in[18];
#pragma unroll
    for (int i = 0; i < 6; ++i) Z[i * T3C + d.c] = in[3 + i];
    P[(pin * 2) * T3C + d.c] = in[12];
    P[(pin * 2 + 1) * T3C + d.c] = in[13];
}

// gather3 after the barrier: the 19 pulls of the centre plane -- which delay
// line, which LDS slot and which DPP shift feeds which speed.  r0: speeds 0,
// 1, 2 of the centre plane; zr: its y +- 1 pulls of 3..8 (reload3, one plane
// ago); r9: speeds 9, 10, 11 of plane jz - 2; pold: the P-ring slot of plane
// jz - 2.
__device__ __forceinline__ void gather3(float (&s)[Q3], const float (&in)[Q3], const float (&r0)[3],
                                        const float (&zr)[6], const float (&r9)[3], const float *lds, int pold,
                                        const Lds3 &d) {
    const float *M = lds, *p = lds + 8 * T3C + pold * 2 * T3C;
    s[0] = r0[0];
    s[1] = dpp_from_left(r0[1]);
    s[2] = dpp_from_right(r0[2]);
#pragma unroll
    for (int i = 0; i < 6; ++i) s[3 + i] = zr[i];
    s[9] = r9[0];
    s[10] = dpp_from_left(r9[1]);
    s[11] = dpp_from_right(r9[2]);
    s[12] = p[d.ym];
    s[13] = p[T3C + d.yp];
    s[14] = in[14];
    s[15] = dpp_from_right(in[15]);
    s[16] = dpp_from_left(in[16]);
    s[17] = M[d.yp];
    s[18] = M[T3C + d.ym];
}

// reload3 after the barrier: plane jz's y +- 1 pulls of speeds 3..8, for the
// next plane (the Z slots are rewritten only after this level's next barrier)
__device__ __forceinline__ void reload3(float (&zr)[6], const float *lds, const Lds3 &d) {
    const float *Z = lds + 2 * T3C;
    zr[0] = Z[0 * T3C + d.ym];
    zr[1] = Z[1 * T3C + d.yp];
    zr[2] = Z[2 * T3C + d.ymxm];
    zr[3] = Z[3 * T3C + d.ypxp];
    zr[4] = Z[4 * T3C + d.ypxm];
    zr[5] = Z[5 * T3C + d.ymxp];
}

// the collision of a level: the numerics the pass is instantiated for
template <bool TOL>
__device__ __forceinline__ float collide3(const float (&s)[Q3], float (&out)[Q3], bool ob, const Two3Args &a) {
    if constexpr (TOL)
        return cell3dt(s, out, ob, a.omo, a.k0, a.k1, a.k2, a.w1, a.w2);
    else
        return cell3d(s, out, ob, a.omega, a.omo, a.w1, a.w2);
}

// One level of the two-step pass for centre plane jz - 1, input plane jz (in).
// Must be reached by every thread of the block (it holds a barrier).  One
// register set per delay line, rotated by copies: r0 and zr as gather3's;
// r9a / r9b: speeds 9, 10, 11 of planes jz - 1 and jz - 2.
template <bool TOL>
__device__ __forceinline__ float level3(const float (&in)[Q3], float (&out)[Q3], float *lds, int jz, float (&r0)[3],
                                        float (&r9a)[3], float (&r9b)[3], float (&zr)[6], const Lds3 &d, bool ob,
                                        const Two3Args &a) {
    publish3(lds, in, ((jz % 3) + 3) % 3, d);
    __syncthreads();
    float s[Q3];
    gather3(s, in, r0, zr, r9b, lds, (((jz - 2) % 3) + 3) % 3, d);
    reload3(zr, lds, d);
    const float u = collide3<TOL>(s, out, ob, a);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        r9b[i] = r9a[i];
        r9a[i] = in[9 + i];
        r0[i] = in[i];
    }
    return u;
}

// PD: input planes in flight -- 1: plane j+1 is loaded while j is computed
// (its loads stay in flight across both barriers of the iteration); 0 (the
// default): plane j+1 is loaded into the input registers once level 1 has
// consumed them, in flight across level 2 only (19 VGPRs fewer).
template <int PD, bool TOL = false>
__global__ __launch_bounds__(T3W * T3TH) void step3d_two(Two3Args a) {
    static_assert(PD == 0 || PD == 1, "two_variant() admits these only");
    __shared__ float lds1[T3LDS], lds2[T3LDS];
    __shared__ float red[2][T3TH];
    const int lane = threadIdx.x, wy = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const Blk3 B = blk3_remap();
    const int ox = B.x * T3OX, oy = B.y * T3OY;
    const int x = (((ox - 2 + lane) % a.nx) + a.nx) % a.nx;
    const int y = (((oy - 2 + wy) % a.ny) + a.ny) % a.ny;
    const bool own = lane >= 2 && lane < T3W - 2 && wy >= 2 && wy < T3TH - 2 && ox + lane - 2 < a.nx &&
                     oy + wy - 2 < a.ny;
    const int zs = a.z0 + B.z * a.seg, ze = min(zs + a.seg, a.zn);
    const long long row = (long long)y * a.px + x;
    const Lds3 d = lds3_offsets(lane, wy);
    float r0a[3] = {0.f, 0.f, 0.f}, r9aa[3] = {0.f, 0.f, 0.f}, r9ba[3] = {0.f, 0.f, 0.f};
    float r0b[3] = {0.f, 0.f, 0.f}, r9ab[3] = {0.f, 0.f, 0.f}, r9bb[3] = {0.f, 0.f, 0.f};
    float zra[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, zrb[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float u[2] = {0.f, 0.f};
    auto obz = [&](int zz) {  // planes zs-4 .. ze are asked for; only zs-1 .. ze are used
        zz = min(max(zz, -2), a.nz + 1);
        return a.obst[((long long)zz * a.ny + y) * a.nx + x] != 0;
    };
    float in[Q3];
    bool ob1 = obz(zs - 3), ob2 = obz(zs - 4);
    {
        const float *pl = a.fin + (long long)(zs - 2) * a.PL + row;
#pragma unroll
        for (int k = 0; k < Q3; ++k) in[k] = pl[k * a.KS];
    }
    for (int j = zs - 2; j <= ze + 1; ++j) {
        float nin[Q3];
        const float *pn = a.fin + (long long)min(j + 1, ze + 1) * a.PL + row;
        if (PD == 1) {
#pragma unroll
            for (int k = 0; k < Q3; ++k) nin[k] = pn[k * a.KS];
        }
        ob2 = ob1;
        ob1 = obz(j - 1);
        float o1[Q3], o2[Q3];
        const float v1 = level3<TOL>(in, o1, lds1, j, r0a, r9aa, r9ba, zra, d, ob1, a);
        if (own && j - 1 >= zs && j - 1 < ze) u[0] += v1;
        if (PD == 0) {  // level 1 is done with plane j: its registers take plane j + 1
#pragma unroll
            for (int k = 0; k < Q3; ++k) in[k] = pn[k * a.KS];
        }
        const float v2 = level3<TOL>(o1, o2, lds2, j - 1, r0b, r9ab, r9bb, zrb, d, ob2, a);
        if (own && j - 2 >= zs && j - 2 < ze) {
            u[1] += v2;
            float *dst = a.fout + (long long)(j - 2) * a.PL + row;
#pragma unroll
            for (int k = 0; k < Q3; ++k) __builtin_nontemporal_store(o2[k], dst + k * a.KS);
        }
        if (PD == 1) {
#pragma unroll
            for (int k = 0; k < Q3; ++k) in[k] = nin[k];
        }
    }
    fold_levels(u, red, lane, wy, a.partials, a.nblocks, a.blk0 + (B.z * gridDim.y + B.y) * gridDim.x + B.x);
}

// ---------------------------------------------------------------------------
// step3d_three: three time steps per pass (single slab).  The same 64 x 12
// block and level pieces with a third level: level 1 computes plane
// j-1 at t+1, level 2 plane j-2 at t+2, level 3 plane j-3 at t+3 as input
// plane j arrives.  A three-cell ring in x and y is recomputed: owned 58 x 6
// of 64 x 12 loaded cells, three levels of 14 plane slots = 126 KB of LDS (one
// block per CU, three waves per SIMD).  Algorithmic traffic per cell update:
// (19 x 768 loads + 19 x 348 stores) x 4 B / (3 x 348) = 81.2 B instead of
// 98.8 for two steps per pass (152 for one).  Input planes zs-3 .. ze+2: the
// lattice carries three ghost planes each side (GZ3), refreshed from the
// periodic images before every pass.  Same cell3d / cell3dt arithmetic as the
// other passes: bitwise equal to them (and the oracle) in bitwise mode.

// Per-level delay lines of the three-step pass in two register sets used on
// alternate planes (the plane loop runs two planes per iteration, set P = 0
// then 1): r0[P ^ 1] / zr[P ^ 1] hold what the previous plane left (speeds 0,
// 1, 2 of the centre plane; its y +- 1 pulls of speeds 3..8), r0[P] / zr[P]
// take this plane's; r9[P] holds the speeds 9, 10, 11 of the plane two back
// and takes this plane's.  (One set per delay line, rotated by copies, cost
// ~45 moves per plane iteration plus ~40 loop-carried copies at the back edge.)
struct Lv3 {
    float r0[2][3], r9[2][3], zr[2][6];
};

// level3 for the three-step pass: level L (centre plane jz - 1, input plane
// jz), register set P as above, for a wave whose row is live for the first D
// levels (SKIP: D = min(row, 11 - row, 3); every row D = 3 without it).
// Level L publishes its input only while some live row reads it (L <= D + 1:
// the rows beside a live row are live one level less) and computes only
// while live (L <= D); every level meets its barrier.  Liveness is static per
// instantiation, so no path merges a computed with a skipped result (the
// merges had cost a register move per population and level).
// pin / pold: P-ring slots of planes jz and jz - 2 (wave-uniform).
template <int P, int L, int D, bool TOL>
__device__ __forceinline__ float level3p(const float (&in)[Q3], float (&out)[Q3], float *lds, int pin, int pold,
                                         Lv3 &st, const Lds3 &d, bool ob, const Two3Args &a) {
    if constexpr (L <= D + 1) publish3(lds, in, pin, d);
    __syncthreads();
    if constexpr (L > D) {
        return 0.f;
    } else {
        float s[Q3];
        gather3(s, in, st.r0[P ^ 1], st.zr[P ^ 1], st.r9[P], lds, pold, d);
        reload3(st.zr[P], lds, d);
        const float u = collide3<TOL>(s, out, ob, a);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            st.r9[P][i] = in[9 + i];
            st.r0[P][i] = in[i];
        }
        return u;
    }
}

// The plane loop of one wave (rows live for D levels, see level3p); input
// planes zs-3 .. ze+2, two per iteration (register sets 0 and 1).  Every
// plane base and speed offset is wave-uniform: loads and stores are buffer
// operations on a per-plane descriptor with the speed offset in soffset and
// the lane's cell in voffset (no per-access 64-bit address arithmetic; the
// engine keeps Q3 x KS x 4 B below 2^31 for this pass).
template <int D, bool TOL>
__device__ __forceinline__ void three_rows(const Two3Args &a, const Lds3 &d, float *lds1, float *lds2, float *lds3,
                                           int x, int y, unsigned rowb, bool own, int zs, int ze, float (&u)[3]) {
    Lv3 s1{}, s2{}, s3{};
    const unsigned nrec = (unsigned)(Q3 * a.KS * 4);
    const int ks4 = (int)(a.KS * 4);
    auto rsrc = [&](const float *base) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base), 0, (int)nrec, 0x00020000);
    };
    auto obz = [&](int zz) {  // planes zs-6 .. ze+1 are asked for; only zs-2 .. ze+1 are used
        zz = min(max(zz, -3), a.nz + 2);
        return a.obst[((long long)zz * a.ny + y) * a.nx + x] != 0;
    };
    float in[Q3];
    auto load = [&](int pl) {
        const auto r = rsrc(a.fin + (long long)pl * a.PL);
#pragma unroll
        for (int k = 0; k < Q3; ++k) in[k] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)rowb, k * ks4, 0));
    };
    bool ob1 = obz(zs - 4), ob2 = obz(zs - 5), ob3 = obz(zs - 6);
    load(zs - 3);
    // P-ring slots (planes mod 3): level L publishes plane j - L + 1 and reads
    // plane j - L - 1 of input plane j
    int sj = (((zs - 3) % 3) + 3) % 3;  // slot of plane j
    auto plane = [&](auto PC, int j) __attribute__((always_inline)) {
        constexpr int P = decltype(PC)::value;
        const int sm1 = sj == 0 ? 2 : sj - 1, sm2 = sj == 2 ? 0 : sj + 1;  // slots of j - 1, j - 2 (j - 3: sj)
        if constexpr (D >= 1) {
            ob3 = ob2;
            ob2 = ob1;
            ob1 = obz(j - 1);
        }
        float o1[Q3], o2[Q3], o3[Q3];
        const float v1 = level3p<P, 1, D, TOL>(in, o1, lds1, sj, sm2, s1, d, ob1, a);
        if (D == 3 && own && j - 1 >= zs && j - 1 < ze) u[0] += v1;
        load(min(j + 1, ze + 2));
        const float v2 = level3p<P, 2, D, TOL>(o1, o2, lds2, sm1, sj, s2, d, ob2, a);
        if (D == 3 && own && j - 2 >= zs && j - 2 < ze) u[1] += v2;
        const float v3 = level3p<P, 3, D, TOL>(o2, o3, lds3, sm2, sm1, s3, d, ob3, a);
        if constexpr (D == 3) {
            if (own && j - 3 >= zs && j - 3 < ze) {
                u[2] += v3;
                const auto r = rsrc(a.fout + (long long)(j - 3) * a.PL);
#pragma unroll
                // plain (temporal) stores: x-neighbouring blocks run on one XCD
                // and each writes a 232-B unaligned row segment, which the L2
                // merges into whole lines before they leave (non-temporal
                // stores: 2.11-2.30 vs 2.07 ms per step at 512^3 tolerance,
                // profiles/r06/d3store/)
                for (int k = 0; k < Q3; ++k) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(o3[k]), r, (int)rowb, k * ks4, 0);
            }
        }
        sj = sj == 2 ? 0 : sj + 1;
    };
    int j = zs - 3;
    for (; j + 1 <= ze + 2; j += 2) {
        plane(std::integral_constant<int, 0>{}, j);
        plane(std::integral_constant<int, 1>{}, j + 1);
    }
    if (j <= ze + 2) plane(std::integral_constant<int, 0>{}, j);
}

// SKIP: rows no later level reads skip the collision (level 1: rows 1..10,
// level 2: 2..9, level 3: 3..8 live) -- each wave runs the plane loop
// instantiated for its row's live depth.
template <bool TOL, bool SKIP>
__global__ __launch_bounds__(T3W *T3TH) void step3d_three(Two3Args a) {
    __shared__ float lds1[T3LDS], lds2[T3LDS], lds3[T3LDS];
    __shared__ float red[3][T3TH];
    const int lane = threadIdx.x, wy = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const Blk3 B = blk3_remap();
    const int ox = B.x * T3OX3, oy = B.y * T3OY3;
    const int x = (((ox - 3 + lane) % a.nx) + a.nx) % a.nx;
    const int y = (((oy - 3 + wy) % a.ny) + a.ny) % a.ny;
    const bool own = lane >= 3 && lane < T3W - 3 && wy >= 3 && wy < T3TH - 3 && ox + lane - 3 < a.nx &&
                     oy + wy - 3 < a.ny;
    const int zs = a.z0 + B.z * a.seg, ze = min(zs + a.seg, a.zn);
    const unsigned rowb = (unsigned)(y * a.px + x) * 4u;  // byte offset of the lane's cell in a speed plane
    const Lds3 d = lds3_offsets(lane, wy);
    float u[3] = {0.f, 0.f, 0.f};
    const int depth = SKIP ? min(min(wy, T3TH - 1 - wy), 3) : 3;  // wave-uniform
    switch (depth) {
        case 0: three_rows<0, TOL>(a, d, lds1, lds2, lds3, x, y, rowb, own, zs, ze, u); break;
        case 1: three_rows<1, TOL>(a, d, lds1, lds2, lds3, x, y, rowb, own, zs, ze, u); break;
        case 2: three_rows<2, TOL>(a, d, lds1, lds2, lds3, x, y, rowb, own, zs, ze, u); break;
        default: three_rows<3, TOL>(a, d, lds1, lds2, lds3, x, y, rowb, own, zs, ze, u); break;
    }
    fold_levels(u, red, lane, wy, a.partials, a.nblocks, a.blk0 + (B.z * gridDim.y + B.y) * gridDim.x + B.x);
}

__global__ __launch_bounds__(BLOCK) void reduce3d(const float *partials, int n, float *av_local, int t) {
    __shared__ float lds[BLOCK / 64];
    const float v = sum_partials_n<BLOCK>(partials, n, lds);
    if (threadIdx.x == 0) av_local[t] = v;
}

// every plane (ghosts included) at rest equilibrium
__global__ __launch_bounds__(BLOCK) void init3d(float *base, long long planes, long long KS, long long PL, float c0,
                                               float c1, float c2) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= planes * KS) return;
    const long long z = i / KS, r = i - z * KS;
    float *d = base + z * PL + r;
    d[0] = c0;
#pragma unroll
    for (int k = 1; k < Q3; ++k) d[k * KS] = (k <= 4 || k == 9 || k == 14) ? c1 : c2;
}

// AoS [nzs][ny][nx][19] staging <-> lattice interior: where cell i of the
// staging array lies in the lattice (speed 0; floats from its origin)
__device__ __forceinline__ long long cell_offset3(long long i, long long PL, int px, int nx, int ny) {
    const long long zy = i / nx;
    const int x = (int)(i - zy * nx);
    const int y = (int)(zy % ny);
    const long long z = zy / ny;
    return z * PL + (long long)y * px + x;
}

__global__ __launch_bounds__(BLOCK) void aos_to_soa3d(const float *aos, float *f, long long PL, long long KS, int px,
                                                     int nx, int ny, long long n) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    float *d = f + cell_offset3(i, PL, px, nx, ny);
#pragma unroll
    for (int k = 0; k < Q3; ++k) d[k * KS] = aos[i * Q3 + k];
}

__global__ __launch_bounds__(BLOCK) void soa_to_aos3d(const float *f, float *aos, long long PL, long long KS, int px,
                                                     int nx, int ny, long long n) {
    const long long i = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const float *s = f + cell_offset3(i, PL, px, nx, ny);
#pragma unroll
    for (int k = 0; k < Q3; ++k) aos[i * Q3 + k] = s[k * KS];
}

// ---- launch wrappers (lbm3d_engine.hpp) ----

// 12 rows without skip, late load (default) or one plane prefetched: the
// instantiations of step3d_two<PD> (see the block constants above)
int two_variant(int th, bool skip, int pd) { return (th == T3TH && !skip && (pd == 0 || pd == 1)) ? pd : -1; }

// grid of an n-step pass: owned tiles of T3OX x T3OY (n = 2) or T3OX3 x T3OY3 (n = 3)
static dim3 pass3d_grid(int n, int nx, int ny, int planes, int seg) {
    const int ox = n == 3 ? T3OX3 : T3OX, oy = n == 3 ? T3OY3 : T3OY;
    return dim3((nx + ox - 1) / ox, (ny + oy - 1) / oy, (planes + seg - 1) / seg);
}

int pass3d_blocks(int n, int nx, int ny, int planes, int seg) {
    const dim3 g = pass3d_grid(n, nx, ny, planes, seg);
    return (int)(g.x * g.y * g.z);
}

hipError_t launch_step3d_two(const Two3Args &a, int variant, bool tol, hipStream_t s) {
    if (a.zn <= a.z0) return hipSuccess;
    const dim3 g = pass3d_grid(2, a.nx, a.ny, a.zn - a.z0, a.seg), b(T3W, T3TH);
    if (tol)  // the default load schedule only (late load)
        hipLaunchKernelGGL((step3d_two<0, true>), g, b, 0, s, a);
    else if (variant == 0)
        hipLaunchKernelGGL((step3d_two<0>), g, b, 0, s, a);
    else if (variant == 1)
        hipLaunchKernelGGL((step3d_two<1>), g, b, 0, s, a);
    else
        return hipErrorInvalidValue;  // no such instantiation (create rejects it)
    return hipGetLastError();
}

hipError_t launch_step3d_three(const Two3Args &a, bool tol, bool skip, hipStream_t s) {
    if (a.zn <= a.z0) return hipSuccess;
    const dim3 g = pass3d_grid(3, a.nx, a.ny, a.zn - a.z0, a.seg), b(T3W, T3TH);
    void (*const kernel[2][2])(Two3Args) = {{step3d_three<false, false>, step3d_three<false, true>},
                                            {step3d_three<true, false>, step3d_three<true, true>}};
    hipLaunchKernelGGL(kernel[tol][skip], g, b, 0, s, a);
    return hipGetLastError();
}

hipError_t launch_reduce3d(const float *partials, int n, float *av_local, int t, hipStream_t s) {
    hipLaunchKernelGGL(reduce3d, dim3(1), dim3(BLOCK), 0, s, partials, n, av_local, t);
    return hipGetLastError();
}

int step3d_blocks(int nx, int ny, int planes, bool pair, int zb) {
    if (pair) return ((nx + 2 * B3X - 1) / (2 * B3X)) * ((ny + B3Y - 1) / B3Y) * ((std::max(planes, 0) + zb - 1) / zb);
    return ((nx + B3X - 1) / B3X) * ((ny + B3Y - 1) / B3Y) * std::max(planes, 0);
}

hipError_t launch_step3d(const Step3Args &a, int planes, bool pair, int zb, bool nt, hipStream_t s) {
    if (planes <= 0) return hipSuccess;
    if (pair) {
        dim3 grid((a.nx + 2 * B3X - 1) / (2 * B3X), (a.ny + B3Y - 1) / B3Y, (planes + zb - 1) / zb);
        auto k = zb == 1 ? (nt ? step3d_pair<1, true> : step3d_pair<1, false>)
               : zb == 2 ? (nt ? step3d_pair<2, true> : step3d_pair<2, false>)
               : zb == 8 ? (nt ? step3d_pair<8, true> : step3d_pair<8, false>)
                         : (nt ? step3d_pair<4, true> : step3d_pair<4, false>);
        hipLaunchKernelGGL(k, grid, dim3(B3X, B3Y), 0, s, a, planes);
    } else {
        dim3 grid((a.nx + B3X - 1) / B3X, (a.ny + B3Y - 1) / B3Y, planes);
        hipLaunchKernelGGL(step3d, grid, dim3(B3X, B3Y), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_init3d(float *base, long long planes, long long KS, long long PL, float c0, float c1, float c2,
                         hipStream_t s) {
    hipLaunchKernelGGL(init3d, dim3((unsigned)((planes * KS + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, base, planes, KS,
                       PL, c0, c1, c2);
    return hipGetLastError();
}

hipError_t launch_aos_to_soa3d(const float *aos, float *f, long long PL, long long KS, int px, int nx, int ny,
                               long long n, hipStream_t s) {
    hipLaunchKernelGGL(aos_to_soa3d, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, aos, f, PL, KS, px,
                       nx, ny, n);
    return hipGetLastError();
}

hipError_t launch_soa_to_aos3d(const float *f, float *aos, long long PL, long long KS, int px, int nx, int ny,
                               long long n, hipStream_t s) {
    hipLaunchKernelGGL(soa_to_aos3d, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, f, aos, PL, KS, px,
                       nx, ny, n);
    return hipGetLastError();
}

}  // namespace lbm
