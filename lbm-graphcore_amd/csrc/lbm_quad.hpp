// lbm_quad.hpp -- what the diagnostics kernels of both engines share on the
// device: the read of four consecutive cells of a row by one lane, and the
// fixed-order fold of a block's statistics.  The views the kernels' argument
// blocks address a lattice through are in lbm_views.hpp.
//
// The access path.  The interior row start is 16-B aligned in every lattice
// layout (D2Q9: xoff, plane and pitch are multiples of 4 floats; D3Q19: px is
// a multiple of 16 floats, KS and PL multiples of 4), so a lane whose x is a
// multiple of 4 reads its four cells with Q 16-B loads (load_quad) and picks
// cell i out of them (quad_cell).  The four map bytes of the quad are one
// aligned word when the map's row length is a multiple of 4, else four byte
// loads (quad_map_bytes).  Cells that do not fill a quad -- the last w % 4 of
// a row, boxes off the alignment -- are read one at a time (load_cell).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lbm_views.hpp"

namespace lbm {

// The Q populations of four consecutive cells from src (16-B aligned).  Two
// forms of the same Q addresses: indexed (src + k * speed_stride), or WALK, the
// pointer stepping from speed to speed.  They differ only in the registers the
// compiler spends on the addresses.  The rule: D3Q19 walks, D2Q9 indexes, and
// a kernel that measures better with the other form says so at its call
// (figures: profiles/diag_refactor/README.md).
template <int Q, bool WALK = (Q > 9)>
__device__ __forceinline__ void load_quad(const float *src, long long speed_stride, float4 (&v)[Q]) {
    if (WALK) {
#pragma unroll
        for (int k = 0; k < Q; ++k, src += speed_stride) v[k] = *reinterpret_cast<const float4 *>(src);
    } else {
#pragma unroll
        for (int k = 0; k < Q; ++k) v[k] = *reinterpret_cast<const float4 *>(src + k * speed_stride);
    }
}

// the quad's four map bytes, byte i in bits 8 i .. 8 i + 7
__device__ __forceinline__ unsigned quad_map_bytes(const uint8_t *ob, bool word_aligned) {
    if (word_aligned) return *reinterpret_cast<const unsigned *>(ob);
    return (unsigned)ob[0] | ((unsigned)ob[1] << 8) | ((unsigned)ob[2] << 16) | ((unsigned)ob[3] << 24);
}

// cell i (a constant after unrolling) of a loaded quad
template <int Q>
__device__ __forceinline__ void quad_cell(const float4 (&v)[Q], int i, float (&c)[Q]) {
#pragma unroll
    for (int k = 0; k < Q; ++k) c[k] = i == 0 ? v[k].x : i == 1 ? v[k].y : i == 2 ? v[k].z : v[k].w;
}

// value i (0..3) of a loaded quad
__device__ __forceinline__ float pick(const float4 &v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

// the Q populations of the single cell src + i
template <int Q>
__device__ __forceinline__ void load_cell(const float *src, long long speed_stride, int i, float (&c)[Q]) {
#pragma unroll
    for (int k = 0; k < Q; ++k) c[k] = src[k * speed_stride + i];
}

// Fold of a block's per-lane sums and maxima in a fixed order, which is what
// makes the statistics reproducible: the lanes of a wave by shuffle from 32
// down to 1, lane 0 of each wave to LDS, then thread 0 takes the WAVES waves in
// index order and writes sum_part[j * blocks + block] / max_part[j * blocks + block].
template <int WAVES, int NS, int NM>
__device__ __forceinline__ void fold_block(double (&s)[NS], float (&m)[NM], long long block, long long blocks,
                                           double *sum_part, float *max_part) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int j = 0; j < NS; ++j) s[j] += __shfl_down(s[j], off, 64);
#pragma unroll
        for (int j = 0; j < NM; ++j) m[j] = fmaxf(m[j], __shfl_down(m[j], off, 64));
    }
    __shared__ double ws[NS][WAVES];
    __shared__ float wm[NM][WAVES];
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) ws[j][threadIdx.x >> 6] = s[j];
#pragma unroll
        for (int j = 0; j < NM; ++j) wm[j][threadIdx.x >> 6] = m[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            double t = ws[j][0];
            for (int i = 1; i < WAVES; ++i) t += ws[j][i];
            sum_part[j * blocks + block] = t;
        }
#pragma unroll
        for (int j = 0; j < NM; ++j) {
            float t = wm[j][0];
            for (int i = 1; i < WAVES; ++i) t = fmaxf(t, wm[j][i]);
            max_part[j * blocks + block] = t;
        }
    }
}

}  // namespace lbm
