// lbm_forces.hpp -- wall list and kernels of the momentum-exchange wall forces
// (include/lbm_forces_hip.h), shared by the D2Q9 engine (lbm_forces.hip) and
// the D3Q19 engine (lbm3d_forces.hip).
//
// Only wall cells (blocked cells with a fluid neighbour) carry force, so the
// hot path is a gather over a compact list: per wall cell the offset of its
// speed-0 population from the lattice origin (the same for both lattices of a
// ping-pong pair), its link mask and its index in the planar map.  The list is
// built on the host from the ghosted obstacle map at the first force call and
// lives on the device; with bodies set it is sorted by body (row-major inside
// a body, unlabelled cells last) and every body's range is cut into chunks of
// at most BODY_CHUNK cells.
//
// The kernels are templates over the lattice model (a class with
// force(p, ks, mask, fx, fy, fz): the expressions of lbm_forces_hip.h from the
// populations p[j * ks], loads gated by the link bits); each engine's .hip
// instantiates them for its model.  One lane per wall cell.  Sums are fp64 of
// the fp32 per-cell values: lanes of a wave by shuffle, a block's waves
// through LDS, per-block partials folded by the host in block order.  Per-body
// sums: one wave per chunk; a body of one chunk is finished by that wave, the
// chunk sums of a larger body are folded by one wave of a second launch (lane
// l takes chunks l, l + 64, ...).  No atomics, and the chunking depends only on
// the list: the same lattice always gives the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace lbm {
namespace forces {

constexpr int WBLOCK = 256;             // 4 wave64s
constexpr int WALL_MAX_BLOCKS = 1024;   // grid-stride beyond: also the most partials folded per list
constexpr int BODY_MAX_BLOCKS = 8192;   // one wave per chunk (or large body), wave-stride beyond
constexpr unsigned BODY_CHUNK = 512;    // most cells a wave sums: 8 per lane
constexpr unsigned BODY_WHOLE = 0x80000000u;  // chunk flag: the chunk is its body's only one

struct WallArgs {
    const float *o;          // lattice origin (current side of the pair)
    long long ks;            // stride between a cell's populations (floats)
    const long long *off;    // [n] offset of population 0 from o
    const unsigned *mask;    // [n] link bits: bit j-1 = link j
    const unsigned *cell;    // [n] index in the planar map
    long long n;
    double *part;            // total: [blocks][3] fp64 partial sums
    long long *lpart;        // total: [blocks] link counts
    float *mx, *my, *mz;     // map: zeroed planar staging arrays (null: not written)
    const unsigned *cs;      // bodies: [nc + 1] list range of each chunk
    const unsigned *cbody;   // bodies: [nc] body of the chunk (| BODY_WHOLE)
    int nc;
    double *csum;            // bodies: [nc][3] sums of the chunks of larger bodies
    long long *clinks;       // bodies: [nc]
    const unsigned *mtab;    // bodies: [nm][3] {body, first chunk, end chunk} of the bodies of several chunks
    int nm;
    int nbodies;
    double *bsum;            // bodies: [nbodies][3], zeroed before the first launch
    long long *blinks;       // bodies: [nbodies]
};

// fixed-order sum over the 64 lanes of a wave: the result is in lane 0
__device__ __forceinline__ void wave_sum(double &x, double &y, double &z, long long &links) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        x += __shfl_down(x, d, 64);
        y += __shfl_down(y, d, 64);
        z += __shfl_down(z, d, 64);
        links += __shfl_down(links, d, 64);
    }
}

template <class M>
__global__ __launch_bounds__(WBLOCK) void wall_force_total(WallArgs a) {
    double sx = 0.0, sy = 0.0, sz = 0.0;
    long long links = 0;
    for (long long i = (long long)blockIdx.x * WBLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * WBLOCK) {
        const unsigned m = a.mask[i];
        float fx, fy, fz;
        M::force(a.o + a.off[i], a.ks, m, fx, fy, fz);
        sx += (double)fx;
        sy += (double)fy;
        sz += (double)fz;
        links += __popc(m);
    }
    wave_sum(sx, sy, sz, links);
    __shared__ double w[WBLOCK / 64][3];
    __shared__ long long wl[WBLOCK / 64];
    if ((threadIdx.x & 63) == 0) {
        w[threadIdx.x >> 6][0] = sx;
        w[threadIdx.x >> 6][1] = sy;
        w[threadIdx.x >> 6][2] = sz;
        wl[threadIdx.x >> 6] = links;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long l = wl[0];
        for (int i = 1; i < WBLOCK / 64; ++i) {
            w[0][0] += w[i][0];
            w[0][1] += w[i][1];
            w[0][2] += w[i][2];
            l += wl[i];
        }
        a.part[3 * blockIdx.x + 0] = w[0][0];
        a.part[3 * blockIdx.x + 1] = w[0][1];
        a.part[3 * blockIdx.x + 2] = w[0][2];
        a.lpart[blockIdx.x] = l;
    }
}

// one wave per chunk: lane l takes cells l, l + 64, ... of the chunk's range
template <class M>
__global__ __launch_bounds__(WBLOCK) void wall_force_chunks(WallArgs a) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (WBLOCK / 64);
    for (long long c = (long long)blockIdx.x * (WBLOCK / 64) + (threadIdx.x >> 6); c < a.nc; c += waves) {
        const unsigned end = a.cs[c + 1];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        long long links = 0;
        for (unsigned i = a.cs[c] + lane; i < end; i += 64) {
            const unsigned m = a.mask[i];
            float fx, fy, fz;
            M::force(a.o + a.off[i], a.ks, m, fx, fy, fz);
            sx += (double)fx;
            sy += (double)fy;
            sz += (double)fz;
            links += __popc(m);
        }
        wave_sum(sx, sy, sz, links);
        if (lane == 0) {
            const unsigned cb = a.cbody[c];
            const bool whole = (cb & BODY_WHOLE) != 0;
            double *d = whole ? a.bsum + 3 * (size_t)(cb & ~BODY_WHOLE) : a.csum + 3 * (size_t)c;
            d[0] = sx;
            d[1] = sy;
            d[2] = sz;
            (whole ? a.blinks[cb & ~BODY_WHOLE] : a.clinks[c]) = links;
        }
    }
}

// one wave per body of several chunks: lane l takes chunk sums l, l + 64, ...
// (a template only so that each engine's unit carries its own copy)
template <class M>
__global__ __launch_bounds__(WBLOCK) void wall_force_fold_chunks(WallArgs a) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (WBLOCK / 64);
    for (long long m = (long long)blockIdx.x * (WBLOCK / 64) + (threadIdx.x >> 6); m < a.nm; m += waves) {
        const unsigned b = a.mtab[3 * m], end = a.mtab[3 * m + 2];
        double sx = 0.0, sy = 0.0, sz = 0.0;
        long long links = 0;
        for (unsigned c = a.mtab[3 * m + 1] + lane; c < end; c += 64) {
            sx += a.csum[3 * (size_t)c + 0];
            sy += a.csum[3 * (size_t)c + 1];
            sz += a.csum[3 * (size_t)c + 2];
            links += a.clinks[c];
        }
        wave_sum(sx, sy, sz, links);
        if (lane == 0) {
            a.bsum[3 * (size_t)b + 0] = sx;
            a.bsum[3 * (size_t)b + 1] = sy;
            a.bsum[3 * (size_t)b + 2] = sz;
            a.blinks[b] = links;
        }
    }
}

template <class M>
__global__ __launch_bounds__(WBLOCK) void wall_force_map(WallArgs a) {
    for (long long i = (long long)blockIdx.x * WBLOCK + threadIdx.x; i < a.n; i += (long long)gridDim.x * WBLOCK) {
        float fx, fy, fz;
        M::force(a.o + a.off[i], a.ks, a.mask[i], fx, fy, fz);
        const unsigned c = a.cell[i];
        if (a.mx) a.mx[c] = fx;
        if (a.my) a.my[c] = fy;
        if (a.mz) a.mz[c] = fz;
    }
}

enum Kind : int { WALL_TOTAL = 0, WALL_BODIES = 1, WALL_MAP = 2 };

inline int wall_blocks(long long n) {
    const long long b = (n + WBLOCK - 1) / WBLOCK;
    return (int)(b < 1 ? 1 : b > WALL_MAX_BLOCKS ? WALL_MAX_BLOCKS : b);
}
inline int body_blocks(int waves) {
    const long long b = ((long long)waves + WBLOCK / 64 - 1) / (WBLOCK / 64);
    return (int)(b < 1 ? 1 : b > BODY_MAX_BLOCKS ? BODY_MAX_BLOCKS : b);
}

template <class M>
hipError_t launch_wall(const WallArgs &a, int kind, hipStream_t s) {
    if (kind == WALL_TOTAL)
        hipLaunchKernelGGL(wall_force_total<M>, dim3(wall_blocks(a.n)), dim3(WBLOCK), 0, s, a);
    else if (kind == WALL_BODIES) {
        // (bsum / blinks zeroed by the caller: WallList::launch)
        if (a.nc > 0) hipLaunchKernelGGL(wall_force_chunks<M>, dim3(body_blocks(a.nc)), dim3(WBLOCK), 0, s, a);
        if (a.nm > 0) hipLaunchKernelGGL(wall_force_fold_chunks<M>, dim3(body_blocks(a.nm)), dim3(WBLOCK), 0, s, a);
    } else
        hipLaunchKernelGGL(wall_force_map<M>, dim3(wall_blocks(a.n)), dim3(WBLOCK), 0, s, a);
    return hipGetLastError();
}

// D2Q9 (lbm_forces.hip) and D3Q19 (lbm3d_forces.hip) instantiations
hipError_t launch_wall2d(const WallArgs &a, int kind, hipStream_t s);
hipError_t launch_wall3d(const WallArgs &a, int kind, hipStream_t s);

// One sub-domain's (slab's) wall list: the host copy in row-major order, and
// the device copy in the order of the bodies set last.
struct WallList {
    int dims = 2;
    std::vector<long long> h_off;
    std::vector<unsigned> h_cell, h_mask;
    std::vector<int> h_body;      // per wall cell, -1: no body (empty: no bodies set)
    long long n = 0;
    int nbodies = 0;              // bodies of the device copy (0: row-major order, no chunks)
    long long *off = nullptr;
    unsigned *cell = nullptr, *mask = nullptr;
    unsigned *ctab = nullptr;     // [nc + 1] chunk ranges, [nc] chunk bodies, [nm][3] bodies of several chunks
    int nc = 0, nm = 0;
    double *part = nullptr;       // [wall_blocks(n)][3] doubles, then as many long long
    double *bpart = nullptr;      // [nbodies][3] doubles, nbodies long long, [nc][3] doubles, nc long long

    void add(long long o, unsigned c, unsigned m) {
        h_off.push_back(o);
        h_cell.push_back(c);
        h_mask.push_back(m);
    }
    // (re)build the device copy: sorted by h_body when nb > 0 (the device of the list must be current)
    hipError_t upload(int nb);
    void release();
    WallArgs args(const float *o, long long ks) const;
    // enqueue; the fetch calls synchronise the stream, copy the partials and ADD to the outputs
    hipError_t launch(int kind, const WallArgs &a, hipStream_t s) const;
    hipError_t fetch_total(hipStream_t s, double (&f)[3], long long &links) const;
    hipError_t fetch_bodies(hipStream_t s, double *fx, double *fy, double *fz, int64_t *links) const;
};

}  // namespace forces
}  // namespace lbm
