// lbm_binned.hip -- sums of per-cell quantities over rectangular bins of the
// D2Q9 engine's current lattice (the lbm_* functions of
// include/lbm_binned_hip.h), and the second pass both engines share.  The
// kernels, then the engine's host side.
//
// First pass (binned_sums): one memory-bound pass over the nine populations of
// the current side of the pair, 37 B read per cell, by the access path of
// lbm_quad.hpp: a lane takes four consecutive cells of a row (nine 16-B loads),
// a wave 256 columns; the last w % 4 cells of a row go one at a time.  A wave
// walks one chunk -- at most BN_CHUNK rows inside one bin -- with the fp64 sums
// of its four columns in registers, then folds along x by bin (fold_x,
// lbm_binned.hpp) and stores one partial per bin it touches.  Nothing goes
// through LDS and no wave waits for another.
//
// Second pass (fold_bins): one thread per (field, bin) adds the bin's partials
// in ascending (chunk, row, wave) order and writes the sub-domain's bin array;
// only that array crosses to the host.  Launches of few bins with many
// partials each take a wave per (field, bin) instead (fold_bins_wave).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "lbm_binned.hpp"
#include "lbm_binned_hip.h"
#include "lbm_engine.hpp"
#include "lbm_quad.hpp"

namespace lbm {
namespace binned {

// of the view the kernel reads o, obst, plane, pitch, w and h (sp and obst_pressure ride along unused)
struct Bin2Args : LatticeView {
    Axis x;
    ChunkAxis y;
    int nwx, nslots;       // waves along x; partial slots of a chunk
    double *part[BN_FIELDS2];  // [chunks][nslots] per requested field, else null
};

__global__ __launch_bounds__(BN_BLOCK) void binned_sums(Bin2Args a) {
    const long long item = (long long)blockIdx.x * (BN_BLOCK / 64) + (threadIdx.x >> 6);
    if (item >= (long long)a.y.chunks() * a.nwx) return;  // wave-uniform: the block never synchronises
    const int chunk = (int)(item / a.nwx), wx = (int)(item - (long long)chunk * a.nwx);
    int r0, r1;
    a.y.chunk_range(chunk, r0, r1);
    if (r0 >= r1) return;
    const int lane = threadIdx.x & 63;
    const int x = wx * BN_WAVE_COLS + lane * BN_QUAD;
    const bool obst_word = (a.w & 3) == 0;  // every quad's four obstacle bytes are one aligned word
    double s[BN_QUAD][BN_FIELDS2];
    int key[BN_QUAD];
#pragma unroll
    for (int i = 0; i < BN_QUAD; ++i) {
        key[i] = x + i < a.w ? (a.x.g0 + x + i) / a.x.bsz : KEY_NONE;
#pragma unroll
        for (int f = 0; f < BN_FIELDS2; ++f) s[i][f] = 0.0;
    }
    if (x + BN_QUAD <= a.w) {
        for (int y = r0; y < r1; ++y) {
            const float *src = a.o + (long long)y * a.pitch + x;
            const uint8_t *ob = a.obst + (long long)y * a.w + x;
            float4 v[Q];
            load_quad<Q>(src, a.plane, v);
            const unsigned bits = quad_map_bytes(ob, obst_word);
#pragma unroll
            for (int i = 0; i < BN_QUAD; ++i) {
                float c[Q];
                quad_cell<Q>(v, i, c);
                add_cell2(c, ((bits >> (8 * i)) & 0xffu) != 0, s[i]);
            }
        }
    } else if (x < a.w) {
        // ragged tail of a row: the last w % 4 cells, one at a time
        for (int y = r0; y < r1; ++y) {
            const float *src = a.o + (long long)y * a.pitch + x;
            const uint8_t *ob = a.obst + (long long)y * a.w + x;
#pragma unroll
            for (int i = 0; i < BN_QUAD - 1; ++i) {
                if (x + i >= a.w) break;
                float c[Q];
                load_cell<Q>(src, a.plane, i, c);
                add_cell2(c, ob[i] != 0, s[i]);
            }
        }
    }
    fold_x<BN_QUAD, BN_FIELDS2>(s, key, a.x.bsz > 1, wx - a.x.b_lo, (long long)chunk * a.nslots, a.part);
}

__global__ __launch_bounds__(BN_BLOCK) void fold_bins(FoldArgs a) {
    const long long nb = (long long)a.c.a.nbl * a.r.nbl * a.x.nbl;
    const long long t = (long long)blockIdx.x * BN_BLOCK + threadIdx.x;
    if (t >= nb * a.want) return;
    const int n = (int)(t / nb);
    const long long b = t - n * nb;
    const int bxl = (int)(b % a.x.nbl);
    const int brl = (int)((b / a.x.nbl) % a.r.nbl);
    const int bcl = (int)(b / ((long long)a.x.nbl * a.r.nbl));
    int xs, xe, rs, re;
    a.x.bin_range(bxl, xs, xe);
    a.r.bin_range(brl, rs, re);
    const int w_lo = xs / a.wave_cols, w_hi = (xe - 1) / a.wave_cols;
    const double *part = a.part[n];
    double sum = 0.0;
    for (int c = 0; c < a.c.cpb; ++c) {
        const int chunk = bcl * a.c.cpb + c;
        int lo, hi;
        a.c.chunk_range(chunk, lo, hi);
        if (lo >= hi) continue;
        for (int r = rs; r < re; ++r) {
            const double *p = part + ((long long)chunk * a.r.len + r) * a.nslots + bxl;
#pragma unroll 8
            for (int w = w_lo; w <= w_hi; ++w) sum += p[w];
        }
    }
    a.out[n][b] = sum;
}

// The same sums with a wave per (field, bin), for launches of few bins with
// many partials each (domain totals: 8192 partials in one bin at 8192^2).  Lane
// l adds the bin's (chunk, row) pairs l, l + 64, ... in ascending order, each
// over its waves; the lanes then fold by shuffle, again in a fixed order.
__global__ __launch_bounds__(BN_BLOCK) void fold_bins_wave(FoldArgs a) {
    const long long nb = (long long)a.c.a.nbl * a.r.nbl * a.x.nbl;
    const long long t = (long long)blockIdx.x * (BN_BLOCK / 64) + (threadIdx.x >> 6);
    if (t >= nb * a.want) return;  // wave-uniform
    const int n = (int)(t / nb);
    const long long b = t - n * nb;
    const int bxl = (int)(b % a.x.nbl);
    const int brl = (int)((b / a.x.nbl) % a.r.nbl);
    const int bcl = (int)(b / ((long long)a.x.nbl * a.r.nbl));
    int xs, xe, rs, re;
    a.x.bin_range(bxl, xs, xe);
    a.r.bin_range(brl, rs, re);
    const int w_lo = xs / a.wave_cols, w_hi = (xe - 1) / a.wave_cols;
    const int nr = re - rs, pairs = a.c.cpb * nr;
    const double *part = a.part[n];
    double sum = 0.0;
    for (int j = threadIdx.x & 63; j < pairs; j += 64) {
        const int c = j / nr, r = rs + (j - c * nr);
        const int chunk = bcl * a.c.cpb + c;
        int lo, hi;
        a.c.chunk_range(chunk, lo, hi);
        if (lo >= hi) continue;
        const double *p = part + ((long long)chunk * a.r.len + r) * a.nslots + bxl;
        for (int w = w_lo; w <= w_hi; ++w) sum += p[w];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) a.out[n][b] = sum;
}

// a wave per bin pays where every bin has at least FOLD_WAVE_PAIRS (chunk, row)
// pairs and the launch has too few bins to fill the device with threads
constexpr int FOLD_WAVE_PAIRS = 64, FOLD_WAVE_MAX_BINS = 1024;

hipError_t launch_fold_bins(const FoldArgs &a, hipStream_t s) {
    const long long items = (long long)a.c.a.nbl * a.r.nbl * a.x.nbl * a.want;
    const long long pairs = (long long)a.c.cpb * std::min(a.r.bsz, a.r.len);
    if (pairs >= FOLD_WAVE_PAIRS && items <= FOLD_WAVE_MAX_BINS) {
        const long long blocks = (items + BN_BLOCK / 64 - 1) / (BN_BLOCK / 64);
        hipLaunchKernelGGL(fold_bins_wave, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    } else {
        hipLaunchKernelGGL(fold_bins, dim3((unsigned)((items + BN_BLOCK - 1) / BN_BLOCK)), dim3(BN_BLOCK), 0, s, a);
    }
    return hipGetLastError();
}

hipError_t launch_binned_sums(const Bin2Args &a, hipStream_t s) {
    const long long waves = (long long)a.y.chunks() * a.nwx;
    const long long blocks = (waves + BN_BLOCK / 64 - 1) / (BN_BLOCK / 64);
    hipLaunchKernelGGL(binned_sums, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace binned
}  // namespace lbm

// ---- D2Q9 engine: host side ----

// The LBM_BIN_* sums of the current lattice into planar host arrays
// double[nby][nbx] over the full bin grid.  A NULL entry is neither staged nor
// copied.  Per sub-domain: first pass, second pass, the sub-domain's bin array
// to the host, added there into the bins it touches -- sub-domain after
// sub-domain, so a bin that spans several is summed in their order.
void lbm_handle::store_binned(int bw, int bh, double *const *out) {
    using namespace lbm::binned;
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take binned sums of");
    lbm::binned::check_bins(p.nx, p.ny, 1, bw, bh, 1);
    const int want = count_wanted(out, LBM_BIN_FIELDS);
    if (want == 0) return;
    const int nbx = LBM_BIN_COUNT(p.nx, bw), nby = LBM_BIN_COUNT(p.ny, bh);
    for (int i = 0; i < LBM_BIN_FIELDS; ++i)
        if (out[i]) std::fill(out[i], out[i] + (size_t)nbx * nby, 0.0);
    sync_all();
    prof_drop();
    for (auto &s : subs) {
        set_device(s);
        Bin2Args a{lattice_view(s)};
        a.x = make_axis(s.rect.x0, s.w, bw);
        a.y = make_chunk_axis(s.rect.y0, s.h, bh);
        a.nwx = (s.w + BN_WAVE_COLS - 1) / BN_WAVE_COLS;
        a.nslots = a.nwx + a.x.nbl - 1;
        if ((long long)a.y.chunks() * a.nwx > (1LL << 32))
            throw lbm_failure(LBM_E_INVALID, "sub-domain too large for binned sums");
        const PartBins<LBM_BIN_FIELDS> pb(a.x, a.y, Axis{0, 1, 1, 0, 1}, 1, BN_WAVE_COLS, a.nslots, out);
        std::copy(pb.part, pb.part + LBM_BIN_FIELDS, a.part);
        timed(s, s.s_comp, "binned_sums", [&] { HIP_CHECK(launch_binned_sums(a, s.s_comp)); });
        timed(s, s.s_comp, "binned_sums fold", [&] { HIP_CHECK(launch_fold_bins(pb.fa, s.s_comp)); });
        pb.add_to(s.s_comp, out, nbx, 1);
    }
    prof_collect();
}

// Fluid cells per bin over the local sub-domains, from their obstacle maps (a
// copy to the host, no launch).
void lbm_handle::bin_fluid_cells(int bw, int bh, int64_t *count) {
    lbm::binned::check_bins(p.nx, p.ny, 1, bw, bh, 1);
    if (!count) return;
    const int nbx = LBM_BIN_COUNT(p.nx, bw), nby = LBM_BIN_COUNT(p.ny, bh);
    std::fill(count, count + (size_t)nbx * nby, (int64_t)0);
    sync_all();
    for (auto &s : subs) {
        set_device(s);
        std::vector<uint8_t> ob((size_t)s.w * s.h);
        HIP_CHECK(hipMemcpy(ob.data(), s.obst, ob.size(), hipMemcpyDeviceToHost));
        for (int y = 0; y < s.h; ++y) {
            int64_t *row = count + (size_t)((s.rect.y0 + y) / bh) * nbx;
            const uint8_t *o = ob.data() + (size_t)y * s.w;
            for (int x = 0; x < s.w; ++x) row[(s.rect.x0 + x) / bw] += o[x] ? 0 : 1;
        }
    }
}
