// lbm_binned.hpp -- what the binned-sum kernels of both engines share
// (lbm_binned.hip, lbm3d_binned.hip; include/lbm_binned_hip.h): the geometry of
// bins, waves and chunks, the per-cell term vectors, the segmented fold of a
// wave's columns along x, the argument block of the second pass, and the host
// side of a pass over one part (bin-size check, staging, copy back).
//
// A launch covers one sub-domain (D2Q9) or slab (D3Q19).  Bins tile the full
// domain from global cell 0, so a sub-domain touches the bins b_lo .. b_lo + nbl
// - 1 of an axis and may own only part of the first and the last.  A wave owns
// `wave_cols` consecutive columns and walks a chunk: at most BN_CHUNK rows
// (D2Q9) or planes (D3Q19) that lie inside one bin.  Each lane keeps fp64 sums
// of its columns in registers; at the end of the chunk the wave folds them
// along x by bin (fold_x) and leaves one partial per bin it touches.  The
// second pass (fold_bins, fold_bins_wave) adds a bin's partials in an order that
// depends on the geometry alone.  No atomics anywhere.
//
// Partials.  A wave's columns and an axis' bins both advance along x, so the
// pairs (wave wx, local bin bxl) that intersect are numbered without gaps that
// matter by slot = wx + bxl < nslots = waves + bins - 1; a slot whose wave and
// bin do not intersect is never written and never read.  Per requested field:
// double[chunks][rows][nslots] with rows = 1 (D2Q9) or ny (D3Q19).
#pragma once

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>
#include <vector>

#include "lbm3d_cell_macro.hpp"
#include "lbm_cell_macro.hpp"
#include "lbm_diag_host.hpp"

namespace lbm {
namespace binned {

constexpr int BN_QUAD = 4;          // D2Q9: consecutive cells of a row a lane takes
constexpr int BN_WAVE_COLS = 256;   // D2Q9: columns of a wave
constexpr int BN3_WAVE_COLS = 64;   // D3Q19: columns of a wave (one cell per lane)
constexpr int BN_CHUNK = 32;        // most rows / planes of a chunk
constexpr int BN_BLOCK = 256;       // four independent waves
constexpr int BN_FIELDS2 = 9, BN_FIELDS3 = 14, BN_MAX_FIELDS = 14;
constexpr int KEY_NONE = INT_MAX;   // bin key of a column beyond the sub-domain

// one axis: the sub-domain owns the global cells [g0, g0 + len), bins are bsz wide
struct Axis {
    int g0, len, bsz;
    int b_lo, nbl;  // first bin touched, bins touched
    // local cells [lo, hi) of local bin bl
    __host__ __device__ void bin_range(int bl, int &lo, int &hi) const {
        const long long b0 = (long long)(b_lo + bl) * bsz;
        const long long s = b0 > g0 ? b0 : g0;
        const long long e = b0 + bsz < (long long)g0 + len ? b0 + bsz : (long long)g0 + len;
        lo = (int)(s - g0);
        hi = (int)(e - g0);
    }
};

inline Axis make_axis(int g0, int len, int bsz) {
    Axis a{g0, len, bsz, g0 / bsz, 0};
    a.nbl = (g0 + len - 1) / bsz - a.b_lo + 1;
    return a;
}

// the axis a wave walks: every bin is cut into cpb chunks of `rows` cells from
// the bin's own first cell, so no chunk straddles a bin; chunk = bl * cpb + c
struct ChunkAxis {
    Axis a;
    int rows, cpb;
    __host__ __device__ int chunks() const { return a.nbl * cpb; }
    // local cells [lo, hi) of a chunk; lo >= hi: the sub-domain owns none of it
    __host__ __device__ void chunk_range(int chunk, int &lo, int &hi) const {
        const int bl = chunk / cpb, c = chunk - bl * cpb;
        const long long b0 = (long long)(a.b_lo + bl) * a.bsz;
        long long s = b0 + (long long)c * rows;
        long long e = s + rows < b0 + a.bsz ? s + rows : b0 + a.bsz;
        if (s < a.g0) s = a.g0;
        if (e > (long long)a.g0 + a.len) e = (long long)a.g0 + a.len;
        lo = (int)(s - a.g0);
        hi = (int)(e - a.g0);
    }
};

inline ChunkAxis make_chunk_axis(int g0, int len, int bsz) {
    ChunkAxis c{make_axis(g0, len, bsz), bsz < BN_CHUNK ? bsz : BN_CHUNK, 0};
    c.cpb = (bsz + c.rows - 1) / c.rows;
    return c;
}

// ---- per-cell term vectors (index order of LBM_BIN_* / LBM3D_BIN_*) ----

// adds the terms of a fluid cell to s; an obstacle cell adds nothing
__device__ __forceinline__ void add_cell2(const float (&c)[9], bool blocked, double (&s)[BN_FIELDS2]) {
    if (blocked) return;
    float rho, jx, jy;
    const CellMacro m = cell_macro<true, true>(c, false, 0.f, rho);
    cell_momentum(c, jx, jy);
    const double ux = (double)m.ux, uy = (double)m.uy;
    s[0] += (double)rho;
    s[1] += (double)jx;
    s[2] += (double)jy;
    s[3] += ux;
    s[4] += uy;
    s[5] += (double)m.u;
    s[6] += ux * ux;
    s[7] += ux * uy;
    s[8] += uy * uy;
}

__device__ __forceinline__ void add_cell3(const float (&c)[19], bool blocked, double (&s)[BN_FIELDS3]) {
    if (blocked) return;
    float rho, jx, jy, jz;
    const Cell3Macro m = cell3_macro<true, true>(c, false, 0.f, rho);
    cell3_momentum(c, jx, jy, jz);
    const double ux = (double)m.ux, uy = (double)m.uy, uz = (double)m.uz;
    s[0] += (double)rho;
    s[1] += (double)jx;
    s[2] += (double)jy;
    s[3] += (double)jz;
    s[4] += ux;
    s[5] += uy;
    s[6] += uz;
    s[7] += (double)m.u;
    s[8] += ux * ux;
    s[9] += ux * uy;
    s[10] += ux * uz;
    s[11] += uy * uy;
    s[12] += uy * uz;
    s[13] += uz * uz;
}

// Fold of a wave's columns along x by bin, and the store of one partial per
// bin the wave touches.  Lane l holds NC consecutive columns (lane-major:
// column = l * NC + i) with sums c[i][] and bin keys key[i], ascending along
// the wave; KEY_NONE marks a column beyond the sub-domain.  Every lane of the
// wave must call it.
//
// scan (wave-uniform; false when bw == 1, where every column is its own bin):
// a segmented inclusive scan keyed by bin.  First inside the lane (NC - 1
// adds), then across the wave over each lane's tail sum -- six __shfl_up steps;
// lane l takes lane l - off's running sum only where all its own columns share
// one key and that key is lane l - off's tail key, which (keys ascend) also
// holds for every lane between -- and last the running sum of lane l - 1 is
// added to the columns that continue its tail bin.
//
// The last column of each bin inside the wave then holds the bin's sum over
// the wave and stores it at part[f][obase + key + slot_off] (slot_off = wave
// index - first bin of the sub-domain).  A null part[f] is not stored.
template <int NC, int NF>
__device__ __forceinline__ void fold_x(double (&c)[NC][NF], const int (&key)[NC], bool scan, int slot_off,
                                       long long obase, double *const *part) {
    const int lane = threadIdx.x & 63;
    const int next0 = __shfl_down(key[0], 1, 64);
    bool last[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int nk = i + 1 < NC ? key[i + 1 < NC ? i + 1 : i] : (lane == 63 ? KEY_NONE : next0);
        last[i] = key[i] != KEY_NONE && nk != key[i];
    }
    if (scan) {
        const int kt = key[NC - 1];
        const bool whole = key[0] == kt;
        bool take[6];
#pragma unroll
        for (int s = 0; s < 6; ++s) {
            const int ko = __shfl_up(kt, 1 << s, 64);
            take[s] = lane >= (1 << s) && whole && ko == kt;
        }
        const int kp = __shfl_up(kt, 1, 64);
        const bool carry = lane > 0 && kp == key[0] && key[0] != KEY_NONE;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
#pragma unroll
            for (int i = 1; i < NC; ++i)
                if (key[i] == key[i - 1]) c[i][f] = c[i - 1][f] + c[i][f];
            double run = c[NC - 1][f];
#pragma unroll
            for (int s = 0; s < 6; ++s) {
                const double o = __shfl_up(run, 1 << s, 64);
                if (take[s]) run = o + run;
            }
            const double prev = __shfl_up(run, 1, 64);
            if (carry) {
#pragma unroll
                for (int i = 0; i < NC; ++i)
                    if (key[i] == key[0]) c[i][f] = prev + c[i][f];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        if (!last[i]) continue;
        const long long at = obase + (key[i] + slot_off);
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (part[f]) part[f][at] = c[i][f];
    }
}

// second pass: one thread (or, for few bins of many partials, one wave) per
// (requested field, local bin) adds the bin's partials and writes
// out[n][(bcl * r.nbl + brl) * x.nbl + bxl]
struct FoldArgs {
    Axis x;            // columns; wave_cols columns per wave
    ChunkAxis c;       // the walked axis: y (D2Q9), z (D3Q19)
    Axis r;            // rows of a plane (D3Q19 y); D2Q9: one row, one bin
    int wave_cols, nslots, want;
    const double *part[BN_MAX_FIELDS];  // requested fields, packed: [chunks][r.len][nslots]
    double *out[BN_MAX_FIELDS];         // [c.nbl][r.nbl][x.nbl]
};

hipError_t launch_fold_bins(const FoldArgs &a, hipStream_t s);  // lbm_binned.hip

// ---- host side of a binned pass over one part (a sub-domain, a slab) ----
// Shared by the flow's binned sums and the scalar transport sums (lbm_transport.hip, lbm3d_transport.hip).

// bin sizes must lie in 1..n along each axis (an engine without z passes nz = bd = 1)
inline void check_bins(int nx, int ny, int nz, int bw, int bh, int bd) {
    if (bw < 1 || bw > nx || bh < 1 || bh > ny || bd < 1 || bd > nz)
        throw lbm_failure(LBM_E_INVALID, "bin sizes must lie in 1..n along every axis");
}

// The staging of one part on the current device, held until it leaves scope: per requested field (out[f]
// non-NULL, f < NF) the first pass's partials, part[f], and the part's local bin array.  The caller launches
// its first pass over part[] and the second pass over fa, then calls add_to.
template <int NF>
class PartBins {
    size_t part_n_, bins_n_;
    int want_;
    DeviceStage stage_;

public:
    double *part[NF] = {};  // in the header's field order; null where not requested
    FoldArgs fa{};
    // x, c, r: the axes of FoldArgs; rows: rows of a chunk that keep partials of their own (D2Q9: 1, D3Q19: ny)
    PartBins(const Axis &x, const ChunkAxis &c, const Axis &r, size_t rows, int wave_cols, int nslots,
             double *const *out)
        : part_n_((size_t)c.chunks() * rows * nslots), bins_n_((size_t)c.a.nbl * r.nbl * x.nbl),
          want_(count_wanted(out, NF)), stage_(sizeof(double) * (part_n_ + bins_n_) * want_) {
        fa.x = x;
        fa.c = c;
        fa.r = r;
        fa.wave_cols = wave_cols;
        fa.nslots = nslots;
        fa.want = want_;
        double *bins = stage_.template as<double>() + part_n_ * want_;
        for (int i = 0, n = 0; i < NF; ++i)
            if (out[i]) {
                part[i] = stage_.template as<double>() + part_n_ * n;
                fa.part[n] = part[i];
                fa.out[n] = bins + bins_n_ * n;
                ++n;
            }
    }
    // Once both passes are in st: waits for it, copies the part's bin arrays to the host and adds them into the
    // bins they cover of out[f], double[..][nbr][nbx] over the full bin grid (nbr: the bins along the axis r,
    // D2Q9: 1).  Called part after part, so a bin that spans several parts is summed in their order.
    void add_to(hipStream_t st, double *const *out, int nbx, int nbr) const {
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<double> host(bins_n_ * want_);
        HIP_CHECK(hipMemcpy(host.data(), fa.out[0], sizeof(double) * host.size(), hipMemcpyDeviceToHost));
        const double *src = host.data();
        for (int i = 0; i < NF; ++i) {
            if (!out[i]) continue;
            for (int bc = 0; bc < fa.c.a.nbl; ++bc)
                for (int br = 0; br < fa.r.nbl; ++br) {
                    double *dst = out[i] + ((size_t)(fa.c.a.b_lo + bc) * nbr + (fa.r.b_lo + br)) * nbx + fa.x.b_lo;
                    for (int bx = 0; bx < fa.x.nbl; ++bx) dst[bx] += *src++;
                }
        }
    }
};

}  // namespace binned
}  // namespace lbm
