// lbm3d_binned.hip -- sums of per-cell quantities over box-shaped bins of the
// D3Q19 engine's current lattice (the lbm3d_* functions of
// include/lbm_binned_hip.h).  The kernel, then the engine's host side.
//
// One memory-bound pass over the 19 populations, 77 B read per cell, one cell
// per lane: a wave takes 64 consecutive cells of one row and walks a chunk --
// at most BN_CHUNK planes inside one z bin -- with its 14 fp64 sums in
// registers, then folds along x by bin (fold_x, lbm_binned.hpp) and stores one
// partial per bin it touches.  The second pass (fold_bins, lbm_binned.hip) adds
// a bin's partials over its chunks, rows and waves.  Offsets are formed in 64
// bits.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "lbm3d_engine.hpp"
#include "lbm_binned.hpp"
#include "lbm_binned_hip.h"
#include "lbm_quad.hpp"

namespace lbm {
namespace binned {

// the view of the whole slab; the kernel reads o, obst, PL, KS, px, nx and ny of it (the box, quad, sp and
// obst_pressure ride along unused)
struct Bin3Args : Box3View {
    Axis x;
    ChunkAxis z;
    int nwx, nslots;       // waves along x; partial slots of a (chunk, row)
    double *part[BN_FIELDS3];  // [chunks][ny][nslots] per requested field, else null
};

__global__ __launch_bounds__(BN_BLOCK) void binned_sums3d(Bin3Args a) {
    const long long item = (long long)blockIdx.x * (BN_BLOCK / 64) + (threadIdx.x >> 6);
    const long long per_chunk = (long long)a.ny * a.nwx;
    if (item >= a.z.chunks() * per_chunk) return;  // wave-uniform: the block never synchronises
    const int chunk = (int)(item / per_chunk);
    const int rest = (int)(item - chunk * per_chunk);
    const int y = rest / a.nwx, wx = rest - y * a.nwx;
    int z0, z1;
    a.z.chunk_range(chunk, z0, z1);
    if (z0 >= z1) return;
    const int x = wx * BN3_WAVE_COLS + (threadIdx.x & 63);
    double s[1][BN_FIELDS3];
#pragma unroll
    for (int f = 0; f < BN_FIELDS3; ++f) s[0][f] = 0.0;
    const int key[1] = {x < a.nx ? x / a.x.bsz : KEY_NONE};
    if (x < a.nx) {
        for (int z = z0; z < z1; ++z) {
            const float *src = a.o + (long long)z * a.PL + (long long)y * a.px + x;
            float c[19];
            load_cell<19>(src, a.KS, 0, c);
            add_cell3(c, a.obst[((long long)z * a.ny + y) * a.nx + x] != 0, s[0]);
        }
    }
    fold_x<1, BN_FIELDS3>(s, key, a.x.bsz > 1, wx, ((long long)chunk * a.ny + y) * a.nslots, a.part);
}

hipError_t launch_binned_sums3d(const Bin3Args &a, hipStream_t s) {
    const long long waves = (long long)a.z.chunks() * a.ny * a.nwx;
    const long long blocks = (waves + BN_BLOCK / 64 - 1) / (BN_BLOCK / 64);
    if (blocks >= (1LL << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(binned_sums3d, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace binned
}  // namespace lbm

// ---- D3Q19 engine: host side ----

using namespace lbm;

// The LBM3D_BIN_* sums of the current lattice into planar host arrays
// double[nbz][nby][nbx] over the full bin grid (a NULL entry is neither staged
// nor copied), slab after slab: a z bin that spans several slabs is summed in
// their order.
void lbm3d_handle::store_binned(int bw, int bh, int bd, double *const *out) {
    using namespace lbm::binned;
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take binned sums of");
    lbm::binned::check_bins(p.nx, p.ny, p.nz, bw, bh, bd);
    const int want = count_wanted(out, LBM3D_BIN_FIELDS);
    if (want == 0) return;
    const int nbx = LBM_BIN_COUNT(p.nx, bw), nby = LBM_BIN_COUNT(p.ny, bh), nbz = LBM_BIN_COUNT(p.nz, bd);
    const size_t layer = (size_t)nbx * nby;
    for (int i = 0; i < LBM3D_BIN_FIELDS; ++i)
        if (out[i]) std::fill(out[i], out[i] + layer * nbz, 0.0);
    sync_all();
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        Bin3Args a{box_view(s, 0, 0, 0, p.nx, p.ny, s.nzs)};
        a.x = make_axis(0, p.nx, bw);
        a.z = make_chunk_axis(s.z0, s.nzs, bd);
        a.nwx = (p.nx + BN3_WAVE_COLS - 1) / BN3_WAVE_COLS;
        a.nslots = a.nwx + a.x.nbl - 1;
        const PartBins<LBM3D_BIN_FIELDS> pb(a.x, a.z, make_axis(0, p.ny, bh), (size_t)p.ny, BN3_WAVE_COLS, a.nslots, out);
        std::copy(pb.part, pb.part + LBM3D_BIN_FIELDS, a.part);
        HIP_CHECK(launch_binned_sums3d(a, s.s_comp));
        HIP_CHECK(launch_fold_bins(pb.fa, s.s_comp));
        pb.add_to(s.s_comp, out, nbx, nby);
    }
}

// Fluid cells per bin over the local slabs, from their obstacle maps (a copy
// to the host, no launch).
void lbm3d_handle::bin_fluid_cells(int bw, int bh, int bd, int64_t *count) {
    lbm::binned::check_bins(p.nx, p.ny, p.nz, bw, bh, bd);
    if (!count) return;
    const int nbx = LBM_BIN_COUNT(p.nx, bw), nby = LBM_BIN_COUNT(p.ny, bh), nbz = LBM_BIN_COUNT(p.nz, bd);
    std::fill(count, count + (size_t)nbx * nby * nbz, (int64_t)0);
    sync_all();
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        std::vector<uint8_t> ob((size_t)p.nx * p.ny * s.nzs);
        HIP_CHECK(hipMemcpy(ob.data(), s.obst, ob.size(), hipMemcpyDeviceToHost));
        const uint8_t *o = ob.data();
        for (int z = 0; z < s.nzs; ++z)
            for (int y = 0; y < p.ny; ++y) {
                int64_t *row = count + ((size_t)((s.z0 + z) / bd) * nby + y / bh) * nbx;
                for (int x = 0; x < p.nx; ++x) row[x / bw] += *o++ ? 0 : 1;
            }
    }
}
