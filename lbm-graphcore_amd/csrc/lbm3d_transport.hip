// lbm3d_transport.hip -- the binned transport sums of the D3Q19 engine's
// passive scalar (the lbm3d_* functions of include/lbm_transport_hip.h): the
// kernel, the engine's host side, the extern "C" functions and the host-only
// restatement lbm3d_scalar_terms_ref.
//
// The kernel (scalar_binned3d) has the shape of binned_sums3d
// (lbm3d_binned.hip): one cell per lane, a wave takes 64 consecutive cells of
// one row and walks a chunk -- at most BN_CHUNK planes inside one z bin -- with
// its fp64 sums in registers, then folds along x by bin (fold_x) and stores one
// partial per bin it touches; the second pass is fold_bins.  Per plane a lane
// first reduces the 19 flow populations to the three velocities, then loads
// its seven scalar populations (loading everything at once is what took all
// 256 VGPRs in scalar_step3d).  g2[x + 1] comes from lane + 1 by a cross-lane
// move -- the trip count of the plane loop is the same for every lane of a
// wave, so the move runs converged -- with a direct load for the last lane of a
// wave and at the periodic wrap; g4[y + 1] and g6[z + 1] are direct loads, the
// latter at the global z with the wrap at the top of the DOMAIN.  No LDS, no
// atomics.  Offsets are formed in 64 bits.
//
// Two compiled forms.  With a U?PHI field requested: 105 B per cell (76 flow,
// 1 map, 28 scalar).  With none: the flow lattice is not loaded (29 B); if no
// PHI / PHIPHI field is requested either, only the planes the requested faces
// need are loaded (FX: g1, g2; FY: g3, g4; FZ: g5, g6).

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm3d_cell_macro.hpp"
#include "lbm3d_engine.hpp"
#include "lbm_binned.hpp"
#include "lbm_quad.hpp"
#include "lbm_transport.hpp"
#include "lbm_transport_hip.h"

namespace lbm {
namespace transport {

using namespace lbm::binned;
using scalar::above;

// the view of the whole slab (the kernel reads o, obst, PL, KS, px, nx, ny and obst_pressure of it), its first
// plane in the domain, the current scalar set and the bins
struct SBin3Args : Box3View {
    Axis x;
    ChunkAxis z;
    int nwx, nslots;  // waves along x; partial slots of a (chunk, row)
    const float *g;
    long long gplane;
    int gsp, gz0, nz;
    int need_own, need_face[3];  // no-flow form: all of g0..g6 and the map; the two planes of a face
    double *part[SB_FIELDS3];    // [chunks][ny][nslots] per requested field, else null
};

template <bool FLOW>
__global__ __launch_bounds__(BN_BLOCK) void scalar_binned3d(SBin3Args a) {
    constexpr int NF = FLOW ? SB_FIELDS3 : SB_NOFLOW3;
    const long long item = (long long)blockIdx.x * (BN_BLOCK / 64) + (threadIdx.x >> 6);
    const long long per_chunk = (long long)a.ny * a.nwx;
    if (item >= a.z.chunks() * per_chunk) return;  // wave-uniform: the block never synchronises
    const int chunk = (int)(item / per_chunk);
    const int rest = (int)(item - chunk * per_chunk);
    const int y = rest / a.nwx, wx = rest - y * a.nwx;
    int z0, z1;
    a.z.chunk_range(chunk, z0, z1);
    if (z0 >= z1) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int x = wx * BN3_WAVE_COLS + lane;
    const bool in = x < a.nx;
    const bool own = FLOW || a.need_own;
    const bool fx = FLOW || a.need_face[0], fy = FLOW || a.need_face[1], fz = FLOW || a.need_face[2];
    double s[1][NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) s[0][f] = 0.0;
    const int key[1] = {in ? x / a.x.bsz : KEY_NONE};
    const int yn = above(y, a.ny);
    // z0, z1 are the same for every lane of the wave and no lane leaves the loop early: the cross-lane move runs
    // converged
    for (int z = z0; z < z1; ++z) {
        const int gz = a.gz0 + z;
        const long long row = ((long long)gz * a.ny + y) * a.gsp;
        float g[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (in && (own || fx)) g[2] = a.g[2 * a.gplane + row + x];
        // lane + 1 holds the cell to the east when that cell lies in this row
        const float east = __shfl_down(g[2], 1, 64);
        if (in) {
            float u[3] = {0.f, 0.f, 0.f};
            bool blocked = false;
            if constexpr (FLOW) {
                // first the flow: its 19 registers are dead once the three velocities stand
                float c[19], rho;
                load_cell<19>(a.o + (long long)z * a.PL + (long long)y * a.px + x, a.KS, 0, c);
                // as a fluid cell, whatever the map says: the terms select afterwards
                const Cell3Macro m = cell3_macro<true, false>(c, false, a.obst_pressure, rho);
                u[0] = m.ux;
                u[1] = m.uy;
                u[2] = m.uz;
                __builtin_amdgcn_sched_barrier(0);
            }
            float back[3] = {0.f, 0.f, 0.f};
            if (fx) back[0] = (lane != 63 && x + 1 < a.nx) ? east : a.g[2 * a.gplane + row + above(x, a.nx)];
            if (fy) back[1] = a.g[4 * a.gplane + ((long long)gz * a.ny + yn) * a.gsp + x];
            if (fz) back[2] = a.g[6 * a.gplane + ((long long)above(gz, a.nz) * a.ny + y) * a.gsp + x];
            if (own || fx) g[1] = a.g[a.gplane + row + x];
            if (own || fy) g[3] = a.g[3 * a.gplane + row + x];
            if (own || fz) g[5] = a.g[5 * a.gplane + row + x];
            if (own) {
                g[0] = a.g[row + x];
                g[4] = a.g[4 * a.gplane + row + x];
                g[6] = a.g[6 * a.gplane + row + x];
                blocked = a.obst[((long long)z * a.ny + y) * a.nx + x] != 0;
            }
            double t[NF];
            if constexpr (FLOW)
                cell_terms<3>(g, back, blocked, u, t);
            else
                cell_terms_noflow<3>(g, back, blocked, t);
#pragma unroll
            for (int f = 0; f < NF; ++f) s[0][f] += t[f];
        }
    }
    double *part[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) part[j] = a.part[FLOW ? j : noflow_field<3>(j)];
    fold_x<1, NF>(s, key, a.x.bsz > 1, wx, ((long long)chunk * a.ny + y) * a.nslots, part);
}

hipError_t launch_scalar_binned3d(const SBin3Args &a, bool flow, hipStream_t s) {
    const long long waves = (long long)a.z.chunks() * a.ny * a.nwx;
    const long long blocks = (waves + BN_BLOCK / 64 - 1) / (BN_BLOCK / 64);
    if (blocks >= (1LL << 31)) return hipErrorInvalidValue;
    if (flow)
        hipLaunchKernelGGL(scalar_binned3d<true>, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(scalar_binned3d<false>, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace transport
}  // namespace lbm

// ---- D3Q19 engine: host side ----

using namespace lbm;

// The LBM3D_SBIN_* sums of the current lattice and scalar into planar host arrays double[nbz][nby][nbx] over the
// full bin grid, slab after slab as lbm3d_handle::store_binned, all on the first slab's compute stream.
void lbm3d_handle::scalar_store_binned(int bw, int bh, int bd, double *const *out) {
    using namespace lbm::binned;
    using namespace lbm::transport;
    if (!scalars) throw lbm_failure(LBM_E_STATE, "no scalar: call lbm3d_scalar_begin first");
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take the scalar's transport sums over");
    check_bins(p.nx, p.ny, p.nz, bw, bh, bd);
    const Wanted<3> want(out);
    if (want.count == 0) return;
    const scalar::State &t = *scalars;
    const int nbx = LBM_BIN_COUNT(p.nx, bw), nby = LBM_BIN_COUNT(p.ny, bh), nbz = LBM_BIN_COUNT(p.nz, bd);
    for (int i = 0; i < LBM3D_SBIN_FIELDS; ++i)
        if (out[i]) std::fill(out[i], out[i] + (size_t)nbx * nby * nbz, 0.0);
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    const hipStream_t st = slabs[0].s_comp;
    for (auto &s : slabs) {
        SBin3Args a{box_view(s, 0, 0, 0, p.nx, p.ny, s.nzs)};
        a.x = make_axis(0, p.nx, bw);
        a.z = make_chunk_axis(s.z0, s.nzs, bd);
        a.nwx = (p.nx + BN3_WAVE_COLS - 1) / BN3_WAVE_COLS;
        a.nslots = a.nwx + a.x.nbl - 1;
        a.g = t.g[t.cur];
        a.gplane = t.grid.plane;
        a.gsp = t.grid.sp;
        a.gz0 = s.z0;
        a.nz = p.nz;
        a.need_own = want.phi;
        for (int c = 0; c < 3; ++c) a.need_face[c] = want.face[c];
        const PartBins<LBM3D_SBIN_FIELDS> pb(a.x, a.z, make_axis(0, p.ny, bh), (size_t)p.ny, BN3_WAVE_COLS, a.nslots,
                                             out);
        std::copy(pb.part, pb.part + LBM3D_SBIN_FIELDS, a.part);
        HIP_CHECK(launch_scalar_binned3d(a, want.flow, st));
        HIP_CHECK(launch_fold_bins(pb.fa, st));
        pb.add_to(st, out, nbx, nby);
    }
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm3d_scalar_store_binned(lbm3d_handle *h, int32_t bw, int32_t bh, int32_t bd,
                              double *const out[LBM3D_SBIN_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_store_binned(bw, bh, bd, out); });
}

int lbm3d_scalar_terms_ref(int32_t nx, int32_t ny, int32_t nz, const float *ux, const float *uy, const float *uz,
                           const uint8_t *obst, const float *g, double *terms) {
    if (!transport::ref_args_ok(nx, ny, nz, {ux, uy, uz, obst, g, terms})) return LBM_E_INVALID;
    const size_t plane = (size_t)nx * ny * nz;
    const auto at = [&](int x, int y, int z) { return ((size_t)z * ny + y) * nx + x; };
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const size_t i = at(x, y, z);
                float gc[7];
                for (int k = 0; k < 7; ++k) gc[k] = g[k * plane + i];
                const float back[3] = {g[2 * plane + at(scalar::above(x, nx), y, z)],
                                       g[4 * plane + at(x, scalar::above(y, ny), z)],
                                       g[6 * plane + at(x, y, scalar::above(z, nz))]};
                const float u[3] = {ux[i], uy[i], uz[i]};
                double t[LBM3D_SBIN_FIELDS];
                transport::cell_terms<3>(gc, back, obst[i] != 0, u, t);
                for (int f = 0; f < LBM3D_SBIN_FIELDS; ++f) terms[f * plane + i] = t[f];
            }
    return LBM_OK;
}

}  // extern "C"
