// lbm_transport.hip -- the binned transport sums of the D2Q9 engine's passive
// scalar (the lbm_* functions of include/lbm_transport_hip.h): the kernel, the
// engine's host side, the extern "C" functions and the host-only restatement
// lbm_scalar_terms_ref.
//
// The kernel (scalar_binned) has the shape of binned_sums (lbm_binned.hip) and
// the access pattern of scalar_step (lbm_scalar.hip).  A lane owns four
// consecutive columns, a wave 256, and walks one chunk -- at most BN_CHUNK rows
// inside one bin -- with the fp64 sums of its four columns in registers, then
// folds along x by bin (fold_x, lbm_binned.hpp) and stores one partial per bin
// it touches; the second pass is fold_bins of the flow's binned sums.  Per row
// a lane makes 16-B loads of the nine flow quads, the obstacle word, its own
// quads of g0..g4 and the g4 quad of the row above (the top of the DOMAIN wraps,
// not that of the sub-domain).  The one value off the alignment, g3[x + 4],
// comes from lane + 1 by a cross-lane move -- the trip count of the row loop is
// the same for every lane of a wave, so the move runs converged -- and the last
// lane of a wave or of a row loads it directly (the periodic image at the
// domain's end).  The scalar is read at global coordinates; no ghost cell of
// either lattice is read.  The last w % 4 cells of a row, and sub-domains whose
// x origin is no multiple of 4, go one cell at a time.  No LDS, no atomics.
//
// Two compiled forms.  With a U?PHI field requested: 57 B per cell (36 flow,
// 1 map, 20 scalar).  With none: the flow lattice is not loaded and no divide
// is made (21 B); if no PHI / PHIPHI field is requested either, only the
// planes the requested faces need are loaded (FX: g1, g3; FY: g2, g4).
//
// Arithmetic: the terms of lbm_transport.hpp, no contraction.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm_binned.hpp"
#include "lbm_cell_macro.hpp"
#include "lbm_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_transport.hpp"
#include "lbm_transport_hip.h"

namespace lbm {
namespace transport {

using namespace lbm::binned;
using scalar::above;

// one sub-domain's flow lattice, where its cell (0, 0) lies in the domain, the current scalar set and the bins
struct SBin2Args : LatticeView {
    Axis x;
    ChunkAxis y;
    int nwx, nslots;  // waves along x; partial slots of a chunk
    const float *g;
    long long gplane;
    int gsp, gx0, gy0, nx, ny;
    int quad;                        // gx0 % 4 == 0: the 16-B path
    int need_own, need_fx, need_fy;  // no-flow form: all of g0..g4 and the map; g1 and g3; g2 and g4
    double *part[SB_FIELDS2];        // [chunks][nslots] per requested field, else null
};

namespace {

// cell (x, y) of the sub-domain, every value loaded on its own
template <bool FLOW, int NF>
__device__ __forceinline__ void add_one(const SBin2Args &a, int x, int y, double (&s)[NF]) {
    const int gx = a.gx0 + x, gy = a.gy0 + y;
    const long long row = (long long)gy * a.gsp;
    float g[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) g[k] = a.g[k * a.gplane + row + gx];
    const float back[2] = {a.g[3 * a.gplane + row + above(gx, a.nx)],
                           a.g[4 * a.gplane + (long long)above(gy, a.ny) * a.gsp + gx]};
    const bool blocked = a.obst[(long long)y * a.w + x] != 0;
    double t[NF];
    if constexpr (FLOW) {
        float c[Q], rho;
        load_cell<Q>(a.o + (long long)y * a.pitch, a.plane, x, c);
        const CellMacro m = cell_macro<true, false>(c, false, a.obst_pressure, rho);
        const float u[2] = {m.ux, m.uy};
        cell_terms<2>(g, back, blocked, u, t);
    } else {
        cell_terms_noflow<2>(g, back, blocked, t);
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) s[f] += t[f];
}

}  // namespace

template <bool FLOW>
__global__ __launch_bounds__(BN_BLOCK) void scalar_binned(SBin2Args a) {
    constexpr int NF = FLOW ? SB_FIELDS2 : SB_NOFLOW2;
    const long long item = (long long)blockIdx.x * (BN_BLOCK / 64) + (threadIdx.x >> 6);
    if (item >= (long long)a.y.chunks() * a.nwx) return;  // wave-uniform: the block never synchronises
    const int chunk = (int)(item / a.nwx), wx = (int)(item - (long long)chunk * a.nwx);
    int r0, r1;
    a.y.chunk_range(chunk, r0, r1);
    if (r0 >= r1) return;  // wave-uniform
    const int lane = threadIdx.x & 63;
    const int x = wx * BN_WAVE_COLS + lane * BN_QUAD;
    const bool obst_word = (a.w & 3) == 0;
    const bool full = a.quad && x + BN_QUAD <= a.w;
    const bool own = FLOW || a.need_own, fx = FLOW || a.need_fx, fy = FLOW || a.need_fy;
    double s[BN_QUAD][NF];
    int key[BN_QUAD];
#pragma unroll
    for (int i = 0; i < BN_QUAD; ++i) {
        key[i] = x + i < a.w ? (a.x.g0 + x + i) / a.x.bsz : KEY_NONE;
#pragma unroll
        for (int f = 0; f < NF; ++f) s[i][f] = 0.0;
    }
    const int gx = a.gx0 + x;
    // r0, r1 are the same for every lane of the wave and no lane leaves the loop early: the cross-lane move runs
    // converged
    for (int y = r0; y < r1; ++y) {
        const int gy = a.gy0 + y;
        const float *row = a.g + (long long)gy * a.gsp;
        const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
        float4 gq[5] = {zero, zero, zero, zero, zero};
        if (full && fx) gq[3] = *reinterpret_cast<const float4 *>(row + 3 * a.gplane + gx);
        // lane + 1 holds the quad to the east when that quad lies in this row
        const float east = __shfl_down(gq[3].x, 1, 64);
        if (full) {
            float pe = 0.f;
            if (fx) pe = (lane != 63 && x + 2 * BN_QUAD <= a.w) ? east : row[3 * a.gplane + (gx + 4 == a.nx ? 0 : gx + 4)];
            float4 north = zero;
            if (fy) north = *reinterpret_cast<const float4 *>(a.g + 4 * a.gplane + (long long)above(gy, a.ny) * a.gsp + gx);
            if (own || fx) gq[1] = *reinterpret_cast<const float4 *>(row + a.gplane + gx);
            if (own || fy) gq[2] = *reinterpret_cast<const float4 *>(row + 2 * a.gplane + gx);
            unsigned bits = 0;
            if (own) {
                gq[0] = *reinterpret_cast<const float4 *>(row + gx);
                if (!fx) gq[3] = *reinterpret_cast<const float4 *>(row + 3 * a.gplane + gx);
                gq[4] = *reinterpret_cast<const float4 *>(row + 4 * a.gplane + gx);
                bits = quad_map_bytes(a.obst + (long long)y * a.w + x, obst_word);
            }
            float4 v[Q];
            if (FLOW) load_quad<Q>(a.o + (long long)y * a.pitch + x, a.plane, v);
            const float4 p3 = make_float4(gq[3].y, gq[3].z, gq[3].w, pe);
#pragma unroll
            for (int i = 0; i < BN_QUAD; ++i) {
                const float g[5] = {pick(gq[0], i), pick(gq[1], i), pick(gq[2], i), pick(gq[3], i), pick(gq[4], i)};
                const float back[2] = {pick(p3, i), pick(north, i)};
                const bool blocked = ((bits >> (8 * i)) & 0xffu) != 0;
                double t[NF];
                if constexpr (FLOW) {
                    float c[Q], rho;
                    quad_cell<Q>(v, i, c);
                    // as a fluid cell, whatever the map says: the terms select afterwards, and a branch on the
                    // map here lets the compiler sink the flow loads into it, 4 B at a time
                    const CellMacro m = cell_macro<true, false>(c, false, a.obst_pressure, rho);
                    const float u[2] = {m.ux, m.uy};
                    cell_terms<2>(g, back, blocked, u, t);
                } else {
                    cell_terms_noflow<2>(g, back, blocked, t);
                }
#pragma unroll
                for (int f = 0; f < NF; ++f) s[i][f] += t[f];
            }
        } else if (x < a.w) {
            // the ragged tail of a row, or a sub-domain off the alignment: one cell at a time
#pragma unroll
            for (int i = 0; i < BN_QUAD; ++i)
                if (x + i < a.w) add_one<FLOW, NF>(a, x + i, y, s[i]);
        }
    }
    double *part[NF];
#pragma unroll
    for (int j = 0; j < NF; ++j) part[j] = a.part[FLOW ? j : noflow_field<2>(j)];
    fold_x<BN_QUAD, NF>(s, key, a.x.bsz > 1, wx - a.x.b_lo, (long long)chunk * a.nslots, part);
}

hipError_t launch_scalar_binned(const SBin2Args &a, bool flow, hipStream_t s) {
    const long long waves = (long long)a.y.chunks() * a.nwx;
    const long long blocks = (waves + BN_BLOCK / 64 - 1) / (BN_BLOCK / 64);
    if (flow)
        hipLaunchKernelGGL(scalar_binned<true>, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(scalar_binned<false>, dim3((unsigned)blocks), dim3(BN_BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace transport
}  // namespace lbm

// ---- D2Q9 engine: host side ----

// The LBM_SBIN_* sums of the current lattice and scalar into planar host arrays double[nby][nbx] over the full
// bin grid, sub-domain after sub-domain as lbm_handle::store_binned, all on the first sub-domain's compute stream.
void lbm_handle::scalar_store_binned(int bw, int bh, double *const *out) {
    using namespace lbm::binned;
    using namespace lbm::transport;
    if (!scalars) throw lbm_failure(LBM_E_STATE, "no scalar: call lbm_scalar_begin first");
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take the scalar's transport sums over");
    check_bins(p.nx, p.ny, 1, bw, bh, 1);
    const Wanted<2> want(out);
    if (want.count == 0) return;
    const scalar::State &t = *scalars;
    const int nbx = LBM_BIN_COUNT(p.nx, bw), nby = LBM_BIN_COUNT(p.ny, bh);
    for (int i = 0; i < LBM_SBIN_FIELDS; ++i)
        if (out[i]) std::fill(out[i], out[i] + (size_t)nbx * nby, 0.0);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    for (auto &s : subs) {
        SBin2Args a{lattice_view(s)};
        a.x = make_axis(s.rect.x0, s.w, bw);
        a.y = make_chunk_axis(s.rect.y0, s.h, bh);
        a.nwx = (s.w + BN_WAVE_COLS - 1) / BN_WAVE_COLS;
        a.nslots = a.nwx + a.x.nbl - 1;
        if ((long long)a.y.chunks() * a.nwx > (1LL << 32))
            throw lbm_failure(LBM_E_INVALID, "sub-domain too large for binned sums");
        a.g = t.g[t.cur];
        a.gplane = t.grid.plane;
        a.gsp = t.grid.sp;
        a.gx0 = s.rect.x0;
        a.gy0 = s.rect.y0;
        a.nx = p.nx;
        a.ny = p.ny;
        a.quad = s.rect.x0 % 4 == 0 ? 1 : 0;
        a.need_own = want.phi;
        a.need_fx = want.face[0];
        a.need_fy = want.face[1];
        const PartBins<LBM_SBIN_FIELDS> pb(a.x, a.y, Axis{0, 1, 1, 0, 1}, 1, BN_WAVE_COLS, a.nslots, out);
        std::copy(pb.part, pb.part + LBM_SBIN_FIELDS, a.part);
        timed(s0, s0.s_comp, "scalar_binned", [&] { HIP_CHECK(launch_scalar_binned(a, want.flow, s0.s_comp)); });
        timed(s0, s0.s_comp, "scalar_binned fold", [&] { HIP_CHECK(launch_fold_bins(pb.fa, s0.s_comp)); });
        pb.add_to(s0.s_comp, out, nbx, 1);
    }
    prof_collect();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm_scalar_store_binned(lbm_handle *h, int32_t bw, int32_t bh, double *const out[LBM_SBIN_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_store_binned(bw, bh, out); });
}

int lbm_scalar_terms_ref(int32_t nx, int32_t ny, const float *ux, const float *uy, const uint8_t *obst,
                         const float *g, double *terms) {
    using namespace lbm;
    if (!transport::ref_args_ok(nx, ny, 1, {ux, uy, obst, g, terms})) return LBM_E_INVALID;
    const size_t plane = (size_t)nx * ny;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const size_t row = (size_t)y * nx, i = row + x;
            const float gc[5] = {g[i], g[plane + i], g[2 * plane + i], g[3 * plane + i], g[4 * plane + i]};
            const float back[2] = {g[3 * plane + row + scalar::above(x, nx)],
                                   g[4 * plane + (size_t)scalar::above(y, ny) * nx + x]};
            const float u[2] = {ux[i], uy[i]};
            double t[LBM_SBIN_FIELDS];
            transport::cell_terms<2>(gc, back, obst[i] != 0, u, t);
            for (int f = 0; f < LBM_SBIN_FIELDS; ++f) terms[f * plane + i] = t[f];
        }
    return LBM_OK;
}

}  // extern "C"
