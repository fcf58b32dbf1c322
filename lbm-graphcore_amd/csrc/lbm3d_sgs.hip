// lbm3d_sgs.hip -- the sub-grid model of the D3Q19 engine (the lbm3d_sgs_*
// functions of include/lbm_sgs_hip.h): the kernel that rescales the stored
// non-equilibrium part of every cell of one slab, the engine's host side, the
// extern "C" functions and the host-only restatement lbm3d_sgs_filter_ref.
//
// The kernel.  A streaming read-modify-write of the current flow lattice over
// the cells of one slab: per cell the nineteen populations read (76 B) and
// written (76 B) and the obstacle byte, 153 B; a coefficient plane adds 4 B.
// The block and grid of the forcing zones (scalar::slab_grid over the slab;
// one wave along x, a block's waves on consecutive rows).  A lane takes four
// consecutive cells with 16-B loads and stores of the nineteen planes (and a
// 16-B load of the coefficient plane, which lies on the same grid:
// lbm_sgs.hpp); the ragged tail of a row goes one cell at a time, and a domain
// of fewer than four columns one cell per lane.  A lane needs only its own
// cells and owns what it writes: no LDS, no atomics, no cross-lane move --
// except, in the forms that return the statistics, the fixed-order fold of the
// block's sums (fold_block).  Ghost planes and pad columns are not touched.
//
// Four compiled forms edit the lattice (coefficient constant or from the plane,
// each with and without the statistics); two more (NUT) write nu_add to a
// staging array and leave the lattice alone (lbm3d_sgs_store_nut).
//
// Arithmetic: IEEE fp32, as the header writes it, no contraction
// (-ffp-contract=off).

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm3d_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_sgs.hpp"
#include "lbm_sgs_hip.h"

namespace lbm {
namespace sgs {

constexpr int WAVE = 64;  // lanes of a block along x: one wave (checked against scalar::slab_lanes_x at the launch)

// The view's box is the whole slab.
struct Sgs3 : Box3Edit {
    Model m;
    float konst;
    const float *coef;  // the coefficient of the slab's cell (x, y, z) at coef[(z * ny + y) * cp + x]; PLANE forms
    int cp;
    float *nut;        // NUT forms: float[bz][by][sp]
    double *sum_part;  // statistics forms: [2][blocks]
    float *max_part;   // [1][blocks]
};

namespace {

template <bool PLANE, bool STATS, bool NUT>
__device__ __forceinline__ void filter_one(const Sgs3 &a, int x, int y, int z, Acc &acc) {
    float *f = a.e + (long long)z * a.PL + (long long)y * a.px + x;
    float c[Q3], q[Q3], d, nut;
    load_cell<Q3>(f, a.KS, 0, c);
    const long long row = (long long)z * a.ny + y;
    const bool blocked = a.obst[row * a.nx + x] != 0;
    const float k = PLANE ? a.coef[row * a.cp + x] : a.konst;
    const bool idle = filter3(c, blocked, a.m, k, q, d, nut);
    if (NUT) {
        a.nut[((long long)z * a.by + y) * a.sp + x] = nut;
    } else {
#pragma unroll
        for (int j = 0; j < Q3; ++j) f[j * a.KS] = rescaled(c[j], q[j], d, idle);
    }
    if (STATS) acc.add(idle, nut);
}

__device__ __forceinline__ void put(float4 &v, int i, float x) {
    if (i == 0)
        v.x = x;
    else if (i == 1)
        v.y = x;
    else if (i == 2)
        v.z = x;
    else
        v.w = x;
}

}  // namespace

template <bool PLANE, bool STATS, bool NUT>
__global__ __launch_bounds__(BLOCK) void sgs_filter3d(Sgs3 a) {
    constexpr int ROWS = BLOCK / WAVE;
    const bool quad = a.quad != 0;
    const int cpl = quad ? 4 : 1;  // cells per lane
    const int tx = threadIdx.x & (WAVE - 1), ty = threadIdx.x / WAVE;
    const int x = (blockIdx.x * WAVE + tx) * cpl;
    const bool full = quad && x + 4 <= a.bx;
    const bool obst_word = (a.nx & 3) == 0;
    Acc acc;
    if (x < a.bx) {
        for (int z = blockIdx.z; z < a.bz; z += gridDim.z) {
            for (int y = blockIdx.y * ROWS + ty; y < a.by; y += gridDim.y * ROWS) {
                if (full) {
                    const long long row = (long long)z * a.ny + y;
                    float *f = a.e + (long long)z * a.PL + (long long)y * a.px + x;
                    float4 v[Q3];
                    load_quad<Q3>(f, a.KS, v);
                    const unsigned bits = quad_map_bytes(a.obst + row * a.nx + x, obst_word);
                    float4 kq = make_float4(a.konst, a.konst, a.konst, a.konst);
                    if (PLANE) kq = *reinterpret_cast<const float4 *>(a.coef + row * a.cp + x);
                    float nu[4];
                    // cell after cell, the new values back into the loaded quads: one cell's q is live at a time
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float c[Q3], q[Q3], d;
                        quad_cell<Q3>(v, i, c);
                        const bool idle = filter3(c, ((bits >> (8 * i)) & 0xffu) != 0, a.m, pick(kq, i), q, d, nu[i]);
                        if (!NUT) {
#pragma unroll
                            for (int j = 0; j < Q3; ++j) put(v[j], i, rescaled(c[j], q[j], d, idle));
                        }
                        if (STATS) acc.add(idle, nu[i]);
                    }
                    if (NUT) {
                        *reinterpret_cast<float4 *>(a.nut + ((long long)z * a.by + y) * a.sp + x) =
                            make_float4(nu[0], nu[1], nu[2], nu[3]);
                    } else {
#pragma unroll
                        for (int j = 0; j < Q3; ++j) *reinterpret_cast<float4 *>(f + j * a.KS) = v[j];
                    }
                } else {
                    // the ragged tail of a row, or one cell per lane
#pragma unroll 1
                    for (int i = 0; i < cpl; ++i)
                        if (x + i < a.bx) filter_one<PLANE, STATS, NUT>(a, x + i, y, z, acc);
                }
            }
        }
    }
    if (STATS) {
        double s[2] = {acc.cells, acc.sum};
        float m[1] = {acc.max};
        const long long block = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        fold_block<ROWS>(s, m, block, (long long)gridDim.x * gridDim.y * gridDim.z, a.sum_part, a.max_part);
    }
}

namespace {

template <bool PLANE>
void launch_filter(const Sgs3 &a, bool stats, bool nut, dim3 grid, hipStream_t st) {
    if (nut)
        hipLaunchKernelGGL((sgs_filter3d<PLANE, false, true>), grid, dim3(BLOCK), 0, st, a);
    else if (stats)
        hipLaunchKernelGGL((sgs_filter3d<PLANE, true, false>), grid, dim3(BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((sgs_filter3d<PLANE, false, false>), grid, dim3(BLOCK), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

void launch_filter(const Sgs3 &a, bool stats, bool nut, dim3 grid, hipStream_t st) {
    if (a.coef)
        launch_filter<true>(a, stats, nut, grid, st);
    else
        launch_filter<false>(a, stats, nut, grid, st);
}

// the arguments of slab s for the model z and the application m, the outputs null
Sgs3 slab_args(const Box3Edit &view, const Slab &s, int ny, const State &z, const Model &m) {
    Sgs3 a{view};
    a.m = m;
    a.konst = z.konst;
    a.cp = z.cp;
    a.coef = z.plane ? z.plane + (long long)s.z0 * ny * z.cp : nullptr;
    a.nut = nullptr;
    a.sum_part = nullptr;
    a.max_part = nullptr;
    return a;
}

void check_block() {
    if (scalar::slab_lanes_x() != WAVE || scalar::slab_rows() * WAVE != BLOCK)
        throw lbm_failure(LBM_E_INTERNAL, "the sub-grid kernel's block is not the block slab_grid lays its grid for");
}

}  // namespace

}  // namespace sgs
}  // namespace lbm

using namespace lbm;

// ---- D3Q19 engine: host side ----

void lbm3d_handle::sgs_set(int mode, float konst, const float *coef) {
    if (mode == LBM_SGS_OFF) {
        sgs_clear();
        return;
    }
    float cmin, cmax;
    sgs::check_model(mode, konst, coef, (long long)p.nx * p.ny * p.nz, cmin, cmax);
    need_whole_domain("sub-grid model");
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    sgs::make_state(sgs, slabs[0].dev, mode, coef ? 0.f : konst, coef, p.nx, (long long)p.ny * p.nz, cmin, cmax);
}

void lbm3d_handle::sgs_clear() { sgs::release(sgs); }

// Every slab's current lattice, then the ghost planes as after load_cells (refresh), exactly as after the
// forcing zones.
void lbm3d_handle::sgs_apply(float steps, double *stats) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice for the sub-grid model to act on");
    sgs::check_steps(steps);
    if (stats) std::fill(stats, stats + 3, 0.0);
    if (steps == 0.f || !sgs) return;
    const sgs::Model m = sgs::make_model(sgs->mode, p.omega, steps);
    sgs::check_rates(m, sgs->cmin, sgs->cmax);
    sgs::check_block();
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    const hipStream_t st = slabs[0].s_comp;
    double sum[2] = {0.0, 0.0};
    float max[1] = {0.f};
    for (const auto &s : slabs) {
        sgs::Sgs3 a = sgs::slab_args(slab_edit(s), s, p.ny, *sgs, m);
        const dim3 grid = scalar::slab_grid(a);
        if (stats) {
            const BlockPartials<2, 1> part((size_t)grid.x * grid.y * grid.z);
            a.sum_part = part.sums();
            a.max_part = part.maxima();
            sgs::launch_filter(a, true, false, grid, st);
            HIP_CHECK(hipStreamSynchronize(st));
            part.fold(sum, max);
        } else {
            sgs::launch_filter(a, false, false, grid, st);
        }
    }
    HIP_CHECK(hipStreamSynchronize(st));
    refresh();
    if (stats) {
        stats[0] = sum[0];
        stats[1] = sum[1];
        stats[2] = (double)max[0];
    }
}

// nu_add of an application with n = 1 into float[nz][ny][nx], staged and copied out as lbm3d_store_stress
void lbm3d_handle::sgs_store_nut(float *nut) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take the eddy viscosity from");
    if (!nut) throw lbm_failure(LBM_E_INVALID, "sub-grid model: NULL output");
    if (!sgs) {
        std::fill(nut, nut + (size_t)p.nx * p.ny * p.nz, 0.f);
        return;
    }
    const sgs::Model m = sgs::make_model(sgs->mode, p.omega, 1.f);
    sgs::check_block();
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    const hipStream_t st = slabs[0].s_comp;
    const lbm3d_box whole{0, 0, 0, p.nx, p.ny, p.nz};
    float *const out[1] = {nut};
    for (const auto &s : slabs) {
        sgs::Sgs3 a = sgs::slab_args(slab_edit(s), s, p.ny, *sgs, m);
        const size_t rows = (size_t)a.by * a.bz;
        const PlanarStage stage(1, rows * a.sp);
        a.nut = stage.field(0);
        sgs::launch_filter(a, false, true, scalar::slab_grid(a), st);
        HIP_CHECK(hipStreamSynchronize(st));
        stage.copy_out(out, 1, box_span(whole, s.z0), (size_t)a.sp, (size_t)p.nx, rows);
    }
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm3d_sgs_set(lbm3d_handle *h, int32_t mode, float konst, const float *coef) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->sgs_set(mode, konst, coef); });
}

int lbm3d_sgs_apply(lbm3d_handle *h, float steps, double stats[3]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->sgs_apply(steps, stats); });
}

int lbm3d_sgs_store_nut(lbm3d_handle *h, float *nut) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->sgs_store_nut(nut); });
}

int lbm3d_sgs_filter_ref(int32_t nx, int32_t ny, int32_t nz, const uint8_t *obst, float *cells, float omega,
                         int32_t mode, float konst, const float *coef, float steps, float *nut) {
    sgs::Model m;
    if (!sgs::ref_args_ok(nx, ny, nz, obst, cells, omega, mode, konst, coef, steps, m)) return LBM_E_INVALID;
    const size_t n = (size_t)nx * ny * nz;
    if (nut) std::fill(nut, nut + n, 0.f);
    if (steps == 0.f) return LBM_OK;
    for (size_t i = 0; i < n; ++i) {
        float *c = cells + i * Q3;
        float cc[Q3], q[Q3], d, nu;
        for (int j = 0; j < Q3; ++j) cc[j] = c[j];
        const bool idle = sgs::filter3(cc, obst[i] != 0, m, coef ? coef[i] : konst, q, d, nu);
        for (int j = 0; j < Q3; ++j) c[j] = sgs::rescaled(cc[j], q[j], d, idle);
        if (nut) nut[i] = nu;
    }
    return LBM_OK;
}

}  // extern "C"
