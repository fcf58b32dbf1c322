// lbm_sgs.hip -- the sub-grid model of the D2Q9 engine (the lbm_sgs_*
// functions of include/lbm_sgs_hip.h): the kernel that rescales the stored
// non-equilibrium part of every cell of one sub-domain, the engine's host
// side, the extern "C" functions and the host-only restatement
// lbm_sgs_filter_ref.
//
// The kernel.  A streaming read-modify-write of the current flow lattice over
// the cells of one sub-domain, memory-bound: per cell the nine populations
// read (36 B) and written (36 B) and the obstacle byte, 73 B; a coefficient
// plane adds 4 B.  The forcing zones' shape: one lane takes four consecutive
// cells of a row on the sub-domain's quad grid, 16-B loads and stores of the
// nine planes (and a 16-B load of the coefficient plane, which lies on the
// same grid: lbm_sgs.hpp), the obstacle bytes through quad_map_bytes.  The
// ragged tail of a row and sub-domains whose x origin is no multiple of 4 go
// one cell at a time.  A lane needs only its own cells and owns what it
// writes: no LDS, no atomics, no cross-lane move, no race in place -- except,
// in the forms that return the statistics, the fixed-order fold of the block's
// sums (fold_block).  Ghost cells and pad columns are not touched.
//
// Four compiled forms edit the lattice: the coefficient as a kernel argument
// or from the plane, each with and without the statistics.  Two more (NUT)
// write nu_add to a staging array and leave the lattice alone
// (lbm_sgs_store_nut).
//
// Arithmetic: IEEE fp32, as the header writes it, no contraction
// (-ffp-contract=off).

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_sgs.hpp"
#include "lbm_sgs_hip.h"

namespace lbm {
namespace sgs {

// One sub-domain's lattice, writable; the launch covers all of it.
struct Sgs2 : LatticeEdit {
    int quad;  // the sub-domain's x origin is a multiple of 4: the 16-B path
    Model m;
    float konst;
    const float *coef;  // the coefficient of the sub-domain's cell (x, y) at coef[y * cp + x]; PLANE forms
    int cp;
    float *nut;        // NUT forms: float[h][sp]
    double *sum_part;  // statistics forms: [2][blocks]
    float *max_part;   // [1][blocks]
};

namespace {

template <bool PLANE, bool STATS, bool NUT>
__device__ __forceinline__ void filter_one(const Sgs2 &a, int x, int y, Acc &acc) {
    float *f = a.e + (long long)y * a.pitch + x;
    float c[Q], q[Q], d, nut;
    load_cell<Q>(f, a.plane, 0, c);
    const bool blocked = a.obst[(long long)y * a.w + x] != 0;
    const float k = PLANE ? a.coef[(long long)y * a.cp + x] : a.konst;
    const bool idle = filter2(c, blocked, a.m, k, q, d, nut);
    if (NUT) {
        a.nut[(long long)y * a.sp + x] = nut;
    } else {
#pragma unroll
        for (int j = 0; j < Q; ++j) f[j * a.plane] = rescaled(c[j], q[j], d, idle);
    }
    if (STATS) acc.add(idle, nut);
}

}  // namespace

template <bool PLANE, bool STATS, bool NUT>
__global__ __launch_bounds__(BLOCK) void sgs_filter(Sgs2 a) {
    const int qpr = (a.w + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * a.h;
    const bool obst_word = (a.w & 3) == 0;
    Acc acc;
    for (long long t = (long long)blockIdx.x * BLOCK + threadIdx.x; t < total; t += (long long)gridDim.x * BLOCK) {
        const int y = (int)(t / qpr);
        const int x = (int)(t - (long long)y * qpr) << 2;
        if (a.quad && x + 4 <= a.w) {
            float *f = a.e + (long long)y * a.pitch + x;
            float4 v[Q];
            load_quad<Q>(f, a.plane, v);
            const unsigned bits = quad_map_bytes(a.obst + (long long)y * a.w + x, obst_word);
            float4 kq = make_float4(a.konst, a.konst, a.konst, a.konst);
            if (PLANE) kq = *reinterpret_cast<const float4 *>(a.coef + (long long)y * a.cp + x);
            float o[Q][4], nu[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q], q[Q], d;
                quad_cell<Q>(v, i, c);
                const bool idle = filter2(c, ((bits >> (8 * i)) & 0xffu) != 0, a.m, pick(kq, i), q, d, nu[i]);
                if (!NUT) {
#pragma unroll
                    for (int j = 0; j < Q; ++j) o[j][i] = rescaled(c[j], q[j], d, idle);
                }
                if (STATS) acc.add(idle, nu[i]);
            }
            if (NUT) {
                *reinterpret_cast<float4 *>(a.nut + (long long)y * a.sp + x) = make_float4(nu[0], nu[1], nu[2], nu[3]);
            } else {
#pragma unroll
                for (int k = 0; k < Q; ++k)
                    *reinterpret_cast<float4 *>(f + k * a.plane) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
            }
        } else {
            // the ragged tail of a row, or a sub-domain off the alignment
            for (int i = 0; i < 4; ++i)
                if (x + i < a.w) filter_one<PLANE, STATS, NUT>(a, x + i, y, acc);
        }
    }
    if (STATS) {
        double s[2] = {acc.cells, acc.sum};
        float m[1] = {acc.max};
        fold_block<BLOCK / 64>(s, m, blockIdx.x, gridDim.x, a.sum_part, a.max_part);
    }
}

namespace {

template <bool PLANE>
void launch_filter(const Sgs2 &a, bool stats, bool nut, int nb, hipStream_t st) {
    if (nut)
        hipLaunchKernelGGL((sgs_filter<PLANE, false, true>), dim3(nb), dim3(BLOCK), 0, st, a);
    else if (stats)
        hipLaunchKernelGGL((sgs_filter<PLANE, true, false>), dim3(nb), dim3(BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((sgs_filter<PLANE, false, false>), dim3(nb), dim3(BLOCK), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

void launch_filter(const Sgs2 &a, bool stats, bool nut, int nb, hipStream_t st) {
    if (a.coef)
        launch_filter<true>(a, stats, nut, nb, st);
    else
        launch_filter<false>(a, stats, nut, nb, st);
}

}  // namespace

}  // namespace sgs
}  // namespace lbm

// ---- D2Q9 engine: host side ----

void lbm_handle::sgs_set(int mode, float konst, const float *coef) {
    if (mode == LBM_SGS_OFF) {
        sgs_clear();
        return;
    }
    float cmin, cmax;
    sgs::check_model(mode, konst, coef, (long long)p.nx * p.ny, cmin, cmax);
    need_whole_domain("sub-grid model");
    sync_all();
    set_device(subs[0]);
    sgs::make_state(sgs, subs[0].dev, mode, coef ? 0.f : konst, coef, p.nx, p.ny, cmin, cmax);
}

void lbm_handle::sgs_clear() { sgs::release(sgs); }

// the arguments of sub-domain s for the handle's model and n steps, the outputs null
lbm::sgs::Sgs2 lbm_handle::sgs_args(const Sub &s, const sgs::Model &m) const {
    sgs::Sgs2 a{lattice_edit(s)};
    a.quad = s.rect.x0 % 4 == 0 ? 1 : 0;
    a.m = m;
    a.konst = sgs->konst;
    a.cp = sgs->cp;
    a.coef = sgs->plane ? sgs->plane + ((long long)s.rect.y0 * sgs->cp + s.rect.x0) : nullptr;
    a.nut = nullptr;
    a.sum_part = nullptr;
    a.max_part = nullptr;
    return a;
}

// Every sub-domain's current lattice.  The ghost ring is left to the next run, which rebuilds it first
// (ring_stale), exactly as after the forcing zones.
void lbm_handle::sgs_apply(float steps, double *stats) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice for the sub-grid model to act on");
    sgs::check_steps(steps);
    if (stats) std::fill(stats, stats + 3, 0.0);
    if (steps == 0.f || !sgs) return;
    const sgs::Model m = sgs::make_model(sgs->mode, p.omega, steps);
    sgs::check_rates(m, sgs->cmin, sgs->cmax);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    double sum[2] = {0.0, 0.0};
    float max[1] = {0.f};
    for (const auto &s : subs) {
        sgs::Sgs2 a = sgs_args(s, m);
        const int nb = fields_blocks(s.w, s.h);
        if (stats) {
            const BlockPartials<2, 1> part((size_t)nb);
            a.sum_part = part.sums();
            a.max_part = part.maxima();
            timed(s0, s0.s_comp, "sgs", [&] { sgs::launch_filter(a, true, false, nb, s0.s_comp); });
            ring_stale = true;
            HIP_CHECK(hipStreamSynchronize(s0.s_comp));
            part.fold(sum, max);
        } else {
            timed(s0, s0.s_comp, "sgs", [&] { sgs::launch_filter(a, false, false, nb, s0.s_comp); });
            ring_stale = true;
        }
    }
    HIP_CHECK(hipStreamSynchronize(s0.s_comp));
    prof_collect();
    if (stats) {
        stats[0] = sum[0];
        stats[1] = sum[1];
        stats[2] = (double)max[0];
    }
}

// nu_add of an application with n = 1 into float[ny][nx], staged and copied out as lbm_store_stress
void lbm_handle::sgs_store_nut(float *nut) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take the eddy viscosity from");
    if (!nut) throw lbm_failure(LBM_E_INVALID, "sub-grid model: NULL output");
    if (!sgs) {
        std::fill(nut, nut + (size_t)p.nx * p.ny, 0.f);
        return;
    }
    const sgs::Model m = sgs::make_model(sgs->mode, p.omega, 1.f);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    float *const out[1] = {nut};
    for (const auto &s : subs) {
        sgs::Sgs2 a = sgs_args(s, m);
        const PlanarStage stage(1, (size_t)a.sp * s.h);
        a.nut = stage.field(0);
        timed(s0, s0.s_comp, "sgs nut", [&] { sgs::launch_filter(a, false, true, fields_blocks(s.w, s.h), s0.s_comp); });
        HIP_CHECK(hipStreamSynchronize(s0.s_comp));
        stage.copy_out(out, 1, host_span(s, false, 0), (size_t)a.sp, (size_t)s.w, (size_t)s.h);
    }
    prof_collect();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm_sgs_set(lbm_handle *h, int32_t mode, float konst, const float *coef) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->sgs_set(mode, konst, coef); });
}

int lbm_sgs_apply(lbm_handle *h, float steps, double stats[3]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->sgs_apply(steps, stats); });
}

int lbm_sgs_store_nut(lbm_handle *h, float *nut) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->sgs_store_nut(nut); });
}

int lbm_sgs_filter_ref(int32_t nx, int32_t ny, const uint8_t *obst, float *cells, float omega, int32_t mode,
                       float konst, const float *coef, float steps, float *nut) {
    sgs::Model m;
    if (!sgs::ref_args_ok(nx, ny, 1, obst, cells, omega, mode, konst, coef, steps, m)) return LBM_E_INVALID;
    const size_t n = (size_t)nx * ny;
    if (nut) std::fill(nut, nut + n, 0.f);
    if (steps == 0.f) return LBM_OK;
    for (size_t i = 0; i < n; ++i) {
        float *c = cells + i * Q;
        float cc[Q], q[Q], d, nu;
        for (int j = 0; j < Q; ++j) cc[j] = c[j];
        const bool idle = sgs::filter2(cc, obst[i] != 0, m, coef ? coef[i] : konst, q, d, nu);
        for (int j = 0; j < Q; ++j) c[j] = sgs::rescaled(cc[j], q[j], d, idle);
        if (nut) nut[i] = nu;
    }
    return LBM_OK;
}

}  // extern "C"
