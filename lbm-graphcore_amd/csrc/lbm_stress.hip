// lbm_stress.hip -- strain rate and wall shear of the D2Q9 engine from the
// non-equilibrium second moment of each cell's own populations (the lbm_*
// functions of include/lbm_stress_hip.h).  The kernel, then the engine's host
// side.
//
// Cell-local: no neighbour is read, so nothing crosses a sub-domain border and
// any transport and world size works.  One memory-bound pass over the nine
// populations of the current side of the pair (origin / plane / pitch, either
// layout): 37 B read per cell, 4 B written per requested field, no LDS but the
// statistics' fold.  A lane takes four consecutive cells of a row (nine 16-B
// loads, lbm_quad.hpp; a float4 store per field) and ST_ITER such quads a
// block apart; the last w % 4 cells of a row go one at a time.
//
// Near-wall cells are a property of the obstacle map alone: the statistics
// read a class map (CLS_*) in place of the obstacle map, built on the host
// from the ghosted map at the first statistics call.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_stress.hpp"
#include "lbm_stress_hip.h"

namespace lbm {
namespace stress {

// STATS: no field is stored and a.obst is the class map; block b writes its
// partial sums and maxima over the fluid cells it owns (fold_block, lbm_quad.hpp).
template <bool STATS>
__global__ __launch_bounds__(ST_BLOCK) void neq_strain(StressArgs a) {
    const int qpr = (a.w + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * a.h;
    const bool obst_word = (a.w & 3) == 0;  // every quad's four map bytes are one aligned word
    double sum_s2 = 0.0, sum_wall = 0.0;
    float max_s = 0.f, max_wall = 0.f;
    const long long q0 = (long long)blockIdx.x * ST_BLOCK_QUADS + threadIdx.x;
    for (int j = 0; j < ST_ITER; ++j) {
        const long long q = q0 + (long long)j * ST_BLOCK;
        if (q >= total) break;
        const int y = (int)(q / qpr);
        const int x = (int)(q - (long long)y * qpr) << 2;
        const float *src = a.o + (long long)y * a.pitch + x;
        const uint8_t *ob = a.obst + (long long)y * a.w + x;
        const long long so = (long long)y * a.sp + x;
        if (x + 4 <= a.w) {
            float4 v[Q];
            // the store variant walks (12 SGPRs fewer), the stats variant indexes (2 VGPRs fewer): lbm_quad.hpp
            load_quad<Q, !STATS>(src, a.plane, v);
            const unsigned bits = quad_map_bytes(ob, obst_word);
            Strain2 s[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q];
                quad_cell<Q>(v, i, c);
                const unsigned cls = (bits >> (8 * i)) & 0xffu;
                const bool blocked = STATS ? cls == CLS_BLOCKED : cls != 0;
                s[i] = neq_strain2(c, blocked, a.coef);
                if (STATS && !blocked) {
                    sum_s2 += (double)s[i].s2;
                    max_s = fmaxf(max_s, s[i].strain);
                    if (cls == CLS_NEAR_WALL) {
                        sum_wall += (double)s[i].strain;
                        max_wall = fmaxf(max_wall, s[i].strain);
                    }
                }
            }
            if (!STATS) {
                if (a.out[0]) *reinterpret_cast<float4 *>(a.out[0] + so) = make_float4(s[0].sxx, s[1].sxx, s[2].sxx, s[3].sxx);
                if (a.out[1]) *reinterpret_cast<float4 *>(a.out[1] + so) = make_float4(s[0].sxy, s[1].sxy, s[2].sxy, s[3].sxy);
                if (a.out[2]) *reinterpret_cast<float4 *>(a.out[2] + so) = make_float4(s[0].syy, s[1].syy, s[2].syy, s[3].syy);
                if (a.out[3])
                    *reinterpret_cast<float4 *>(a.out[3] + so) =
                        make_float4(s[0].strain, s[1].strain, s[2].strain, s[3].strain);
            }
        } else {
            // ragged tail of a row: the last w % 4 cells, one at a time
            for (int i = 0; x + i < a.w; ++i) {
                float c[Q];
                load_cell<Q>(src, a.plane, i, c);
                const unsigned cls = ob[i];
                const bool blocked = STATS ? cls == CLS_BLOCKED : cls != 0;
                const Strain2 s = neq_strain2(c, blocked, a.coef);
                if (STATS && !blocked) {
                    sum_s2 += (double)s.s2;
                    max_s = fmaxf(max_s, s.strain);
                    if (cls == CLS_NEAR_WALL) {
                        sum_wall += (double)s.strain;
                        max_wall = fmaxf(max_wall, s.strain);
                    }
                }
                if (!STATS) {
                    if (a.out[0]) a.out[0][so + i] = s.sxx;
                    if (a.out[1]) a.out[1][so + i] = s.sxy;
                    if (a.out[2]) a.out[2][so + i] = s.syy;
                    if (a.out[3]) a.out[3][so + i] = s.strain;
                }
            }
        }
    }
    if (STATS) {
        double s[2] = {sum_s2, sum_wall};
        float m[2] = {max_s, max_wall};
        fold_block<ST_BLOCK / 64>(s, m, blockIdx.x, gridDim.x, a.sum_part, a.max_part);
    }
}

// blocks of a launch over w x h: also the partials a stats launch writes
int stress_blocks(int w, int h) {
    const long long quads = (long long)((w + 3) / 4) * h;
    return (int)((quads + ST_BLOCK_QUADS - 1) / ST_BLOCK_QUADS);
}

hipError_t launch_neq_strain(const StressArgs &a, bool stats, hipStream_t s) {
    const int blocks = stress_blocks(a.w, a.h);
    if (stats)
        hipLaunchKernelGGL(neq_strain<true>, dim3(blocks), dim3(ST_BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(neq_strain<false>, dim3(blocks), dim3(ST_BLOCK), 0, s, a);
    return hipGetLastError();
}

// class maps of a handle that asked for the statistics: per local sub-domain
// uint8[h][w] on its device, and the near-wall cells counted while building
struct State {
    std::vector<uint8_t *> cls;
    long long wall_cells = 0;
};

}  // namespace stress
}  // namespace lbm

// ---- D2Q9 engine: host side ----

using lbm::stress::StressArgs;

// the arguments of sub-domain s but the outputs; refuses omega = 1
StressArgs lbm_handle::stress_args(const Sub &s) const {
    StressArgs a{lattice_view(s)};
    a.coef = neq_strain_coef(p.omega);
    return a;
}

// Build the class maps at the first statistics call: the neighbours of a cell
// on a sub-domain border come from the ring of the ghosted obstacle map (the
// neighbour's cells, or the periodic image of the full domain).
void lbm_handle::stress_build() {
    if (stress) return;
    auto *st = new lbm::stress::State();
    stress = st;  // owned by the handle from here (stress_release)
    st->cls.assign(subs.size(), nullptr);
    try {
        for (size_t k = 0; k < subs.size(); ++k) {
            const Sub &s = subs[k];
            set_device(s);
            const int gw = s.w + 2 * og;
            std::vector<uint8_t> g((size_t)gw * (s.h + 2 * og));
            HIP_CHECK(hipMemcpy(g.data(), s.obst_g, g.size(), hipMemcpyDeviceToHost));
            std::vector<uint8_t> cls((size_t)s.w * s.h);
            for (int y = 0; y < s.h; ++y) {
                const uint8_t *row = g.data() + (size_t)(y + og) * gw + og;
                for (int x = 0; x < s.w; ++x) {
                    uint8_t c = lbm::stress::CLS_BLOCKED;
                    if (!row[x]) {
                        c = lbm::stress::CLS_FLUID;
                        for (int j = 0; j < 8; ++j)
                            if (row[x + DIR_Y[j] * gw + DIR_X[j]]) c = lbm::stress::CLS_NEAR_WALL;
                        if (c == lbm::stress::CLS_NEAR_WALL) ++st->wall_cells;
                    }
                    cls[(size_t)y * s.w + x] = c;
                }
            }
            // the kernel reads a quad's four bytes as one word: slack as the obstacle map's
            HIP_CHECK(hipMalloc(&st->cls[k], (size_t)round_up((long long)s.w * s.h + 16, 256)));
            HIP_CHECK(hipMemcpy(st->cls[k], cls.data(), cls.size(), hipMemcpyHostToDevice));
        }
    } catch (...) {
        stress_release();  // a later call builds again
        throw;
    }
}

void lbm_handle::stress_release() {
    if (!stress) return;
    for (size_t k = 0; k < stress->cls.size() && k < subs.size(); ++k)
        if (stress->cls[k] && hipSetDevice(subs[k].dev) == hipSuccess) (void)hipFree(stress->cls[k]);
    delete stress;
    stress = nullptr;
}

// sxx, sxy, syy, strain of the current lattice into planar host arrays
// (out[LBM_STRESS_*]; layout rules of store_fields).  A NULL entry is neither
// stored nor staged.
void lbm_handle::store_stress(float *const *out, bool local) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive the strain rate from");
    const int want = count_wanted(out, LBM_STRESS_FIELDS);
    if (want == 0) return;
    stress_args(subs.at(0));  // omega = 1 is refused before anything is launched or written
    sync_all();
    prof_drop();
    size_t packed = 0;  // local: cells of the sub-domains before this one
    for (auto &s : subs) {
        set_device(s);
        StressArgs a = stress_args(s);
        const PlanarStage stage(want, (size_t)a.sp * s.h);
        for (int i = 0, n = 0; i < LBM_STRESS_FIELDS; ++i)
            if (out[i]) a.out[i] = stage.field(n++);
        timed(s, s.s_comp, "neq_strain", [&] { HIP_CHECK(stress::launch_neq_strain(a, false, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(out, LBM_STRESS_FIELDS, host_span(s, local, packed), (size_t)a.sp, (size_t)s.w, (size_t)s.h);
        packed += (size_t)s.w * s.h;
    }
    prof_collect();
}

// Sum of S:S (fp64) and the largest strain over the local fluid cells; count,
// fp64 sum and maximum of the strain over the near-wall ones, from the
// kernel's per-block partials (BlockPartials, lbm_diag_host.hpp).
void lbm_handle::stress_stats(double *sum_s2, float *max_strain, int64_t *wall_cells, double *sum_wall_strain,
                              float *max_wall_strain) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!sum_s2 && !max_strain && !wall_cells && !sum_wall_strain && !max_wall_strain) return;
    stress_args(subs.at(0));
    sync_all();
    stress_build();
    prof_drop();
    double sum[2] = {0.0, 0.0};  // s2, near-wall strain
    float max[2] = {0.f, 0.f};   // strain, near-wall strain
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        set_device(s);
        StressArgs a = stress_args(s);
        a.obst = stress->cls[k];
        const BlockPartials<2, 2> part((size_t)stress::stress_blocks(s.w, s.h));
        a.sum_part = part.sums();
        a.max_part = part.maxima();
        timed(s, s.s_comp, "neq_strain stats", [&] { HIP_CHECK(stress::launch_neq_strain(a, true, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        part.fold(sum, max);
    }
    prof_collect();
    if (sum_s2) *sum_s2 = sum[0];
    if (max_strain) *max_strain = max[0];
    if (wall_cells) *wall_cells = stress->wall_cells;
    if (sum_wall_strain) *sum_wall_strain = sum[1];
    if (max_wall_strain) *max_wall_strain = max[1];
}
