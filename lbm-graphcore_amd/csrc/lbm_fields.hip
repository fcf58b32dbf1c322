// lbm_fields.hip -- macroscopic fields and lattice statistics on the device
// (lbm_store_fields / lbm_field_stats): u_x, u_y, |u| and pressure of the
// current SoA lattice, exactly as lbmhost::macroscopic (host/lbm_host.hpp;
// writeResults, LatticeBoltzmannUtils.hpp:221-281) derives them from the AoS
// cells, without moving the nine populations to the host.  The kernel, then
// the D2Q9 engine's host side.
//
// Memory-bound: 37 B read (nine populations + the obstacle byte) and at most
// 16 B written per cell, no reuse, no LDS staging.  One lane takes four
// consecutive cells of a row by the access path of lbm_quad.hpp: nine 16-B
// loads and up to four 16-B stores; the last w % 4 cells of a row go one at a
// time.
//
// Arithmetic: IEEE fp32, evaluation order of the host function, no
// contraction (-ffp-contract=off), correctly rounded divide and sqrt (hipcc
// default): the fields equal the host's bit for bit.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm_cell_macro.hpp"
#include "lbm_engine.hpp"
#include "lbm_quad.hpp"

namespace lbm {

namespace {

// most blocks of a launch (grid-stride beyond): also the most partials the host folds per sub-domain
constexpr int FIELDS_MAX_BLOCKS = 8192;

}  // namespace

// Fields of the w x h interior of the lattice at origin a.o into the planar
// staging arrays float[h][sp] (sp = roundup(w, 4); a null array is neither
// computed nor stored).  STATS: block b also writes mass[b] = fp64 sum of
// the fp32 densities of its cells (obstacle cells included) and umax[b] = the
// largest |u| of its fluid cells, folded in a fixed order (no atomics).
template <bool STATS>
__global__ __launch_bounds__(BLOCK) void macroscopic_fields(FieldsArgs a) {
    const int qpr = (a.w + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * a.h;
    const bool want_v = STATS || a.ux || a.uy || a.speed;
    const bool want_u = STATS || a.speed;
    const bool obst_word = (a.w & 3) == 0;  // every quad's four obstacle bytes are one aligned word
    double mass = 0.0;
    float umax = 0.f;
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * BLOCK) {
        const int y = (int)(q / qpr);
        const int x = (int)(q - (long long)y * qpr) << 2;
        const float *src = a.o + (long long)y * a.pitch + x;
        const uint8_t *ob = a.obst + (long long)y * a.w + x;
        const long long so = (long long)y * a.sp + x;
        if (x + 4 <= a.w) {
            float4 v[Q];
            load_quad<Q>(src, a.plane, v);
            const unsigned bits = quad_map_bytes(ob, obst_word);
            CellMacro m[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q];
                quad_cell<Q>(v, i, c);
                const bool blocked = ((bits >> (8 * i)) & 0xffu) != 0;
                float rho;
                if (want_u)
                    m[i] = cell_macro<true, true>(c, blocked, a.obst_pressure, rho);
                else if (want_v)
                    m[i] = cell_macro<true, false>(c, blocked, a.obst_pressure, rho);
                else
                    m[i] = cell_macro<false, false>(c, blocked, a.obst_pressure, rho);
                if (STATS) {
                    mass += (double)rho;
                    if (!blocked) umax = fmaxf(umax, m[i].u);
                }
            }
            if (a.ux) *reinterpret_cast<float4 *>(a.ux + so) = make_float4(m[0].ux, m[1].ux, m[2].ux, m[3].ux);
            if (a.uy) *reinterpret_cast<float4 *>(a.uy + so) = make_float4(m[0].uy, m[1].uy, m[2].uy, m[3].uy);
            if (a.speed) *reinterpret_cast<float4 *>(a.speed + so) = make_float4(m[0].u, m[1].u, m[2].u, m[3].u);
            if (a.pressure)
                *reinterpret_cast<float4 *>(a.pressure + so) =
                    make_float4(m[0].pressure, m[1].pressure, m[2].pressure, m[3].pressure);
        } else {
            // ragged tail of a row: the last w % 4 cells, one at a time
            for (int i = 0; x + i < a.w; ++i) {
                float c[Q];
                load_cell<Q>(src, a.plane, i, c);
                const bool blocked = ob[i] != 0;
                float rho;
                CellMacro m;
                if (want_u)
                    m = cell_macro<true, true>(c, blocked, a.obst_pressure, rho);
                else if (want_v)
                    m = cell_macro<true, false>(c, blocked, a.obst_pressure, rho);
                else
                    m = cell_macro<false, false>(c, blocked, a.obst_pressure, rho);
                if (STATS) {
                    mass += (double)rho;
                    if (!blocked) umax = fmaxf(umax, m.u);
                }
                if (a.ux) a.ux[so + i] = m.ux;
                if (a.uy) a.uy[so + i] = m.uy;
                if (a.speed) a.speed[so + i] = m.u;
                if (a.pressure) a.pressure[so + i] = m.pressure;
            }
        }
    }
    if (STATS) {
        double s[1] = {mass};
        float m[1] = {umax};
        fold_block<BLOCK / 64>(s, m, blockIdx.x, gridDim.x, a.mass_part, a.umax_part);
    }
}

int fields_blocks(int w, int h) {
    const long long quads = (long long)((w + 3) / 4) * h;
    return (int)std::max<long long>(1, std::min<long long>(FIELDS_MAX_BLOCKS, (quads + BLOCK - 1) / BLOCK));
}

// stats = false: the requested fields; stats = true: the per-block partials
// (mass_part / umax_part hold fields_blocks(w, h) entries each)
hipError_t launch_macroscopic_fields(const FieldsArgs &a, bool stats, hipStream_t s) {
    const int blocks = fields_blocks(a.w, a.h);
    if (stats)
        hipLaunchKernelGGL(macroscopic_fields<true>, dim3(blocks), dim3(BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(macroscopic_fields<false>, dim3(blocks), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace lbm

// ---- D2Q9 engine: host side ----

LatticeView lbm_handle::lattice_view(const Sub &s) const {
    return LatticeView{s.o[s.cur], s.obst, s.plane, s.pitch, s.w, s.h, (int)round_up(s.w, 4), p.density * (1.f / 3.f)};
}

// u_x, u_y, |u|, pressure of the current lattice into planar
// host arrays: float[ny][nx] with each sub-domain at its rectangle, or (local)
// the sub-domains' float[h][w] blocks packed in lbm_local_rects order.  A
// NULL field is neither computed nor staged.
void lbm_handle::store_fields(float *ux, float *uy, float *speed, float *pressure, bool local) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive fields from");
    float *const host[4] = {ux, uy, speed, pressure};
    const int want = count_wanted(host, 4);
    if (want == 0) return;
    sync_all();
    prof_drop();
    size_t packed = 0;  // local: cells of the sub-domains before this one
    for (auto &s : subs) {
        set_device(s);
        FieldsArgs a{lattice_view(s)};
        const PlanarStage stage(want, (size_t)a.sp * s.h);
        float **dev[4] = {&a.ux, &a.uy, &a.speed, &a.pressure};
        for (int i = 0, n = 0; i < 4; ++i)
            if (host[i]) *dev[i] = stage.field(n++);
        timed(s, s.s_comp, "macroscopic_fields", [&] { HIP_CHECK(launch_macroscopic_fields(a, false, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(host, 4, host_span(s, local, packed), (size_t)a.sp, (size_t)s.w, (size_t)s.h);
        packed += (size_t)s.w * s.h;
    }
    prof_collect();
}

// Total mass (fp64 sum of every local cell's fp32 density) and the largest
// |u| over the local fluid cells, from the kernel's per-block partials
// (BlockPartials, lbm_diag_host.hpp).
void lbm_handle::field_stats(double *mass, float *max_speed) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!mass && !max_speed) return;
    sync_all();
    prof_drop();
    double total[1] = {0.0};
    float umax[1] = {0.f};
    for (auto &s : subs) {
        set_device(s);
        FieldsArgs a{lattice_view(s)};
        const BlockPartials<1, 1> part((size_t)fields_blocks(s.w, s.h));
        a.mass_part = part.sums();
        a.umax_part = part.maxima();
        timed(s, s.s_comp, "macroscopic_fields stats", [&] { HIP_CHECK(launch_macroscopic_fields(a, true, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        part.fold(total, umax);
    }
    prof_collect();
    if (mass) *mass = total[0];
    if (max_speed) *max_speed = umax[0];
}
