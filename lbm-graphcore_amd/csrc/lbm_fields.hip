// lbm_fields.hip -- macroscopic fields and lattice statistics on the device
// (lbm_store_fields / lbm_field_stats): u_x, u_y, |u| and pressure of the
// current SoA lattice, exactly as lbmhost::macroscopic (host/lbm_host.hpp;
// writeResults, LatticeBoltzmannUtils.hpp:221-281) derives them from the AoS
// cells, without moving the nine populations to the host.  The kernel, then
// the D2Q9 engine's host side.
//
// Memory-bound: 37 B read (nine populations + the obstacle byte) and at most
// 16 B written per cell, no reuse, no LDS staging.  One lane takes four
// consecutive cells of a row: the interior row start is 16-B aligned in both
// lattice layouts (xoff, plane and pitch are multiples of 4 floats), so that
// is nine 16-B loads and up to four 16-B stores.  The last w % 4 cells of a
// row take a scalar path.
//
// Arithmetic: IEEE fp32, evaluation order of the host function, no
// contraction (-ffp-contract=off), correctly rounded divide and sqrt (hipcc
// default): the fields equal the host's bit for bit.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm_cell_macro.hpp"
#include "lbm_engine.hpp"

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
#pragma unroll
            for (int k = 0; k < Q; ++k) v[k] = *reinterpret_cast<const float4 *>(src + k * a.plane);
            unsigned bits;
            if (obst_word)
                bits = *reinterpret_cast<const unsigned *>(ob);
            else
                bits = (unsigned)ob[0] | ((unsigned)ob[1] << 8) | ((unsigned)ob[2] << 16) | ((unsigned)ob[3] << 24);
            CellMacro m[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q];
#pragma unroll
                for (int k = 0; k < Q; ++k) c[k] = i == 0 ? v[k].x : i == 1 ? v[k].y : i == 2 ? v[k].z : v[k].w;
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
#pragma unroll
                for (int k = 0; k < Q; ++k) c[k] = src[k * a.plane + i];
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
        // lanes of a wave by shuffle, the block's four waves through LDS: fixed order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mass += __shfl_down(mass, off, 64);
            umax = fmaxf(umax, __shfl_down(umax, off, 64));
        }
        __shared__ double wmass[BLOCK / 64];
        __shared__ float wmax[BLOCK / 64];
        if ((threadIdx.x & 63) == 0) {
            wmass[threadIdx.x >> 6] = mass;
            wmax[threadIdx.x >> 6] = umax;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double ms = wmass[0];
            float mx = wmax[0];
            for (int i = 1; i < BLOCK / 64; ++i) {
                ms += wmass[i];
                mx = fmaxf(mx, wmax[i]);
            }
            a.mass_part[blockIdx.x] = ms;
            a.umax_part[blockIdx.x] = mx;
        }
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

FieldsArgs lbm_handle::fields_args(const Sub &s) const {
    FieldsArgs a{};
    a.o = s.o[s.cur];
    a.obst = s.obst;
    a.plane = s.plane;
    a.pitch = s.pitch;
    a.w = s.w;
    a.h = s.h;
    a.sp = (int)round_up(s.w, 4);
    a.obst_pressure = p.density * (1.f / 3.f);
    return a;
}

// u_x, u_y, |u|, pressure of the current lattice into planar
// host arrays: float[ny][nx] with each sub-domain at its rectangle, or (local)
// the sub-domains' float[h][w] blocks packed in lbm_local_rects order.  A
// NULL field is neither computed nor staged.
void lbm_handle::store_fields(float *ux, float *uy, float *speed, float *pressure, bool local) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive fields from");
    float *const host[4] = {ux, uy, speed, pressure};
    int want = 0;
    for (float *f : host) want += f ? 1 : 0;
    if (want == 0) return;
    sync_all();
    prof_drop();
    size_t packed = 0;  // local: cells of the sub-domains before this one
    for (auto &s : subs) {
        set_device(s);
        FieldsArgs a = fields_args(s);
        const size_t field_floats = (size_t)a.sp * s.h;
        const DeviceStage stage(sizeof(float) * field_floats * want);
        float **dev[4] = {&a.ux, &a.uy, &a.speed, &a.pressure};
        for (int i = 0, n = 0; i < 4; ++i)
            if (host[i]) *dev[i] = stage.as<float>() + field_floats * n++;
        timed(s, s.s_comp, "macroscopic_fields", [&] { HIP_CHECK(launch_macroscopic_fields(a, false, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        const size_t off = local ? packed : (size_t)s.rect.y0 * p.nx + s.rect.x0;
        const size_t pitch = sizeof(float) * (size_t)(local ? s.w : p.nx);
        for (int i = 0; i < 4; ++i)
            if (host[i])
                HIP_CHECK(hipMemcpy2D(host[i] + off, pitch, *dev[i], sizeof(float) * (size_t)a.sp,
                                      sizeof(float) * (size_t)s.w, (size_t)s.h, hipMemcpyDeviceToHost));
        packed += (size_t)s.w * s.h;
    }
    prof_collect();
}

// Total mass (fp64 sum of every local cell's fp32 density) and the largest
// |u| over the local fluid cells.  The kernel leaves per-block partials;
// they are folded here in block order, sub-domain after sub-domain, so the
// same lattice always gives the same bits.
void lbm_handle::field_stats(double *mass, float *max_speed) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!mass && !max_speed) return;
    sync_all();
    prof_drop();
    double total = 0.0;
    float umax = 0.f;
    for (auto &s : subs) {
        set_device(s);
        FieldsArgs a = fields_args(s);
        const int nb = fields_blocks(s.w, s.h);
        // [nb doubles | nb floats]
        const DeviceStage part((sizeof(double) + sizeof(float)) * (size_t)nb);
        std::vector<double> host((size_t)nb + ((size_t)nb + 1) / 2);  // the same block: doubles, then floats
        a.mass_part = part.as<double>();
        a.umax_part = reinterpret_cast<float *>(a.mass_part + nb);
        timed(s, s.s_comp, "macroscopic_fields stats", [&] { HIP_CHECK(launch_macroscopic_fields(a, true, s.s_comp)); });
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        HIP_CHECK(hipMemcpy(host.data(), part.get(), (sizeof(double) + sizeof(float)) * (size_t)nb, hipMemcpyDeviceToHost));
        std::vector<float> hu((size_t)nb);
        memcpy(hu.data(), host.data() + nb, sizeof(float) * (size_t)nb);
        for (int b = 0; b < nb; ++b) {
            total += host[(size_t)b];
            umax = std::max(umax, hu[(size_t)b]);
        }
    }
    prof_collect();
    if (mass) *mass = total;
    if (max_speed) *max_speed = umax;
}
