// lbm3d_fields.hip -- macroscopic fields and lattice statistics of the D3Q19
// engine on the device (include/lbm3d_fields_hip.h: lbm3d_store_fields,
// lbm3d_store_fields_box, lbm3d_field_stats): u_x, u_y, u_z, |u| and pressure
// of the current lattice, from each cell's 19 stored populations, without
// moving them to the host.  The kernel, then the engine's host side.
//
// Memory-bound: 77 B read (19 populations + the obstacle byte) and at most
// 20 B written per cell, no reuse, no LDS staging.  A box at least 4 cells
// wide whose x origin is a multiple of 4 (every full-row box: the whole
// domain, z- and y-normal planes) gives one lane four consecutive cells of a
// row (Box3View::quad) by the access path of lbm_quad.hpp: nineteen 16-B loads
// and up to five 16-B stores into staging rows padded to 4 floats; the last
// bx % 4 cells of a row go one at a time.  Other boxes take one cell per
// lane and stage unpadded rows.  A block is 64 lanes along x by 4 rows;
// blockIdx.y / .z walk rows and planes, so no index is ever divided and the
// float offsets are formed in 64 bits (512^3 x 19 floats exceeds 2^31).
//
// Arithmetic: IEEE fp32, the expressions and order of oracle/lbm_oracle3d.c
// cell3d, no contraction (-ffp-contract=off), correctly rounded divide and
// sqrt (hipcc default): the fields equal the host's bit for bit.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "lbm3d_cell_macro.hpp"
#include "lbm3d_engine.hpp"
#include "lbm_quad.hpp"

namespace lbm {

namespace {

constexpr int F3Q = 19;
constexpr int F3X = 64, F3Y = 4;  // block: 64 lanes along x (one wave) x 4 rows
// blocks a launch aims for (planes beyond are strided over): bounds the partials the host folds per slab
constexpr int F3_TARGET_BLOCKS = 16384;

__device__ __forceinline__ Cell3Macro cell3_dispatch(const float (&s)[F3Q], bool blocked, float obst_pressure,
                                                     bool want_v, bool want_u, float &rho) {
    if (want_u) return cell3_macro<true, true>(s, blocked, obst_pressure, rho);
    if (want_v) return cell3_macro<true, false>(s, blocked, obst_pressure, rho);
    return cell3_macro<false, false>(s, blocked, obst_pressure, rho);
}

}  // namespace

// STATS: block b (x fastest, then y, then z) also writes mass[b] = fp64 sum of
// the fp32 densities of its cells (obstacle cells included) and umax[b] = the
// largest |u| of its fluid cells, folded in a fixed order (no atomics).
template <bool STATS>
__global__ __launch_bounds__(F3X *F3Y) void macroscopic_fields3d(Fields3Args a) {
    const bool quad = a.quad != 0;      // the lane's four cells are one aligned 16 B of every speed row
    const int cpl = quad ? 4 : 1;       // cells per lane
    const int tx = threadIdx.x & (F3X - 1), ty = threadIdx.x / F3X;
    const int x = (blockIdx.x * F3X + tx) * cpl;  // box-local
    const bool want_v = STATS || a.ux || a.uy || a.uz || a.speed;
    const bool want_u = STATS || a.speed;
    const bool obst_word = (a.nx & 3) == 0;  // every quad's four obstacle bytes are one aligned word
    double mass = 0.0;
    float umax = 0.f;
    if (x < a.bx) {
        for (int z = blockIdx.z; z < a.bz; z += gridDim.z) {
            for (int y = blockIdx.y * F3Y + ty; y < a.by; y += gridDim.y * F3Y) {
                const long long lz = a.z0 + z, ly = a.y0 + y;
                const float *src = a.o + lz * a.PL + ly * a.px + (a.x0 + x);
                const uint8_t *ob = a.obst + (lz * a.ny + ly) * a.nx + (a.x0 + x);
                const long long so = ((long long)z * a.by + y) * a.sp + x;
                if (quad && x + 4 <= a.bx) {
                    float4 v[F3Q];
                    load_quad<F3Q>(src, a.KS, v);
                    const unsigned bits = quad_map_bytes(ob, obst_word);
                    Cell3Macro m[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float s[F3Q];
                        quad_cell<F3Q>(v, i, s);
                        const bool blocked = ((bits >> (8 * i)) & 0xffu) != 0;
                        float rho;
                        m[i] = cell3_dispatch(s, blocked, a.obst_pressure, want_v, want_u, rho);
                        if (STATS) {
                            mass += (double)rho;
                            if (!blocked) umax = fmaxf(umax, m[i].u);
                        }
                    }
                    if (a.ux) *reinterpret_cast<float4 *>(a.ux + so) = make_float4(m[0].ux, m[1].ux, m[2].ux, m[3].ux);
                    if (a.uy) *reinterpret_cast<float4 *>(a.uy + so) = make_float4(m[0].uy, m[1].uy, m[2].uy, m[3].uy);
                    if (a.uz) *reinterpret_cast<float4 *>(a.uz + so) = make_float4(m[0].uz, m[1].uz, m[2].uz, m[3].uz);
                    if (a.speed) *reinterpret_cast<float4 *>(a.speed + so) = make_float4(m[0].u, m[1].u, m[2].u, m[3].u);
                    if (a.pressure)
                        *reinterpret_cast<float4 *>(a.pressure + so) =
                            make_float4(m[0].pressure, m[1].pressure, m[2].pressure, m[3].pressure);
                } else {
                    // one cell per lane, or the ragged tail of a row: its last bx % 4 cells, one at a time
                    for (int i = 0; i < cpl && x + i < a.bx; ++i) {
                        float s[F3Q];
                        load_cell<F3Q>(src, a.KS, i, s);
                        const bool blocked = ob[i] != 0;
                        float rho;
                        const Cell3Macro m = cell3_dispatch(s, blocked, a.obst_pressure, want_v, want_u, rho);
                        if (STATS) {
                            mass += (double)rho;
                            if (!blocked) umax = fmaxf(umax, m.u);
                        }
                        if (a.ux) a.ux[so + i] = m.ux;
                        if (a.uy) a.uy[so + i] = m.uy;
                        if (a.uz) a.uz[so + i] = m.uz;
                        if (a.speed) a.speed[so + i] = m.u;
                        if (a.pressure) a.pressure[so + i] = m.pressure;
                    }
                }
            }
        }
    }
    if (STATS) {
        double s[1] = {mass};
        float m[1] = {umax};
        const long long b = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        // a row of the block is a wave
        fold_block<F3Y>(s, m, b, (long long)gridDim.x * gridDim.y * gridDim.z, a.mass_part, a.umax_part);
    }
}

namespace {

dim3 fields3d_grid(const Fields3Args &a) {
    const int cpl = a.quad ? 4 : 1;
    const long long lanes = ((long long)a.bx + cpl - 1) / cpl;
    const long long gx = (lanes + F3X - 1) / F3X;
    const long long gy = std::min<long long>(((long long)a.by + F3Y - 1) / F3Y, 65535);
    const long long gz = std::max<long long>(1, std::min<long long>(std::min(a.bz, 65535), F3_TARGET_BLOCKS / (gx * gy)));
    return dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
}

}  // namespace

int fields3d_blocks(const Fields3Args &a) {
    const dim3 g = fields3d_grid(a);
    return (int)(g.x * g.y * g.z);
}

hipError_t launch_macroscopic_fields3d(const Fields3Args &a, bool stats, hipStream_t s) {
    const dim3 g = fields3d_grid(a);
    if (stats)
        hipLaunchKernelGGL(macroscopic_fields3d<true>, g, dim3(F3X * F3Y), 0, s, a);
    else
        hipLaunchKernelGGL(macroscopic_fields3d<false>, g, dim3(F3X * F3Y), 0, s, a);
    return hipGetLastError();
}

}  // namespace lbm

// ---- D3Q19 engine: host side ----

using namespace lbm;

// the cells [x0, x0+bx) x [y0, y0+by) x [z0, z0+bz) of slab s (z0 slab-local)
Box3View lbm3d_handle::box_view(const Slab &s, int x0, int y0, int z0, int bx, int by, int bz) const {
    const int quad = (x0 % 4 == 0 && bx >= 4) ? 1 : 0;  // every full-row box of a domain >= 4 cells wide
    return Box3View{s.o[s.cur], s.obst, PL, KS, px, p.nx, p.ny, x0, y0, z0, bx, by, bz,
                    quad, quad ? (bx + 3) / 4 * 4 : bx, p.density * (1.f / 3.f)};
}

void lbm3d_handle::check_box(const lbm3d_box &b) const {
    if (b.nx <= 0 || b.ny <= 0 || b.nz <= 0 || b.x0 < 0 || b.y0 < 0 || b.z0 < 0 ||
        (long long)b.x0 + b.nx > p.nx || (long long)b.y0 + b.ny > p.ny || (long long)b.z0 + b.nz > p.nz)
        throw lbm_failure(LBM_E_INVALID, "box must be non-empty and inside the domain");
}

// the planes [zlo, zhi) (global) of box b that lie in slab s; false: none
bool lbm3d_handle::slab_planes(const Slab &s, const lbm3d_box &b, int &zlo, int &zhi) const {
    zlo = std::max(b.z0, s.z0);
    zhi = std::min(b.z0 + b.nz, s.z0 + s.nzs);
    return zlo < zhi;
}

// u_x, u_y, u_z, |u|, pressure of the box's cells into the packed planar
// host arrays float[b.nz][b.ny][b.nx] (host[i] NULL: field i is neither
// computed nor staged).  Slab by slab: the part of the box inside the slab
// is staged on its device (requested fields x cells; rows padded to 4
// floats on the 16-B path) and copied to its planes of the host arrays.
void lbm3d_handle::store_fields_box(const lbm3d_box &b, float *const (&host)[5]) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive fields from");
    check_box(b);
    const int want = count_wanted(host, 5);
    if (want == 0) return;
    sync_all();
    for (auto &s : slabs) {
        int zlo, zhi;
        if (!slab_planes(s, b, zlo, zhi)) continue;
        HIP_CHECK(hipSetDevice(s.dev));
        Fields3Args a{box_view(s, b.x0, b.y0, zlo - s.z0, b.nx, b.ny, zhi - zlo)};
        const size_t rows = (size_t)a.by * a.bz;
        const PlanarStage stage(want, rows * a.sp);
        float **dev[5] = {&a.ux, &a.uy, &a.uz, &a.speed, &a.pressure};
        for (int i = 0, n = 0; i < 5; ++i)
            if (host[i]) *dev[i] = stage.field(n++);
        HIP_CHECK(launch_macroscopic_fields3d(a, false, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(host, 5, box_span(b, zlo), (size_t)a.sp, (size_t)b.nx, rows);
    }
}

// Total mass (fp64 sum of every local cell's fp32 density) and the largest
// |u| over the local fluid cells, from the kernel's per-block partials
// (BlockPartials, lbm_diag_host.hpp), slab after slab.
void lbm3d_handle::field_stats(double *mass, float *max_speed) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!mass && !max_speed) return;
    sync_all();
    double total[1] = {0.0};
    float umax[1] = {0.f};
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        Fields3Args a{box_view(s, 0, 0, 0, p.nx, p.ny, s.nzs)};
        const BlockPartials<1, 1> part((size_t)fields3d_blocks(a));
        a.mass_part = part.sums();
        a.umax_part = part.maxima();
        HIP_CHECK(launch_macroscopic_fields3d(a, true, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        part.fold(total, umax);
    }
    if (mass) *mass = total[0];
    if (max_speed) *max_speed = umax[0];
}
