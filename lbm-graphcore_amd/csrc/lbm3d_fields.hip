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
// row (Fields3Args::quad): lattice rows start 16-B aligned (px is a multiple
// of 16 floats, KS and PL multiples of 4), so that is nineteen 16-B loads and
// up to five 16-B stores into staging rows padded to 4 floats; the last
// bx % 4 cells of a row take a scalar path.  Other boxes take one cell per
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
#pragma unroll
                    for (int k = 0; k < F3Q; ++k) v[k] = *reinterpret_cast<const float4 *>(src + k * a.KS);
                    unsigned bits;
                    if (obst_word)
                        bits = *reinterpret_cast<const unsigned *>(ob);
                    else
                        bits = (unsigned)ob[0] | ((unsigned)ob[1] << 8) | ((unsigned)ob[2] << 16) |
                               ((unsigned)ob[3] << 24);
                    Cell3Macro m[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float s[F3Q];
#pragma unroll
                        for (int k = 0; k < F3Q; ++k)
                            s[k] = i == 0 ? v[k].x : i == 1 ? v[k].y : i == 2 ? v[k].z : v[k].w;
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
#pragma unroll
                        for (int k = 0; k < F3Q; ++k) s[k] = src[k * a.KS + i];
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
        // lanes of a wave by shuffle, the block's four waves through LDS: fixed order
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mass += __shfl_down(mass, off, 64);
            umax = fmaxf(umax, __shfl_down(umax, off, 64));
        }
        __shared__ double wmass[F3Y];
        __shared__ float wmax[F3Y];
        if (tx == 0) {
            wmass[ty] = mass;
            wmax[ty] = umax;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double ms = wmass[0];
            float mx = wmax[0];
            for (int i = 1; i < F3Y; ++i) {
                ms += wmass[i];
                mx = fmaxf(mx, wmax[i]);
            }
            const long long b = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
            a.mass_part[b] = ms;
            a.umax_part[b] = mx;
        }
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
Fields3Args lbm3d_handle::fields_args(const Slab &s, int x0, int y0, int z0, int bx, int by, int bz) const {
    const int quad = (x0 % 4 == 0 && bx >= 4) ? 1 : 0;  // every full-row box of a domain >= 4 cells wide
    // o, obst, strides, plane extents, box, quad, sp, obst_pressure; the output pointers stay null
    return Fields3Args{s.o[s.cur], s.obst, PL, KS, px, p.nx, p.ny, x0, y0, z0, bx, by, bz,
                       quad, quad ? (bx + 3) / 4 * 4 : bx, p.density * (1.f / 3.f)};
}

// u_x, u_y, u_z, |u|, pressure of the box's cells into the packed planar
// host arrays float[b.nz][b.ny][b.nx] (host[i] NULL: field i is neither
// computed nor staged).  Slab by slab: the part of the box inside the slab
// is staged on its device (requested fields x cells; rows padded to 4
// floats on the 16-B path) and copied to its planes of the host arrays.
void lbm3d_handle::store_fields_box(const lbm3d_box &b, float *const (&host)[5]) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive fields from");
    if (b.nx <= 0 || b.ny <= 0 || b.nz <= 0 || b.x0 < 0 || b.y0 < 0 || b.z0 < 0 ||
        (long long)b.x0 + b.nx > p.nx || (long long)b.y0 + b.ny > p.ny || (long long)b.z0 + b.nz > p.nz)
        throw lbm_failure(LBM_E_INVALID, "box must be non-empty and inside the domain");
    int want = 0;
    for (float *f : host) want += f ? 1 : 0;
    if (want == 0) return;
    sync_all();
    for (auto &s : slabs) {
        const int zlo = std::max(b.z0, s.z0), zhi = std::min(b.z0 + b.nz, s.z0 + s.nzs);
        if (zlo >= zhi) continue;
        HIP_CHECK(hipSetDevice(s.dev));
        Fields3Args a = fields_args(s, b.x0, b.y0, zlo - s.z0, b.nx, b.ny, zhi - zlo);
        const size_t rows = (size_t)a.by * a.bz, field_floats = rows * a.sp;
        const DeviceStage stage(sizeof(float) * field_floats * want);
        float **dev[5] = {&a.ux, &a.uy, &a.uz, &a.speed, &a.pressure};
        for (int i = 0, n = 0; i < 5; ++i)
            if (host[i]) *dev[i] = stage.as<float>() + field_floats * n++;
        HIP_CHECK(launch_macroscopic_fields3d(a, false, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        const size_t off = (size_t)(zlo - b.z0) * b.ny * b.nx;
        for (int i = 0; i < 5; ++i) {
            if (!host[i]) continue;
            if (a.sp == b.nx)  // no row padding: one contiguous copy
                HIP_CHECK(hipMemcpy(host[i] + off, *dev[i], sizeof(float) * field_floats, hipMemcpyDeviceToHost));
            else
                HIP_CHECK(hipMemcpy2D(host[i] + off, sizeof(float) * (size_t)b.nx, *dev[i], sizeof(float) * (size_t)a.sp,
                                      sizeof(float) * (size_t)b.nx, rows, hipMemcpyDeviceToHost));
        }
    }
}

// Total mass (fp64 sum of every local cell's fp32 density) and the largest
// |u| over the local fluid cells.  The kernel leaves per-block partials;
// they are folded here in block order, slab after slab, so the same
// lattice always gives the same bits.
void lbm3d_handle::field_stats(double *mass, float *max_speed) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!mass && !max_speed) return;
    sync_all();
    double total = 0.0;
    float umax = 0.f;
    for (auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        Fields3Args a = fields_args(s, 0, 0, 0, p.nx, p.ny, s.nzs);
        const size_t nb = (size_t)fields3d_blocks(a);
        const DeviceStage part((sizeof(double) + sizeof(float)) * nb);  // [nb doubles | nb floats]
        std::vector<double> hm(nb);
        std::vector<float> hu(nb);
        a.mass_part = part.as<double>();
        a.umax_part = reinterpret_cast<float *>(a.mass_part + nb);
        HIP_CHECK(launch_macroscopic_fields3d(a, true, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        HIP_CHECK(hipMemcpy(hm.data(), a.mass_part, sizeof(double) * nb, hipMemcpyDeviceToHost));
        HIP_CHECK(hipMemcpy(hu.data(), a.umax_part, sizeof(float) * nb, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nb; ++i) {
            total += hm[i];
            umax = std::max(umax, hu[i]);
        }
    }
    if (mass) *mass = total;
    if (max_speed) *max_speed = umax;
}
