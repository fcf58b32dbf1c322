// lbm3d_gradients.hip -- vorticity, divergence, strain rate and the Q criterion
// of the D3Q19 engine on the device (the lbm3d_* functions of
// include/lbm_gradients_hip.h).  The kernel, then the engine's host side.
//
// Neighbours in x and y wrap by index inside the slab; across the slab's two
// z faces they come from velocity planes, never from the lattice's ghost
// planes: macroscopic_fields3d writes (ux, uy, uz) of every slab's first and
// last plane, and each slab receives its neighbours' facing planes by a
// device copy (the periodic self-image is the same path).
//
// velocity_gradients3d: a block owns a tile of 64 x 16 cells of a plane and
// walks a segment of 32 planes in z.  A thread takes four consecutive cells
// (nineteen 16-B loads per plane, lbm_quad.hpp) and keeps the
// velocities of three planes in registers (36 VGPRs), so each population of
// the tile is read once per plane; the in-plane neighbours go through LDS:
// the centre plane's velocities as aligned float4 rows, plus the 160 cells
// around the tile (no corners), which 160 threads compute from single-cell
// loads.  Reads per owned cell: 1 + 160 / 1024 in the plane, times 34 / 32
// along z.  Boxes whose x origin is no multiple of 4 take one-cell loads.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "lbm3d_cell_macro.hpp"
#include "lbm3d_engine.hpp"
#include "lbm_gradients.hpp"
#include "lbm_gradients_hip.h"
#include "lbm_quad.hpp"

namespace lbm {
namespace grad {

namespace {

constexpr int G3Q = 19;
constexpr int G3T = G3X * G3Y;  // threads of a block

// velocity of the cell (xg, yg) of slab plane lz (0 <= lz < nzs)
__device__ __forceinline__ void cell3_velocity(const Grad3Args &a, int xg, int yg, int lz, float (&u)[3],
                                               bool &blocked) {
    const float *src = a.o + (long long)lz * a.PL + (long long)yg * a.px + xg;
    float s[G3Q];
    load_cell<G3Q>(src, a.KS, 0, s);
    blocked = a.obst[((long long)lz * a.ny + yg) * a.nx + xg] != 0;
    float rho;
    const Cell3Macro m = cell3_macro<true, false>(s, blocked, a.obst_pressure, rho);
    u[0] = m.ux;
    u[1] = m.uy;
    u[2] = m.uz;
}

// The velocities of the thread's four cells (box-local x .. x + 3, row y) of
// slab plane lz (-1 <= lz <= nzs): every cell the tile's stencils can touch
// (x + i <= bx, y <= by, wrapped into the plane), +0 elsewhere.
__device__ __forceinline__ void quad_velocities(const Grad3Args &a, int x, int y, int lz, float (&u)[3][4],
                                                unsigned &blocked) {
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) u[c][i] = 0.f;
    blocked = 0;
    if (x > a.bx || y > a.by) return;
    int yg = a.y0 + y;
    if (yg == a.ny) yg = 0;
    if (lz < 0 || lz >= a.nzs) {
        const float *e = lz < 0 ? a.below : a.above;
        const long long comp = (long long)a.ny * a.hp;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (x + i > a.bx) continue;
            int xg = a.x0 + x + i;
            if (xg == a.nx) xg = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) u[c][i] = e[c * comp + (long long)yg * a.hp + xg];
        }
        return;
    }
    if (a.quad && x + 4 <= a.bx) {
        const int xg = a.x0 + x;
        const float *src = a.o + (long long)lz * a.PL + (long long)yg * a.px + xg;
        const uint8_t *ob = a.obst + ((long long)lz * a.ny + yg) * a.nx + xg;
        float4 v[G3Q];
        load_quad<G3Q>(src, a.KS, v);
        const unsigned bits = quad_map_bytes(ob, (a.nx & 3) == 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float s[G3Q];
            quad_cell<G3Q>(v, i, s);
            const bool b = ((bits >> (8 * i)) & 0xffu) != 0;
            if (b) blocked |= 1u << i;
            float rho;
            const Cell3Macro m = cell3_macro<true, false>(s, b, a.obst_pressure, rho);
            u[0][i] = m.ux;
            u[1][i] = m.uy;
            u[2][i] = m.uz;
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (x + i > a.bx) continue;
        int xg = a.x0 + x + i;
        if (xg == a.nx) xg = 0;
        float w[3];
        bool b;
        cell3_velocity(a, xg, yg, lz, w, b);
        if (b) blocked |= 1u << i;
        u[0][i] = w[0];
        u[1][i] = w[1];
        u[2][i] = w[2];
    }
}

}  // namespace

// STATS: no field is stored; block b (x fastest, then y, then z) writes its
// partial sums and maxima over the fluid cells it owns (fold_block, lbm_quad.hpp).
template <bool STATS>
__global__ __launch_bounds__(G3T) void velocity_gradients3d(Grad3Args a) {
    // centre plane: rows -1 .. G3Y of the tile (index + 1), then the columns -1 and G3W beside it
    __shared__ __attribute__((aligned(16))) float tile[3][G3Y + 2][G3W];
    __shared__ float side[3][G3Y][2];
    const int tid = threadIdx.x;
    const int lx = tid & (G3X - 1), ry = tid / G3X;
    const int X = blockIdx.x * G3W, Y = blockIdx.y * G3Y;
    const int x = X + 4 * lx, y = Y + ry;  // box-local
    const int zs = blockIdx.z * G3_SEG, ze = min(zs + G3_SEG, a.bz);
    // the cell around the tile this thread also computes (tid < 2 G3W + 2 G3Y): box-local (hx, hy)
    int hx = 0, hy = 0;
    bool halo = false;
    if (tid < 2 * G3W) {
        hx = X + (tid & (G3W - 1));
        hy = tid < G3W ? Y - 1 : Y + G3Y;
        halo = true;
    } else if (tid < 2 * G3W + 2 * G3Y) {
        hy = Y + ((tid - 2 * G3W) & (G3Y - 1));
        hx = tid < 2 * G3W + G3Y ? X - 1 : X + G3W;
        halo = true;
    }
    halo = halo && hx <= a.bx && hy <= a.by;
    int hxg = a.x0 + hx, hyg = a.y0 + hy;
    hxg = hxg < 0 ? a.nx - 1 : hxg == a.nx ? 0 : hxg;
    hyg = hyg < 0 ? a.ny - 1 : hyg == a.ny ? 0 : hyg;

    double sw2 = 0.0, ss2 = 0.0;
    float mw = 0.f, md = 0.f;
    float p[3][4], c[3][4], n[3][4];
    unsigned pb, cb, nb;
    quad_velocities(a, x, y, a.z0 + zs - 1, p, pb);
    quad_velocities(a, x, y, a.z0 + zs, c, cb);
    for (int z = zs; z < ze; ++z) {
        const int lz = a.z0 + z;
        quad_velocities(a, x, y, lz + 1, n, nb);
        float hu[3] = {0.f, 0.f, 0.f};
        if (halo) {
            bool b;
            cell3_velocity(a, hxg, hyg, lz, hu, b);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            *reinterpret_cast<float4 *>(&tile[k][ry + 1][4 * lx]) = make_float4(c[k][0], c[k][1], c[k][2], c[k][3]);
            if (tid < 2 * G3W)
                tile[k][tid < G3W ? 0 : G3Y + 1][tid & (G3W - 1)] = hu[k];
            else if (tid < 2 * G3W + 2 * G3Y)
                side[k][(tid - 2 * G3W) & (G3Y - 1)][tid < 2 * G3W + G3Y ? 0 : 1] = hu[k];
        }
        __syncthreads();
        if (x < a.bx && y < a.by) {
            float4 north[3], south[3];
            float west[3], east[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                north[k] = *reinterpret_cast<const float4 *>(&tile[k][ry + 2][4 * lx]);
                south[k] = *reinterpret_cast<const float4 *>(&tile[k][ry][4 * lx]);
                west[k] = lx > 0 ? tile[k][ry + 1][4 * lx - 1] : side[k][ry][0];
                east[k] = lx < G3X - 1 ? tile[k][ry + 1][4 * lx + 4] : side[k][ry][1];
            }
            Grad3 g[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float ex[3], wx[3], ny_[3], sy[3], uz[3], dz[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    ex[k] = i < 3 ? c[k][i + 1] : east[k];
                    wx[k] = i > 0 ? c[k][i - 1] : west[k];
                    ny_[k] = i == 0 ? north[k].x : i == 1 ? north[k].y : i == 2 ? north[k].z : north[k].w;
                    sy[k] = i == 0 ? south[k].x : i == 1 ? south[k].y : i == 2 ? south[k].z : south[k].w;
                    uz[k] = n[k][i];
                    dz[k] = p[k][i];
                }
                g[i] = gradients3(ex, wx, ny_, sy, uz, dz);
                const bool fluid = x + i < a.bx && !((cb >> i) & 1u);
                if (!fluid) g[i] = Grad3{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
                if (STATS && fluid) {
                    sw2 += ((double)g[i].wx * (double)g[i].wx + (double)g[i].wy * (double)g[i].wy) +
                           (double)g[i].wz * (double)g[i].wz;
                    ss2 += (double)g[i].s2;
                    mw = fmaxf(mw, fabsf(g[i].vorticity));
                    md = fmaxf(md, fabsf(g[i].divergence));
                }
            }
            if (!STATS) {
                const long long so = ((long long)z * a.by + y) * a.sp + x;
#pragma unroll
                for (int f = 0; f < 7; ++f) {
                    if (!a.out[f]) continue;
                    float v[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        v[i] = f == 0 ? g[i].wx : f == 1 ? g[i].wy : f == 2 ? g[i].wz : f == 3 ? g[i].vorticity
                             : f == 4 ? g[i].divergence : f == 5 ? g[i].strain : g[i].q;
                    if (x + 4 <= a.bx) {
                        *reinterpret_cast<float4 *>(a.out[f] + so) = make_float4(v[0], v[1], v[2], v[3]);
                    } else {
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (x + i < a.bx) a.out[f][so + i] = v[i];
                    }
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                p[k][i] = c[k][i];
                c[k][i] = n[k][i];
            }
        cb = nb;
    }
    (void)pb;
    if (STATS) {
        double s[2] = {sw2, ss2};
        float m[2] = {mw, md};
        const long long b = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        fold_block<G3T / 64>(s, m, b, (long long)gridDim.x * gridDim.y * gridDim.z, a.sum_part, a.max_part);
    }
}

namespace {
dim3 gradients3d_grid(const Grad3Args &a) {
    return dim3((unsigned)((a.bx + G3W - 1) / G3W), (unsigned)((a.by + G3Y - 1) / G3Y),
                (unsigned)((a.bz + G3_SEG - 1) / G3_SEG));
}
}  // namespace

// blocks of a launch over a.bx x a.by x a.bz: also the partials a stats launch writes
long long gradients3d_blocks(const Grad3Args &a) {
    const dim3 g = gradients3d_grid(a);
    return (long long)g.x * g.y * g.z;
}

hipError_t launch_velocity_gradients3d(const Grad3Args &a, bool stats, hipStream_t s) {
    const dim3 g = gradients3d_grid(a);
    if (g.y > 65535u || g.z > 65535u) return hipErrorInvalidValue;
    if (stats)
        hipLaunchKernelGGL(velocity_gradients3d<true>, g, dim3(G3T), 0, s, a);
    else
        hipLaunchKernelGGL(velocity_gradients3d<false>, g, dim3(G3T), 0, s, a);
    return hipGetLastError();
}

}  // namespace grad
}  // namespace lbm

// ---- D3Q19 engine: host side ----

using namespace lbm;
using lbm::grad::Grad3Args;

// Allocates the face buffers at the first call -- per slab [own top | own
// bottom | above | below], one velocity plane [3][ny][hp] each -- then fills
// every slab's `above` / `below` from its z neighbours' facing planes.  Ends
// synchronised; returns the row pitch hp.
int lbm3d_handle::grad_prepare() {
    if (transport == LBM_TRANSPORT_RCCL && world > 1)
        throw lbm_failure(LBM_E_INVALID,
                          "velocity gradients are not built for RCCL handles of world size > 1: the neighbours' "
                          "face velocities live in other processes");
    const int hp = box_view(slabs[0], 0, 0, 0, p.nx, p.ny, 1).sp;
    const size_t plane = (size_t)3 * p.ny * hp;
    if (grad_faces.empty()) {
        grad_faces.assign(slabs.size(), nullptr);
        for (size_t k = 0; k < slabs.size(); ++k) {
            HIP_CHECK(hipSetDevice(slabs[k].dev));
            HIP_CHECK(hipMalloc(&grad_faces[k], sizeof(float) * 4 * plane));
        }
    }
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        for (int top = 0; top < 2; ++top) {
            Fields3Args a{box_view(s, 0, 0, top == 0 ? s.nzs - 1 : 0, p.nx, p.ny, 1)};
            float *buf = grad_faces[k] + (size_t)top * plane;
            a.ux = buf;
            a.uy = buf + (size_t)p.ny * hp;
            a.uz = buf + 2 * (size_t)p.ny * hp;
            HIP_CHECK(launch_macroscopic_fields3d(a, false, s.s_comp));
        }
    }
    for (const auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        const Slab *up = local((s.id + 1) % parts), *down = local((s.id + parts - 1) % parts);
        if (!up || !down) throw lbm_failure(LBM_E_INTERNAL, "missing local neighbour slab");
        // above <- the upper neighbour's bottom plane; below <- the lower neighbour's top plane
        const Slab *src[2] = {up, down};
        for (int j = 0; j < 2; ++j) {
            const float *from = grad_faces[(size_t)(src[j] - slabs.data())] + (size_t)(j == 0 ? 1 : 0) * plane;
            float *to = grad_faces[k] + (size_t)(2 + j) * plane;
            if (src[j]->dev == s.dev)
                HIP_CHECK(hipMemcpyAsync(to, from, sizeof(float) * plane, hipMemcpyDeviceToDevice, s.s_comp));
            else
                HIP_CHECK(hipMemcpyPeerAsync(to, s.dev, from, src[j]->dev, sizeof(float) * plane, s.s_comp));
        }
    }
    for (const auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    return hp;
}

void lbm3d_handle::grad_release() {
    for (size_t k = 0; k < grad_faces.size() && k < slabs.size(); ++k)
        if (grad_faces[k] && hipSetDevice(slabs[k].dev) == hipSuccess) (void)hipFree(grad_faces[k]);
    grad_faces.clear();
}

// the cells [x0, x0+bx) x [y0, y0+by) x [z0, z0+bz) of slab k (z0 slab-local); the output pointers stay null
Grad3Args lbm3d_handle::grad_args(size_t k, int hp, int x0, int y0, int z0, int bx, int by, int bz) const {
    const Slab &s = slabs[k];
    const size_t plane = (size_t)3 * p.ny * hp;
    Grad3Args a{box_view(s, x0, y0, z0, bx, by, bz)};
    a.nzs = s.nzs;
    // a thread owns four cells of a row whatever the box: aligned boxes narrower than 4 too, rows always padded
    a.quad = x0 % 4 == 0 ? 1 : 0;
    a.sp = (bx + 3) / 4 * 4;
    a.above = grad_faces[k] + 2 * plane;
    a.below = grad_faces[k] + 3 * plane;
    a.hp = hp;
    return a;
}

// The LBM3D_GRAD_* fields of the box's cells into the packed planar host
// arrays float[b.nz][b.ny][b.nx] (a NULL entry is neither computed nor
// staged), slab by slab as store_fields_box.
void lbm3d_handle::store_gradients_box(const lbm3d_box &b, float *const *host) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive gradients from");
    check_box(b);
    const int want = count_wanted(host, LBM3D_GRAD_FIELDS);
    if (want == 0) return;
    sync_all();
    const int hp = grad_prepare();
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        int zlo, zhi;
        if (!slab_planes(s, b, zlo, zhi)) continue;
        HIP_CHECK(hipSetDevice(s.dev));
        Grad3Args a = grad_args(k, hp, b.x0, b.y0, zlo - s.z0, b.nx, b.ny, zhi - zlo);
        const size_t rows = (size_t)a.by * a.bz;
        const PlanarStage stage(want, rows * a.sp);
        for (int i = 0, n = 0; i < LBM3D_GRAD_FIELDS; ++i)
            if (host[i]) a.out[i] = stage.field(n++);
        HIP_CHECK(grad::launch_velocity_gradients3d(a, false, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(host, LBM3D_GRAD_FIELDS, box_span(b, zlo), (size_t)a.sp, (size_t)b.nx, rows);
    }
}

// Sums of |vorticity|^2 and S:S (fp64) and the largest |vorticity| and
// |divergence| over the local fluid cells, from the kernel's per-block
// partials (BlockPartials, lbm_diag_host.hpp), slab after slab.
void lbm3d_handle::gradient_stats(double *sum_w2, double *sum_s2, float *max_w, float *max_div) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!sum_w2 && !sum_s2 && !max_w && !max_div) return;
    sync_all();
    const int hp = grad_prepare();
    double sum[2] = {0.0, 0.0};  // w2, s2
    float max[2] = {0.f, 0.f};   // |vorticity|, |divergence|
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        Grad3Args a = grad_args(k, hp, 0, 0, 0, p.nx, p.ny, s.nzs);
        const BlockPartials<2, 2> part((size_t)grad::gradients3d_blocks(a));
        a.sum_part = part.sums();
        a.max_part = part.maxima();
        HIP_CHECK(grad::launch_velocity_gradients3d(a, true, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        part.fold(sum, max);
    }
    if (sum_w2) *sum_w2 = sum[0];
    if (sum_s2) *sum_s2 = sum[1];
    if (max_w) *max_w = max[0];
    if (max_div) *max_div = max[1];
}
