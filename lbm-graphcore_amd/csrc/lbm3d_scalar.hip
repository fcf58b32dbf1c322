// lbm3d_scalar.hip -- the passive scalar of the D3Q19 engine (the
// lbm3d_scalar_* functions of include/lbm_scalar_hip.h and lbm_thermal_hip.h):
// the D3Q7 step kernel over the lattice of one z slab, the buoyancy kick on
// that lattice, the engine's host side, the extern "C" functions and the
// host-only restatements lbm3d_scalar_step_ref and lbm3d_scalar_buoyancy_ref.
//
// The step kernel.  Memory-bound: per cell it must move 76 B of flow
// populations, the obstacle byte, 28 B of scalar populations read and 28 B
// written, no LDS, no atomics.  The shape of macroscopic_fields3d: a block is
// 64 lanes along x (one wave) by 4 rows, blockIdx.y / .z walk rows and planes,
// offsets in 64 bits.  In a domain at least 4 cells wide (Box3View::quad) a
// lane takes four consecutive cells of a row: nineteen 16-B loads of the flow,
// the obstacle word, one 16-B load each of the rest, +-y and +-z scalar planes,
// and the +-x planes as the lane's own aligned quad plus one value from the
// neighbouring lane by a cross-lane move (the lanes at the ends of a wave or
// of a row load that cell directly); seven 16-B stores.  The last nx % 4
// cells of a row, and domains narrower than 4, go one cell at a time.  Only
// rho and the three velocity components are formed.
//
// One launch per local slab reads the flow through that slab's Box3View and
// the scalar at global z with periodic wrap, all on the compute stream of the
// first slab after a synchronisation of every stream.
//
// Arithmetic: IEEE fp32, as the header writes it, no contraction
// (-ffp-contract=off), correctly rounded divide.

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm3d_cell_macro.hpp"
#include "lbm3d_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_scalar.hpp"
#include "lbm_scalar_hip.h"

namespace lbm {
namespace scalar {

constexpr int S3Q = 19;
constexpr int S3X = 64, S3Y = 4;          // block: 64 lanes along x (one wave) x 4 rows
constexpr int S3_TARGET_BLOCKS = 16384;   // blocks a launch aims for (planes beyond are strided over)

// all cells of one slab (box origin 0, extents nx, ny, nzs), its first plane in the domain, and the two scalar sets
struct Step3 : Box3View {
    const float *gin;
    float *gout;
    long long gplane;
    int gsp, gz0, nz;
    float omega;
};

namespace {

// offset of cell (x, y, z) of the domain inside a scalar plane
__device__ __forceinline__ long long goff(const Step3 &a, int x, int y, int z) {
    return ((long long)z * a.ny + y) * a.gsp + x;
}

// cell (x, y, z) of the slab, every value loaded on its own
__device__ __forceinline__ void step_one(const Step3 &a, int x, int y, int z) {
    float c[S3Q];
    load_cell<S3Q>(a.o + (long long)z * a.PL + (long long)y * a.px, a.KS, x, c);
    const bool blocked = a.obst[((long long)z * a.ny + y) * a.nx + x] != 0;
    float rho;
    const Cell3Macro m = cell3_macro<true, false>(c, blocked, a.obst_pressure, rho);
    const int gz = a.gz0 + z;
    const float p[7] = {a.gin[goff(a, x, y, gz)],
                        a.gin[a.gplane + goff(a, below(x, a.nx), y, gz)],
                        a.gin[2 * a.gplane + goff(a, above(x, a.nx), y, gz)],
                        a.gin[3 * a.gplane + goff(a, x, below(y, a.ny), gz)],
                        a.gin[4 * a.gplane + goff(a, x, above(y, a.ny), gz)],
                        a.gin[5 * a.gplane + goff(a, x, y, below(gz, a.nz))],
                        a.gin[6 * a.gplane + goff(a, x, y, above(gz, a.nz))]};
    float out[7];
    cell3(p, blocked, m.ux, m.uy, m.uz, a.omega, out);
    const long long d = goff(a, x, y, gz);
#pragma unroll
    for (int k = 0; k < 7; ++k) a.gout[k * a.gplane + d] = out[k];
}

}  // namespace

__global__ __launch_bounds__(S3X *S3Y) void scalar_step3d(Step3 a) {
    const bool quad = a.quad != 0;
    const int cpl = quad ? 4 : 1;  // cells per lane
    const int tx = threadIdx.x & (S3X - 1), ty = threadIdx.x / S3X;
    const int x = (blockIdx.x * S3X + tx) * cpl;
    const bool active = x < a.bx;
    const bool full = quad && x + 4 <= a.bx;
    const bool obst_word = (a.nx & 3) == 0;
    // a row of the block is a wave and the loops below depend on ty alone: the cross-lane moves run converged
    for (int z = blockIdx.z; z < a.bz; z += gridDim.z) {
        for (int y = blockIdx.y * S3Y + ty; y < a.by; y += gridDim.y * S3Y) {
            const int gz = a.gz0 + z;
            const long long here = goff(a, full ? x : 0, y, gz);
            float4 g1 = make_float4(0.f, 0.f, 0.f, 0.f), g2 = g1;
            if (full) {
                g1 = *reinterpret_cast<const float4 *>(a.gin + a.gplane + here);
                g2 = *reinterpret_cast<const float4 *>(a.gin + 2 * a.gplane + here);
            }
            const float west = __shfl_up(g1.w, 1, 64);
            const float east = __shfl_down(g2.x, 1, 64);
            if (full) {
                const long long row = goff(a, 0, y, gz);
                const float pw = tx != 0 ? west : a.gin[a.gplane + row + below(x, a.nx)];
                const float pe =
                    (tx != S3X - 1 && x + 8 <= a.bx) ? east : a.gin[2 * a.gplane + row + (x + 4 == a.nx ? 0 : x + 4)];
                // First the flow: its 76 registers are dead once the four velocities stand, before the
                // scalar planes are loaded (issued together the kernel took all 256 VGPRs: one wave per SIMD).
                float u[4][3];
                unsigned bits;
                {
                    float4 v[S3Q];
                    load_quad<S3Q>(a.o + (long long)z * a.PL + (long long)y * a.px + x, a.KS, v);
                    bits = quad_map_bytes(a.obst + ((long long)z * a.ny + y) * a.nx + x, obst_word);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float c[S3Q];
                        quad_cell<S3Q>(v, i, c);
                        float rho;
                        // as a fluid cell, whatever the map says: an obstacle cell's velocity is never used, and
                        // a branch on the map here lets the compiler sink the flow loads into it, 4 B at a time
                        const Cell3Macro m = cell3_macro<true, false>(c, false, a.obst_pressure, rho);
                        u[i][0] = m.ux;
                        u[i][1] = m.uy;
                        u[i][2] = m.uz;
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
                const float4 g0 = *reinterpret_cast<const float4 *>(a.gin + here);
                const float4 g3 = *reinterpret_cast<const float4 *>(a.gin + 3 * a.gplane + goff(a, x, below(y, a.ny), gz));
                const float4 g4 = *reinterpret_cast<const float4 *>(a.gin + 4 * a.gplane + goff(a, x, above(y, a.ny), gz));
                const float4 g5 = *reinterpret_cast<const float4 *>(a.gin + 5 * a.gplane + goff(a, x, y, below(gz, a.nz)));
                const float4 g6 = *reinterpret_cast<const float4 *>(a.gin + 6 * a.gplane + goff(a, x, y, above(gz, a.nz)));
                const float4 p1 = make_float4(pw, g1.x, g1.y, g1.z);
                const float4 p2 = make_float4(g2.y, g2.z, g2.w, pe);
                float o[7][4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p[7] = {pick(g0, i), pick(p1, i), pick(p2, i), pick(g3, i),
                                        pick(g4, i), pick(g5, i), pick(g6, i)};
                    float out[7];
                    cell3(p, ((bits >> (8 * i)) & 0xffu) != 0, u[i][0], u[i][1], u[i][2], a.omega, out);
#pragma unroll
                    for (int k = 0; k < 7; ++k) o[k][i] = out[k];
                }
                float *dst = a.gout + here;
#pragma unroll
                for (int k = 0; k < 7; ++k)
                    *reinterpret_cast<float4 *>(dst + k * a.gplane) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
            } else if (active) {
                // one cell per lane, or the ragged tail of a row: its last nx % 4 cells, one at a time
#pragma unroll 1
                for (int i = 0; i < cpl && x + i < a.bx; ++i) step_one(a, x + i, y, z);
            }
        }
    }
}

// ---- the buoyancy kick (include/lbm_thermal_hip.h) ----
//
// A streaming read-modify-write of the current flow lattice: per cell 28 B of
// scalar populations and the obstacle byte read, the eighteen moving flow
// planes read and written (173 B; f0 is not touched).  The block and grid of
// the step kernel.  On the quad path a lane first forms the nine increments of
// each of its four cells from the seven scalar planes, then walks the nine
// opposite pairs of flow planes three at a time: six 16-B loads, then six
// 16-B stores (the 25 quads are never live together).  A lane needs only its own cells and
// owns what it writes: no LDS, no atomics, no cross-lane move, no race in
// place.  Ghost planes and pad columns are not touched.

// all cells of one slab, writable, its first plane in the domain, and the current scalar set
constexpr int KICK3_BATCH = 3;  // pairs loaded together; divides KICK3_PAIRS
static_assert(KICK3_PAIRS % KICK3_BATCH == 0, "whole batches");

struct Kick3 : Box3Edit {
    const float *g;
    long long gplane;
    int gsp, gz0;
    float kx, ky, kz, phi_ref;
};

namespace {

__device__ __forceinline__ void kick_one(const Kick3 &a, int x, int y, int z) {
    const long long at = ((long long)(a.gz0 + z) * a.ny + y) * a.gsp + x;
    float g[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) g[k] = a.g[k * a.gplane + at];
    const bool blocked = a.obst[((long long)z * a.ny + y) * a.nx + x] != 0;
    float inc[KICK3_PAIRS];
    kick3_inc(cell_phi<7>(g), a.phi_ref, a.kx, a.ky, a.kz, inc);
    float *f = a.e + (long long)z * a.PL + (long long)y * a.px + x;
#pragma unroll
    for (int j = 0; j < KICK3_PAIRS; ++j) {
        float *fp = f + kick3_plus(j) * a.KS, *fm = f + kick3_minus(j) * a.KS;
        float plus = *fp, minus = *fm;
        kick_pair(plus, minus, blocked, inc[j]);
        *fp = plus;
        *fm = minus;
    }
}

__device__ __forceinline__ float4 quad_of(const float (&c)[4]) { return make_float4(c[0], c[1], c[2], c[3]); }

}  // namespace

__global__ __launch_bounds__(S3X *S3Y) void scalar_buoyancy3d(Kick3 a) {
    const bool quad = a.quad != 0;
    const int cpl = quad ? 4 : 1;  // cells per lane
    const int tx = threadIdx.x & (S3X - 1), ty = threadIdx.x / S3X;
    const int x = (blockIdx.x * S3X + tx) * cpl;
    if (x >= a.bx) return;
    const bool full = quad && x + 4 <= a.bx;
    const bool obst_word = (a.nx & 3) == 0;
    for (int z = blockIdx.z; z < a.bz; z += gridDim.z) {
        for (int y = blockIdx.y * S3Y + ty; y < a.by; y += gridDim.y * S3Y) {
            if (full) {
                float inc[4][KICK3_PAIRS];
                unsigned bits;
                {
                    float4 gq[7];
                    load_quad<7, true>(a.g + ((long long)(a.gz0 + z) * a.ny + y) * a.gsp + x, a.gplane, gq);
                    bits = quad_map_bytes(a.obst + ((long long)z * a.ny + y) * a.nx + x, obst_word);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float g[7] = {pick(gq[0], i), pick(gq[1], i), pick(gq[2], i), pick(gq[3], i),
                                            pick(gq[4], i), pick(gq[5], i), pick(gq[6], i)};
                        kick3_inc(cell_phi<7>(g), a.phi_ref, a.kx, a.ky, a.kz, inc[i]);
                    }
                }
                float *f = a.e + (long long)z * a.PL + (long long)y * a.px + x;
                // three pairs at a time: six 16-B loads in flight, then their six stores (a store ends the run
                // of loads the compiler may issue ahead of it: the planes may alias for all it knows)
#pragma unroll
                for (int j0 = 0; j0 < KICK3_PAIRS; j0 += KICK3_BATCH) {
                    float4 vp[KICK3_BATCH], vm[KICK3_BATCH];
#pragma unroll
                    for (int j = 0; j < KICK3_BATCH; ++j) {
                        vp[j] = *reinterpret_cast<const float4 *>(f + kick3_plus(j0 + j) * a.KS);
                        vm[j] = *reinterpret_cast<const float4 *>(f + kick3_minus(j0 + j) * a.KS);
                    }
#pragma unroll
                    for (int j = 0; j < KICK3_BATCH; ++j) {
                        float plus[4] = {vp[j].x, vp[j].y, vp[j].z, vp[j].w};
                        float minus[4] = {vm[j].x, vm[j].y, vm[j].z, vm[j].w};
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            kick_pair(plus[i], minus[i], ((bits >> (8 * i)) & 0xffu) != 0, inc[i][j0 + j]);
                        *reinterpret_cast<float4 *>(f + kick3_plus(j0 + j) * a.KS) = quad_of(plus);
                        *reinterpret_cast<float4 *>(f + kick3_minus(j0 + j) * a.KS) = quad_of(minus);
                    }
                }
            } else {
                // one cell per lane, or the ragged tail of a row: its last nx % 4 cells, one at a time
#pragma unroll 1
                for (int i = 0; i < cpl && x + i < a.bx; ++i) kick_one(a, x + i, y, z);
            }
        }
    }
}

// the grid of both kernels over a whole-slab view (and of the forcing zones over a box: lbm_scalar.hpp)
dim3 slab_grid(const Box3View &a) {
    const int cpl = a.quad ? 4 : 1;
    const long long lanes = ((long long)a.bx + cpl - 1) / cpl;
    const long long gx = (lanes + S3X - 1) / S3X;
    const long long gy = std::min<long long>(((long long)a.by + S3Y - 1) / S3Y, 65535);
    const long long gz =
        std::max<long long>(1, std::min<long long>(std::min(a.bz, 65535), S3_TARGET_BLOCKS / (gx * gy)));
    return dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
}

int slab_lanes_x() { return S3X; }
int slab_rows() { return S3Y; }

}  // namespace scalar
}  // namespace lbm

using namespace lbm;

namespace {

scalar::State &scalar_state(lbm3d_handle &h) {
    if (!h.scalars) throw lbm_failure(LBM_E_STATE, "no scalar: call lbm3d_scalar_begin first");
    return *h.scalars;
}

const auto run_directly = [](auto &&launch) { launch(); };  // no profile classes on this engine

}  // namespace

// ---- D3Q19 engine: host side ----

// What a feature that keeps one global array beside the lattice asks of the handle (the scalar; the forcing zones
// of lbm3d_forcing.hip): one device, the whole domain here, at most 16 local slabs, no RCCL world > 1.
void lbm3d_handle::need_whole_domain(const char *what) const {
    const std::string w(what);
    if (transport == LBM_TRANSPORT_RCCL && world > 1)
        throw lbm_failure(LBM_E_INVALID, w + " on RCCL handles of more than one rank are not built");
    if ((int)slabs.size() > scalar::MAX_PARTS)
        throw lbm_failure(LBM_E_INVALID, w + " on more than 16 local slabs are not built");
    int planes = 0;
    for (const auto &s : slabs) {
        if (s.dev != slabs[0].dev)
            throw lbm_failure(LBM_E_INVALID, w + " on slabs of more than one device are not built");
        planes += s.nzs;
    }
    if (slabs.empty() || planes != p.nz)
        throw lbm_failure(LBM_E_INVALID, w + " need every slab of the domain on this handle");
}

void lbm3d_handle::scalar_begin(float omega_s, const float *phi0) {
    need_whole_domain("scalars");
    scalar::check_omega(omega_s);
    sync_all();
    scalar::begin(scalars, slabs[0].dev, 7, p.nx, p.ny, p.nz, omega_s, phi0);
}

void lbm3d_handle::scalar_set_fixed(int64_t n, const int32_t *x, const int32_t *y, const int32_t *z,
                                    const float *value) {
    scalar::State &t = scalar_state(*this);
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    scalar::set_fixed<7>(t, n, x, y, z, true, value, slabs[0].s_comp, run_directly);
}

void lbm3d_handle::scalar_advance(int steps) {
    scalar::State &t = scalar_state(*this);
    if (steps < 0) throw lbm_failure(LBM_E_INVALID, "steps must not be negative");
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to advance the scalar over");
    if (steps == 0) return;
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    const hipStream_t st = slabs[0].s_comp;
    for (int n = 0; n < steps; ++n) {
        for (const auto &s : slabs) {
            scalar::Step3 a{box_view(s, 0, 0, 0, p.nx, p.ny, s.nzs)};
            a.gin = t.g[t.cur];
            a.gout = t.g[t.cur ^ 1];
            a.gplane = t.grid.plane;
            a.gsp = t.grid.sp;
            a.gz0 = s.z0;
            a.nz = p.nz;
            a.omega = t.omega;
            hipLaunchKernelGGL(scalar::scalar_step3d, scalar::slab_grid(a), dim3(scalar::S3X * scalar::S3Y), 0, st, a);
            HIP_CHECK(hipGetLastError());
        }
        t.cur ^= 1;
        ++t.steps;
        // the wall models (include/lbm_scalar_walls_hip.h), before the fixed list
        if (scalar::walls_listed(t)) HIP_CHECK(scalar::walls_pass3d(t, t.g[t.cur], st));
        scalar::apply_fixed<7>(t, t.g[t.cur], st, run_directly);
    }
    HIP_CHECK(hipStreamSynchronize(st));
}

int64_t lbm3d_handle::scalar_steps() { return scalar_state(*this).steps; }

void lbm3d_handle::scalar_store(float *phi, float *g) {
    scalar::State &t = scalar_state(*this);
    if (!phi && !g) return;
    sync_all();
    scalar::store<7>(t, phi, g, slabs[0].s_comp);
}

void lbm3d_handle::scalar_stats(double *total, float *min, float *max) {
    scalar::State &t = scalar_state(*this);
    if (!total && !min && !max) return;
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    double sum[1] = {0.0};
    float m[2] = {-INFINITY, -INFINITY};
    for (const auto &s : slabs)
        scalar::stats_region<7>(t, scalar::Region{s.obst, 0, 0, s.z0, p.nx, p.ny, s.nzs}, slabs[0].s_comp, sum, m,
                                run_directly);
    scalar::stats_out(sum, m, total, min, max);
}

void lbm3d_handle::scalar_end() { scalar::end(scalars); }

// The kick on the current lattice of every slab, then the ghost planes as after load_cells (refresh).
void lbm3d_handle::scalar_buoyancy(float sx, float sy, float sz, float phi_ref) {
    scalar::State &t = scalar_state(*this);
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice for the scalar to act on");
    if (!(std::isfinite(sx) && std::isfinite(sy) && std::isfinite(sz) && std::isfinite(phi_ref)))
        throw lbm_failure(LBM_E_INVALID, "the impulse and phi_ref must be finite");
    if (sx == 0.f && sy == 0.f && sz == 0.f) return;
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    const hipStream_t st = slabs[0].s_comp;
    for (const auto &s : slabs) {
        scalar::Kick3 a{slab_edit(s)};
        a.g = t.g[t.cur];
        a.gplane = t.grid.plane;
        a.gsp = t.grid.sp;
        a.gz0 = s.z0;
        a.kx = p.density * sx;
        a.ky = p.density * sy;
        a.kz = p.density * sz;
        a.phi_ref = phi_ref;
        hipLaunchKernelGGL(scalar::scalar_buoyancy3d, scalar::slab_grid(a), dim3(scalar::S3X * scalar::S3Y), 0, st, a);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(st));
    refresh();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm3d_scalar_begin(lbm3d_handle *h, float omega_s, const float *phi0) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_begin(omega_s, phi0); });
}

int lbm3d_scalar_set_fixed(lbm3d_handle *h, int64_t n, const int32_t *x, const int32_t *y, const int32_t *z,
                           const float *value) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_set_fixed(n, x, y, z, value); });
}

int lbm3d_scalar_advance(lbm3d_handle *h, int32_t steps) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_advance(steps); });
}

int lbm3d_scalar_steps(lbm3d_handle *h, int64_t *n) {
    if (!h || !n) return LBM_E_INVALID;
    return guarded(h, [&] { *n = h->scalar_steps(); });
}

int lbm3d_scalar_store(lbm3d_handle *h, float *phi, float *g) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_store(phi, g); });
}

int lbm3d_scalar_stats(lbm3d_handle *h, double *total, float *min, float *max) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_stats(total, min, max); });
}

int lbm3d_scalar_end(lbm3d_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_end(); });
}

int lbm3d_scalar_step_ref(int32_t nx, int32_t ny, int32_t nz, float omega_s, const float *ux, const float *uy,
                          const float *uz, const uint8_t *obst, const float *g_in, float *g_out) {
    if (!scalar::ref_args_ok(nx, ny, nz, omega_s, {ux, uy, uz, obst, g_in, g_out})) return LBM_E_INVALID;
    const size_t plane = (size_t)nx * ny * nz;
    const auto at = [&](int x, int y, int z) { return ((size_t)z * ny + y) * nx + x; };
    for (int z = 0; z < nz; ++z)
        for (int y = 0; y < ny; ++y)
            for (int x = 0; x < nx; ++x) {
                const size_t i = at(x, y, z);
                const float p[7] = {g_in[i],
                                    g_in[plane + at(scalar::below(x, nx), y, z)],
                                    g_in[2 * plane + at(scalar::above(x, nx), y, z)],
                                    g_in[3 * plane + at(x, scalar::below(y, ny), z)],
                                    g_in[4 * plane + at(x, scalar::above(y, ny), z)],
                                    g_in[5 * plane + at(x, y, scalar::below(z, nz))],
                                    g_in[6 * plane + at(x, y, scalar::above(z, nz))]};
                float out[7];
                scalar::cell3(p, obst[i] != 0, ux[i], uy[i], uz[i], omega_s, out);
                for (int k = 0; k < 7; ++k) g_out[k * plane + i] = out[k];
            }
    return LBM_OK;
}

int lbm3d_scalar_buoyancy(lbm3d_handle *h, float sx, float sy, float sz, float phi_ref) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_buoyancy(sx, sy, sz, phi_ref); });
}

int lbm3d_scalar_buoyancy_ref(int32_t nx, int32_t ny, int32_t nz, float density, float sx, float sy, float sz,
                              float phi_ref, const uint8_t *obst, const float *g, float *cells) {
    if (!scalar::kick_args_ok(nx, ny, nz, {density, sx, sy, sz, phi_ref}, {obst, g, cells})) return LBM_E_INVALID;
    if (sx == 0.f && sy == 0.f && sz == 0.f) return LBM_OK;
    const float kx = density * sx, ky = density * sy, kz = density * sz;
    const size_t plane = (size_t)nx * ny * nz;
    for (size_t i = 0; i < plane; ++i) {
        float gc[7];
        for (int k = 0; k < 7; ++k) gc[k] = g[k * plane + i];
        float inc[scalar::KICK3_PAIRS];
        scalar::kick3_inc(scalar::cell_phi<7>(gc), phi_ref, kx, ky, kz, inc);
        float *c = cells + i * scalar::S3Q;
        for (int j = 0; j < scalar::KICK3_PAIRS; ++j)
            scalar::kick_pair(c[scalar::kick3_plus(j)], c[scalar::kick3_minus(j)], obst[i] != 0, inc[j]);
    }
    return LBM_OK;
}

}  // extern "C"
