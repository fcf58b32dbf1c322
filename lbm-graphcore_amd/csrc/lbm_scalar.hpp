// lbm_scalar.hpp -- the passive scalar of both engines (lbm_scalar.hip,
// lbm3d_scalar.hip; include/lbm_scalar_hip.h) and its buoyancy kick on the
// flow (include/lbm_thermal_hip.h): the per-cell arithmetic,
// compiled for the device and for the host from one text, the scalar lattice a
// handle keeps, the small kernels both engines share (fixed cells, phi,
// statistics) and their host side.  The step kernels, which read the flow
// lattice through each engine's own view, are in the two .hip files.
//
// The scalar lattice is global: Q planes (5 or 7) of nz x ny rows padded to
// sp = roundup(nx, 4) floats, twice (ping-pong), in one allocation.  Cell
// (x, y, z), speed k of set s at g[s] + k * plane + (z * ny + y) * sp + x.  The
// pad columns are zeroed at begin and never read or written afterwards.
//
// Index safety: every neighbour index is formed from a cell inside the domain
// by `c == 0 ? n - 1 : c - 1` or `c + 1 == n ? 0 : c + 1`, the fixed list is
// checked against the extents before it reaches the device.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "lbm_diag_host.hpp"
#include "lbm_quad.hpp"
#include "lbm_scalar_hip.h"

namespace lbm {
namespace scalar {

#define LBM_HD __host__ __device__ __forceinline__

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 8192;  // grid-stride beyond; also the most partials the host folds per part
constexpr int MAX_PARTS = LBM_SCALAR_MAX_PARTS;

// ---- the per-cell arithmetic (host and device) ----

// D2Q5: p[k] is the population that arrives along speed k (0 rest, 1 E, 2 N, 3 W, 4 S).  Both outcomes are formed
// and one is selected: a branch on `blocked` lets the compiler sink the flow loads behind the velocity into it,
// where they become 4-B loads.
LBM_HD void cell2(const float (&p)[5], bool blocked, float ux, float uy, float omega, float (&out)[5]) {
    constexpr int opp[5] = {0, 3, 4, 1, 2};
    const float phi = (((p[0] + p[1]) + p[2]) + p[3]) + p[4];
    const float e0 = phi * (1.f / 3.f);
    const float t = phi * (1.f / 6.f);
    const float a = t * (3.f * ux);
    const float b = t * (3.f * uy);
    const float e[5] = {e0, t + a, t + b, t - a, t - b};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const float relaxed = p[k] + omega * (e[k] - p[k]);
        out[k] = blocked ? p[opp[k]] : relaxed;
    }
}

// D3Q7: 0 rest, 1 +x, 2 -x, 3 +y, 4 -y, 5 +z, 6 -z
LBM_HD void cell3(const float (&p)[7], bool blocked, float ux, float uy, float uz, float omega, float (&out)[7]) {
    constexpr int opp[7] = {0, 2, 1, 4, 3, 6, 5};
    float phi = p[0];
#pragma unroll
    for (int k = 1; k < 7; ++k) phi += p[k];
    const float e0 = phi * 0.25f;
    const float t = phi * 0.125f;
    const float a = t * (4.f * ux);
    const float b = t * (4.f * uy);
    const float c = t * (4.f * uz);
    const float e[7] = {e0, t + a, t - a, t + b, t - b, t + c, t - c};
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float relaxed = p[k] + omega * (e[k] - p[k]);
        out[k] = blocked ? p[opp[k]] : relaxed;
    }
}

LBM_HD int below(int c, int n) { return c == 0 ? n - 1 : c - 1; }
LBM_HD int above(int c, int n) { return c + 1 == n ? 0 : c + 1; }

// ---- the buoyancy kick (include/lbm_thermal_hip.h), host and device ----
//
// Per opposite pair of flow speeds one increment: added to the first speed of the pair, subtracted from the
// second.  The pairs, in the order of the increments kick2_inc / kick3_inc form:
constexpr int KICK2_PAIRS = 4, KICK3_PAIRS = 9;
LBM_HD int kick2_plus(int j) {
    constexpr int t[KICK2_PAIRS] = {1, 2, 5, 6};
    return t[j];
}
LBM_HD int kick2_minus(int j) {
    constexpr int t[KICK2_PAIRS] = {3, 4, 7, 8};
    return t[j];
}
LBM_HD int kick3_plus(int j) {
    constexpr int t[KICK3_PAIRS] = {1, 3, 9, 5, 7, 10, 11, 12, 13};
    return t[j];
}
LBM_HD int kick3_minus(int j) {
    constexpr int t[KICK3_PAIRS] = {2, 4, 14, 6, 8, 15, 16, 17, 18};
    return t[j];
}

// the scalar of a cell: its Q stored populations summed in speed order
template <int Q>
LBM_HD float cell_phi(const float (&g)[Q]) {
    float phi = g[0];
#pragma unroll
    for (int k = 1; k < Q; ++k) phi += g[k];
    return phi;
}

// D2Q9: E/W, N/S, NE/SW, NW/SE
// the pair increments of the momentum (jx, jy); the forcing zones (lbm_forcing.hpp) form theirs through it too
LBM_HD void kick2_pairs(float jx, float jy, float (&inc)[KICK2_PAIRS]) {
    inc[0] = jx * (1.f / 3.f);
    inc[1] = jy * (1.f / 3.f);
    const float bx = jx * (1.f / 12.f), by = jy * (1.f / 12.f);
    inc[2] = bx + by;
    inc[3] = by - bx;
}

LBM_HD void kick2_inc(float phi, float phi_ref, float kx, float ky, float (&inc)[KICK2_PAIRS]) {
    const float d = phi - phi_ref;
    kick2_pairs(kx * d, ky * d, inc);
}

// D3Q19: +-x, +-y, +-z, then the six diagonal pairs in the order of kick3_plus
LBM_HD void kick3_pairs(float jx, float jy, float jz, float (&inc)[KICK3_PAIRS]) {
    inc[0] = jx * (1.f / 6.f);
    inc[1] = jy * (1.f / 6.f);
    inc[2] = jz * (1.f / 6.f);
    const float bx = jx * (1.f / 12.f), by = jy * (1.f / 12.f), bz = jz * (1.f / 12.f);
    inc[3] = bx + by;
    inc[4] = bx - by;
    inc[5] = bx + bz;
    inc[6] = bz - bx;
    inc[7] = by + bz;
    inc[8] = bz - by;
}

LBM_HD void kick3_inc(float phi, float phi_ref, float kx, float ky, float kz, float (&inc)[KICK3_PAIRS]) {
    const float d = phi - phi_ref;
    kick3_pairs(kx * d, ky * d, kz * d, inc);
}

// One pair of one cell.  A select of the loaded value, not an added zero: an obstacle cell keeps its bits
// (-0.f + 0.f is +0.f), and a branch here would sink the 16-B loads into it.
LBM_HD void kick_pair(float &plus, float &minus, bool blocked, float inc) {
    const float up = plus + inc, down = minus - inc;
    plus = blocked ? plus : up;
    minus = blocked ? minus : down;
}

// ---- the scalar lattice of a handle ----

struct Grid {
    int nx, ny, nz, sp;
    long long plane;  // floats of one speed plane: nz * ny * sp
};

// The cells a launch of the shared kernels owns: the w x h x d cells at (x0, y0, z0) and their obstacle bytes
// uint8[d][h][w] (a D2Q9 sub-domain, a D3Q19 slab).
struct Region {
    const uint8_t *obst;
    int x0, y0, z0, w, h, d;
};

struct Walls;                 // wall models and the wall list of a scalar (lbm_scalar_walls.hpp)
void walls_free(Walls *w);    // lbm_scalar_walls.hip; NULL allowed, the device of the state current
struct State;
// The wall pass on set g, enqueued on st: D2Q5 (lbm_scalar_walls.hip) and D3Q7 (lbm3d_scalar_walls.hip).  Only
// where walls_listed(s): a state without walls, or with no labelled wall cell, launches nothing.
bool walls_listed(const State &s);
hipError_t walls_pass2d(const State &s, float *g, hipStream_t st);
hipError_t walls_pass3d(const State &s, float *g, hipStream_t st);

struct State {
    int dev = 0, q = 0;
    Grid grid{};
    float w0 = 0.f, w1 = 0.f;  // begin weights of the rest speed and of a moving one
    float omega = 0.f;
    float *g[2] = {nullptr, nullptr};
    int cur = 0;
    long long steps = 0;
    long long nfixed = 0;
    long long *fix_cell = nullptr;  // offset of each fixed cell inside a speed plane
    float *fix_value = nullptr;
    Walls *walls = nullptr;  // set by *_scalar_set_walls (include/lbm_scalar_walls_hip.h); NULL: none
    size_t set_floats() const { return (size_t)q * (size_t)grid.plane; }
};

// ---- kernels both engines share ----

template <int Q>
__global__ __launch_bounds__(BLOCK) void scalar_fixed(float *g, long long plane, const long long *cell,
                                                      const float *value, long long n, float w0, float w1) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * BLOCK) {
        const float v = value[i];
        float *dst = g + cell[i];
        dst[0] = v * w0;
        const float m = v * w1;
#pragma unroll
        for (int k = 1; k < Q; ++k) dst[k * plane] = m;
    }
}

// phi of every entry of a plane (pad columns too: they hold zeros)
template <int Q>
__global__ __launch_bounds__(BLOCK) void scalar_phi(const float *g, long long plane, float *phi) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < plane; i += (long long)gridDim.x * BLOCK) {
        float s = g[i];
#pragma unroll
        for (int k = 1; k < Q; ++k) s += g[k * plane + i];
        phi[i] = s;
    }
}

// Per block: the fp64 sum of the fp32 phi of its cells of the region and, over its fluid cells, max phi and
// max -phi, folded in a fixed order (fold_block, lbm_quad.hpp).
template <int Q>
__global__ __launch_bounds__(BLOCK) void scalar_stats(const float *g, Grid grid, Region r, double *sum_part,
                                                      float *max_part) {
    const long long cells = (long long)r.w * r.h * r.d;
    double s[1] = {0.0};
    float m[2] = {-INFINITY, -INFINITY};
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < cells; i += (long long)gridDim.x * BLOCK) {
        const long long row = i / r.w;
        const int lx = (int)(i - row * r.w);
        const int lz = (int)(row / r.h);
        const int ly = (int)(row - (long long)lz * r.h);
        const float *src = g + ((long long)(r.z0 + lz) * grid.ny + (r.y0 + ly)) * grid.sp + (r.x0 + lx);
        float phi = src[0];
#pragma unroll
        for (int k = 1; k < Q; ++k) phi += src[k * grid.plane];
        s[0] += (double)phi;
        if (r.obst[i] == 0) {
            m[0] = fmaxf(m[0], phi);
            m[1] = fmaxf(m[1], -phi);
        }
    }
    fold_block<BLOCK / 64>(s, m, blockIdx.x, gridDim.x, sum_part, max_part);
}

inline int blocks_for(long long n) {
    const long long b = (n + BLOCK - 1) / BLOCK;
    return (int)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

// ---- host side both engines share ----

inline void check_omega(float omega) {
    if (!(std::isfinite(omega) && omega > 0.f && omega < 2.f))
        throw lbm_failure(LBM_E_INVALID, "omega_s must be finite and inside (0, 2)");
}

inline void release(State *s) {
    if (!s) return;
    if (hipSetDevice(s->dev) == hipSuccess) {
        (void)hipFree(s->g[0]);
        (void)hipFree(s->fix_cell);
        (void)hipFree(s->fix_value);
        walls_free(s->walls);
    }
    delete s;
}

inline void end(State *&s) {
    release(s);
    s = nullptr;
}

// The begin state of phi0 (NULL: zeros) on device dev (the current device on return); `old` is replaced only
// once the new state stands.
inline void begin(State *&old, int dev, int q, int nx, int ny, int nz, float omega, const float *phi0) {
    check_omega(omega);
    HIP_CHECK(hipSetDevice(dev));
    State *s = new State;
    s->dev = dev;
    s->q = q;
    s->grid.nx = nx;
    s->grid.ny = ny;
    s->grid.nz = nz;
    s->grid.sp = (nx + 3) / 4 * 4;
    s->grid.plane = (long long)nz * ny * s->grid.sp;
    s->w0 = q == 5 ? 1.f / 3.f : 0.25f;
    s->w1 = q == 5 ? 1.f / 6.f : 0.125f;
    s->omega = omega;
    const size_t bytes = sizeof(float) * 2 * s->set_floats();
    if (hipMalloc((void **)&s->g[0], bytes) != hipSuccess) {
        (void)hipGetLastError();
        delete s;
        throw lbm_failure(LBM_E_NOMEM, "no device memory for the scalar lattice");
    }
    s->g[1] = s->g[0] + s->set_floats();
    try {
        HIP_CHECK(hipMemset(s->g[0], 0, bytes));
        if (phi0) {
            // the rest plane and one moving plane on the host, padded; the other moving planes are device copies
            const size_t rows = (size_t)nz * ny, sp = (size_t)s->grid.sp;
            std::vector<float> host(rows * sp, 0.f);
            for (int pass = 0; pass < 2; ++pass) {
                const float w = pass == 0 ? s->w0 : s->w1;
                for (size_t r = 0; r < rows; ++r)
                    for (int x = 0; x < nx; ++x) host[r * sp + x] = phi0[r * nx + x] * w;
                HIP_CHECK(hipMemcpy(s->g[0] + (size_t)pass * s->grid.plane, host.data(), sizeof(float) * rows * sp,
                                    hipMemcpyHostToDevice));
            }
            for (int k = 2; k < q; ++k)
                HIP_CHECK(hipMemcpy(s->g[0] + (size_t)k * s->grid.plane, s->g[0] + s->grid.plane,
                                    sizeof(float) * rows * sp, hipMemcpyDeviceToDevice));
        }
    } catch (...) {
        release(s);
        throw;
    }
    release(old);
    old = s;
}

template <int Q, class Around>
void apply_fixed(const State &s, float *g, hipStream_t st, Around &&around) {
    if (s.nfixed == 0) return;
    around([&] {
        hipLaunchKernelGGL(scalar_fixed<Q>, dim3(blocks_for(s.nfixed)), dim3(BLOCK), 0, st, g, s.grid.plane,
                           s.fix_cell, s.fix_value, s.nfixed, s.w0, s.w1);
        HIP_CHECK(hipGetLastError());
    });
}

// Checks the list (z NULL: 2-D), replaces the old one and applies it once to the current set.
template <int Q, class Around>
void set_fixed(State &s, int64_t n, const int32_t *x, const int32_t *y, const int32_t *z, bool need_z,
               const float *value, hipStream_t st, Around &&around) {
    if (n < 0) throw lbm_failure(LBM_E_INVALID, "the fixed list holds n >= 0 cells");
    if (n > 0 && (!x || !y || (need_z && !z) || !value)) throw lbm_failure(LBM_E_INVALID, "NULL fixed-cell array");
    const Grid &gr = s.grid;
    std::vector<long long> cell((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int zi = need_z ? z[i] : 0;
        if (x[i] < 0 || x[i] >= gr.nx || y[i] < 0 || y[i] >= gr.ny || zi < 0 || zi >= gr.nz)
            throw lbm_failure(LBM_E_INVALID, "fixed cell " + std::to_string(i) + " lies outside the domain");
        cell[(size_t)i] = ((long long)zi * gr.ny + y[i]) * gr.sp + x[i];
    }
    std::vector<long long> sorted(cell);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
        throw lbm_failure(LBM_E_INVALID, "a cell is listed twice in the fixed list");
    HIP_CHECK(hipSetDevice(s.dev));
    long long *dc = nullptr;
    float *dv = nullptr;
    if (n > 0) {
        if (hipMalloc((void **)&dc, sizeof(long long) * (size_t)n) != hipSuccess ||
            hipMalloc((void **)&dv, sizeof(float) * (size_t)n) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(dc);
            throw lbm_failure(LBM_E_NOMEM, "no device memory for the fixed list");
        }
        const hipError_t e1 = hipMemcpy(dc, cell.data(), sizeof(long long) * (size_t)n, hipMemcpyHostToDevice);
        const hipError_t e2 = hipMemcpy(dv, value, sizeof(float) * (size_t)n, hipMemcpyHostToDevice);
        if (e1 != hipSuccess || e2 != hipSuccess) {
            (void)hipFree(dc);
            (void)hipFree(dv);
            HIP_CHECK(e1);
            HIP_CHECK(e2);
        }
    }
    (void)hipFree(s.fix_cell);
    (void)hipFree(s.fix_value);
    s.fix_cell = dc;
    s.fix_value = dv;
    s.nfixed = n;
    apply_fixed<Q>(s, s.g[s.cur], st, around);
    HIP_CHECK(hipStreamSynchronize(st));
}

// phi (float[nz][ny][nx]) and the populations (planar, unpadded) of the current set; NULL skipped
template <int Q>
void store(const State &s, float *phi, float *g, hipStream_t st) {
    const Grid &gr = s.grid;
    const size_t rows = (size_t)gr.nz * gr.ny;
    HIP_CHECK(hipSetDevice(s.dev));
    if (phi) {
        const DeviceStage stage(sizeof(float) * (size_t)gr.plane);
        hipLaunchKernelGGL(scalar_phi<Q>, dim3(blocks_for(gr.plane)), dim3(BLOCK), 0, st, s.g[s.cur], gr.plane,
                           stage.as<float>());
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipMemcpy2D(phi, sizeof(float) * gr.nx, stage.get(), sizeof(float) * gr.sp, sizeof(float) * gr.nx,
                              rows, hipMemcpyDeviceToHost));
    }
    if (g)
        for (int k = 0; k < Q; ++k)
            HIP_CHECK(hipMemcpy2D(g + (size_t)k * rows * gr.nx, sizeof(float) * gr.nx,
                                  s.g[s.cur] + (size_t)k * gr.plane, sizeof(float) * gr.sp, sizeof(float) * gr.nx,
                                  rows, hipMemcpyDeviceToHost));
}

// The statistics of one region into the running totals (sum; m[0] = max phi, m[1] = max -phi), part after part.
template <int Q, class Around>
void stats_region(const State &s, const Region &r, hipStream_t st, double (&sum)[1], float (&m)[2], Around &&around) {
    const int nb = blocks_for((long long)r.w * r.h * r.d);
    const BlockPartials<1, 2> part((size_t)nb);
    around([&] {
        hipLaunchKernelGGL(scalar_stats<Q>, dim3(nb), dim3(BLOCK), 0, st, s.g[s.cur], s.grid, r, part.sums(),
                           part.maxima());
        HIP_CHECK(hipGetLastError());
    });
    HIP_CHECK(hipStreamSynchronize(st));
    part.fold(sum, m);
}

inline void stats_out(const double (&sum)[1], const float (&m)[2], double *total, float *min, float *max) {
    if (total) *total = sum[0];
    if (min) *min = -m[1];
    if (max) *max = m[0];
}

// the *_ref entry points
inline bool ref_args_ok(int nx, int ny, int nz, float omega, std::initializer_list<const void *> arrays) {
    if (nx < 1 || ny < 1 || nz < 1 || !(std::isfinite(omega) && omega > 0.f && omega < 2.f)) return false;
    for (const void *p : arrays)
        if (!p) return false;
    return true;
}

// the *_buoyancy_ref entry points
inline bool kick_args_ok(int nx, int ny, int nz, std::initializer_list<float> numbers,
                         std::initializer_list<const void *> arrays) {
    if (nx < 1 || ny < 1 || nz < 1) return false;
    for (float v : numbers)
        if (!std::isfinite(v)) return false;
    for (const void *p : arrays)
        if (!p) return false;
    return true;
}

// The launch shape of the D3Q19 kernels that walk a box of a slab a row of lanes at a time (lbm3d_scalar.hip; the
// forcing zones of lbm3d_forcing.hip launch on it too): the grid over the view's box, the lanes of a block along x
// and its rows.
dim3 slab_grid(const Box3View &a);
int slab_lanes_x();
int slab_rows();

#undef LBM_HD

}  // namespace scalar
}  // namespace lbm
