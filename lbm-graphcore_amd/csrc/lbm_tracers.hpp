// lbm_tracers.hpp -- Lagrangian tracers and point probes of both engines
// (lbm_tracers.hip, lbm3d_tracers.hip; include/lbm_tracers_hip.h): the
// per-point arithmetic, compiled for the device and for the host from one
// text, the fields it reads cells through, the kernels as templates over those
// fields, and the point set both handles keep.
//
// The per-point functions (wrap, split, interp2 / interp3, advance2 /
// advance3, nearest) are the header's definition, fp64, as written, no
// contraction (-ffp-contract=off).  They read cells through a field F with
//   F::nx, ny[, nz]                        the periodic extents
//   F::row(i0, i1, j[, k], a, b)           the values of cells (i0, j[, k]) and (i1, j[, k])
//   F::blocked(i, j[, k])                  the obstacle flag of a cell
// Planar2 / Planar3 are host arrays float[ny][nx] / float[nz][ny][nx] (the
// *_ref entry points); Lattice2 / Lattice3 are the device lattices of every
// local sub-domain / slab, whose cell values are cell_macro / cell3_macro of
// the stored populations -- the text lbm_store_fields compiles, so the values
// are those fields widened to double by construction.
//
// The gather.  One point per lane, 256-lane blocks, grid-stride, no LDS, no
// atomics: each point has one owner lane.  Per interpolation a lane reads the
// 4 (2-D) or 8 (3-D) surrounding cells: Q populations and the obstacle byte
// each, Q 4-B loads per cell, the two x-neighbours of a row issued together
// (where i1 == i0 + 1 inside one sub-domain they are adjacent floats of every
// speed plane: one 64-B segment unless they straddle it).  Neighbouring lanes
// hold unrelated points, so nothing coalesces across lanes: the kernel is
// bound by the number of 64-B segments it touches, 2 Q per row pair, and by
// the L2 / Infinity Cache hit rate of the point distribution.  Bytes a point
// needs: 4 x 37 B (2-D), 8 x 77 B (3-D) per interpolation, twice for Heun,
// plus 16 / 24 B of position read and written.
//
// Index safety rests on one invariant: a stored position p satisfies
// 0 <= p < n per coordinate.  begin checks the seeds, wrap() restores it after
// every move whatever the lattice holds (NaN, Inf), and every index formed
// from a position in range is in range: floor(p) in [0, n - 1], its periodic
// successor, and floor(p + 0.5) in [0, n] taken to 0 at n.  No other clamp.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "lbm3d_cell_macro.hpp"
#include "lbm_cell_macro.hpp"
#include "lbm_diag_host.hpp"
#include "lbm_tracers_hip.h"
#include "lbm_views.hpp"

namespace lbm {
namespace tracer {

#define LBM_HD __host__ __device__ __forceinline__

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 8192;  // grid-stride beyond
constexpr int MAX_VIEWS = LBM_TRACER_MAX_PARTS;

// ---- the per-point arithmetic (host and device) ----

LBM_HD double wrap(double v, int extent) {
    const double n = (double)extent;
    double r = v - n * floor(v / n);
    if (!(r >= 0.0 && r < n)) r = 0.0;
    return r;
}

LBM_HD double lerp(double a, double b, double t) { return a + t * (b - a); }

// x in [0, n): the cell below, its periodic successor and the fraction
LBM_HD void split(double x, int n, int &i0, int &i1, double &t) {
    i0 = (int)floor(x);
    t = x - (double)i0;
    i1 = (i0 + 1 == n) ? 0 : i0 + 1;
}

LBM_HD int nearest(double x, int n) {
    const int i = (int)floor(x + 0.5);
    return i == n ? 0 : i;
}

struct Val2 {
    double ux, uy, p;
};
struct Val3 {
    double ux, uy, uz, p;
};

LBM_HD Val2 lerp(const Val2 &a, const Val2 &b, double t) {
    return Val2{lerp(a.ux, b.ux, t), lerp(a.uy, b.uy, t), lerp(a.p, b.p, t)};
}
LBM_HD Val3 lerp(const Val3 &a, const Val3 &b, double t) {
    return Val3{lerp(a.ux, b.ux, t), lerp(a.uy, b.uy, t), lerp(a.uz, b.uz, t), lerp(a.p, b.p, t)};
}

template <class F>
LBM_HD Val2 interp2(const F &f, double x, double y) {
    int i0, i1, j0, j1;
    double tx, ty;
    split(x, f.nx, i0, i1, tx);
    split(y, f.ny, j0, j1, ty);
    Val2 a, b;
    f.row(i0, i1, j0, a, b);
    const Val2 lo = lerp(a, b, tx);
    f.row(i0, i1, j1, a, b);
    const Val2 hi = lerp(a, b, tx);
    return lerp(lo, hi, ty);
}

template <class F>
LBM_HD Val3 interp3(const F &f, double x, double y, double z) {
    int i0, i1, j0, j1, k0, k1;
    double tx, ty, tz;
    split(x, f.nx, i0, i1, tx);
    split(y, f.ny, j0, j1, ty);
    split(z, f.nz, k0, k1, tz);
    Val3 a, b;
    f.row(i0, i1, j0, k0, a, b);
    const Val3 c00 = lerp(a, b, tx);
    f.row(i0, i1, j1, k0, a, b);
    const Val3 c10 = lerp(a, b, tx);
    const Val3 lo = lerp(c00, c10, ty);
    f.row(i0, i1, j0, k1, a, b);
    const Val3 c01 = lerp(a, b, tx);
    f.row(i0, i1, j1, k1, a, b);
    const Val3 c11 = lerp(a, b, tx);
    const Val3 hi = lerp(c01, c11, ty);
    return lerp(lo, hi, tz);
}

template <class F>
LBM_HD void advance2(const F &f, double &x, double &y, double dt, int scheme) {
    const Val2 k1 = interp2(f, x, y);
    double h = dt, sx = k1.ux, sy = k1.uy;
    if (scheme == LBM_TRACER_HEUN) {
        const Val2 k2 = interp2(f, wrap(x + dt * k1.ux, f.nx), wrap(y + dt * k1.uy, f.ny));
        h = 0.5 * dt;
        sx = k1.ux + k2.ux;
        sy = k1.uy + k2.uy;
    }
    x = wrap(x + h * sx, f.nx);
    y = wrap(y + h * sy, f.ny);
}

template <class F>
LBM_HD void advance3(const F &f, double &x, double &y, double &z, double dt, int scheme) {
    const Val3 k1 = interp3(f, x, y, z);
    double h = dt, sx = k1.ux, sy = k1.uy, sz = k1.uz;
    if (scheme == LBM_TRACER_HEUN) {
        const Val3 k2 =
            interp3(f, wrap(x + dt * k1.ux, f.nx), wrap(y + dt * k1.uy, f.ny), wrap(z + dt * k1.uz, f.nz));
        h = 0.5 * dt;
        sx = k1.ux + k2.ux;
        sy = k1.uy + k2.uy;
        sz = k1.uz + k2.uz;
    }
    x = wrap(x + h * sx, f.nx);
    y = wrap(y + h * sy, f.ny);
    z = wrap(z + h * sz, f.nz);
}

// ---- host fields: planar fp32 arrays (a NULL array reads as 0) ----

struct Planar2 {
    const float *ux, *uy, *p;
    int nx, ny;
    LBM_HD Val2 at(int i, int j) const {
        const size_t o = (size_t)j * nx + i;
        return Val2{ux ? (double)ux[o] : 0.0, uy ? (double)uy[o] : 0.0, p ? (double)p[o] : 0.0};
    }
    LBM_HD void row(int i0, int i1, int j, Val2 &a, Val2 &b) const {
        a = at(i0, j);
        b = at(i1, j);
    }
};

struct Planar3 {
    const float *ux, *uy, *uz, *p;
    int nx, ny, nz;
    LBM_HD Val3 at(int i, int j, int k) const {
        const size_t o = ((size_t)k * ny + j) * nx + i;
        return Val3{ux ? (double)ux[o] : 0.0, uy ? (double)uy[o] : 0.0, uz ? (double)uz[o] : 0.0,
                    p ? (double)p[o] : 0.0};
    }
    LBM_HD void row(int i0, int i1, int j, int k, Val3 &a, Val3 &b) const {
        a = at(i0, j, k);
        b = at(i1, j, k);
    }
};

// ---- device fields: the current lattices of every local sub-domain / slab ----

// one D2Q9 sub-domain and the cell of the domain its (0, 0) is
struct View2 {
    LatticeView v;
    int x0, y0;
};

// The sub-domains tile the domain, so the last view owns whatever no earlier one does.
struct Lattice2 {
    View2 view[MAX_VIEWS];
    int nviews, nx, ny;

    __device__ __forceinline__ const View2 &owner(int i, int j) const {
        int k = 0;
        for (; k < nviews - 1; ++k) {
            const View2 &q = view[k];
            if ((unsigned)(i - q.x0) < (unsigned)q.v.w && (unsigned)(j - q.y0) < (unsigned)q.v.h) break;
        }
        return view[k];
    }
    static __device__ __forceinline__ Val2 value(const float (&c)[9], bool blocked, float obst_pressure) {
        float rho;
        const CellMacro m = cell_macro<true, false>(c, blocked, obst_pressure, rho);
        return Val2{(double)m.ux, (double)m.uy, (double)m.pressure};
    }
    __device__ __forceinline__ void row(int i0, int i1, int j, Val2 &a, Val2 &b) const {
        const View2 &q = owner(i0, j);
        const int lx = i0 - q.x0, ly = j - q.y0;
        const float *s0 = q.v.o + (long long)ly * q.v.pitch + lx;
        const uint8_t *m0 = q.v.obst + (long long)ly * q.v.w + lx;
        const float *s1 = s0 + 1;
        const uint8_t *m1 = m0 + 1;
        long long plane1 = q.v.plane;
        float op1 = q.v.obst_pressure;
        if (!(i1 == i0 + 1 && lx + 1 < q.v.w)) {
            // the successor wraps round the domain or lies in the next sub-domain
            const View2 &r = owner(i1, j);
            const int rx = i1 - r.x0, ry = j - r.y0;
            s1 = r.v.o + (long long)ry * r.v.pitch + rx;
            m1 = r.v.obst + (long long)ry * r.v.w + rx;
            plane1 = r.v.plane;
            op1 = r.v.obst_pressure;
        }
        float c0[9], c1[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            c0[k] = s0[k * q.v.plane];
            c1[k] = s1[k * plane1];
        }
        a = value(c0, *m0 != 0, q.v.obst_pressure);
        b = value(c1, *m1 != 0, op1);
    }
    __device__ __forceinline__ bool blocked(int i, int j) const {
        const View2 &q = owner(i, j);
        return q.v.obst[(long long)(j - q.y0) * q.v.w + (i - q.x0)] != 0;
    }
};

// one D3Q19 slab: the view of all its cells (box origin 0, extents nx, ny, nzs) and its first plane
struct View3 {
    Box3View v;
    int gz0;
};

struct Lattice3 {
    View3 view[MAX_VIEWS];
    int nviews, nx, ny, nz;

    __device__ __forceinline__ const View3 &owner(int k) const {
        int s = 0;
        for (; s < nviews - 1; ++s)
            if ((unsigned)(k - view[s].gz0) < (unsigned)view[s].v.bz) break;
        return view[s];
    }
    static __device__ __forceinline__ Val3 value(const float (&c)[19], bool blocked, float obst_pressure) {
        float rho;
        const Cell3Macro m = cell3_macro<true, false>(c, blocked, obst_pressure, rho);
        return Val3{(double)m.ux, (double)m.uy, (double)m.uz, (double)m.pressure};
    }
    __device__ __forceinline__ void row(int i0, int i1, int j, int k, Val3 &a, Val3 &b) const {
        const View3 &q = owner(k);
        const long long lz = k - q.gz0;
        const float *src = q.v.o + lz * q.v.PL + (long long)j * q.v.px;
        const uint8_t *map = q.v.obst + (lz * q.v.ny + j) * q.v.nx;
        float c0[19], c1[19];
#pragma unroll
        for (int s = 0; s < 19; ++s) {
            c0[s] = src[s * q.v.KS + i0];
            c1[s] = src[s * q.v.KS + i1];
        }
        a = value(c0, map[i0] != 0, q.v.obst_pressure);
        b = value(c1, map[i1] != 0, q.v.obst_pressure);
    }
    __device__ __forceinline__ bool blocked(int i, int j, int k) const {
        const View3 &q = owner(k);
        const long long lz = k - q.gz0;
        return q.v.obst[(lz * q.v.ny + j) * q.v.nx + i] != 0;
    }
};

// ---- kernels ----

// The points of a set: SoA doubles c[d][n]; and what a launch writes besides.
template <int DIM>
struct Points {
    double *c[DIM];
    long long n;
};

template <class F>
struct AdvanceArgs {
    F f;
    Points<F::DIM> pts;
    double dt;
    int scheme;
};

// out[d] (d < DIM: velocity component d, d == DIM: pressure): NULL is not written
template <class F>
struct SampleArgs {
    F f;
    Points<F::DIM> pts;
    double *out[F::DIM + 1];
};

template <class F>
struct FlagArgs {
    F f;
    Points<F::DIM> pts;
    uint8_t *flag;
};

struct Dev2 : Lattice2 {
    static constexpr int DIM = 2;
};
struct Dev3 : Lattice3 {
    static constexpr int DIM = 3;
};

__device__ __forceinline__ void point_advance(const AdvanceArgs<Dev2> &a, long long i) {
    double x = a.pts.c[0][i], y = a.pts.c[1][i];
    advance2(a.f, x, y, a.dt, a.scheme);
    a.pts.c[0][i] = x;
    a.pts.c[1][i] = y;
}
__device__ __forceinline__ void point_advance(const AdvanceArgs<Dev3> &a, long long i) {
    double x = a.pts.c[0][i], y = a.pts.c[1][i], z = a.pts.c[2][i];
    advance3(a.f, x, y, z, a.dt, a.scheme);
    a.pts.c[0][i] = x;
    a.pts.c[1][i] = y;
    a.pts.c[2][i] = z;
}
__device__ __forceinline__ void point_sample(const SampleArgs<Dev2> &a, long long i) {
    const Val2 v = interp2(a.f, a.pts.c[0][i], a.pts.c[1][i]);
    if (a.out[0]) a.out[0][i] = v.ux;
    if (a.out[1]) a.out[1][i] = v.uy;
    if (a.out[2]) a.out[2][i] = v.p;
}
__device__ __forceinline__ void point_sample(const SampleArgs<Dev3> &a, long long i) {
    const Val3 v = interp3(a.f, a.pts.c[0][i], a.pts.c[1][i], a.pts.c[2][i]);
    if (a.out[0]) a.out[0][i] = v.ux;
    if (a.out[1]) a.out[1][i] = v.uy;
    if (a.out[2]) a.out[2][i] = v.uz;
    if (a.out[3]) a.out[3][i] = v.p;
}
__device__ __forceinline__ void point_flag(const FlagArgs<Dev2> &a, long long i) {
    a.flag[i] = a.f.blocked(nearest(a.pts.c[0][i], a.f.nx), nearest(a.pts.c[1][i], a.f.ny)) ? 1 : 0;
}
__device__ __forceinline__ void point_flag(const FlagArgs<Dev3> &a, long long i) {
    a.flag[i] = a.f.blocked(nearest(a.pts.c[0][i], a.f.nx), nearest(a.pts.c[1][i], a.f.ny),
                            nearest(a.pts.c[2][i], a.f.nz))
                    ? 1
                    : 0;
}

template <class F>
__global__ __launch_bounds__(BLOCK) void advance_tracers(AdvanceArgs<F> a) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.pts.n; i += (long long)gridDim.x * BLOCK)
        point_advance(a, i);
}

template <class F>
__global__ __launch_bounds__(BLOCK) void sample_tracers(SampleArgs<F> a) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.pts.n; i += (long long)gridDim.x * BLOCK)
        point_sample(a, i);
}

template <class F>
__global__ __launch_bounds__(BLOCK) void flag_tracers(FlagArgs<F> a) {
    for (long long i = (long long)blockIdx.x * BLOCK + threadIdx.x; i < a.pts.n; i += (long long)gridDim.x * BLOCK)
        point_flag(a, i);
}

inline int blocks_for(long long n) {
    const long long b = (n + BLOCK - 1) / BLOCK;
    return (int)(b < 1 ? 1 : b > MAX_BLOCKS ? MAX_BLOCKS : b);
}

// ---- the point set a handle keeps, and the host side both engines share ----

// n points of `dims` coordinates on device `dev`: SoA doubles c(d)[n] in one allocation
struct State {
    int dev = 0, dims = 0;
    long long n = 0;
    double *pos = nullptr;
    double *c(int d) const { return pos + (size_t)d * n; }
    template <int DIM>
    Points<DIM> points() const {
        Points<DIM> p;
        for (int d = 0; d < DIM; ++d) p.c[d] = c(d);
        p.n = n;
        return p;
    }
};

// Every seed finite and inside [0, extent[d]): else LBM_E_INVALID.  Nothing is allocated before this holds.
inline void check_seeds(int dims, const int *extent, long long n, const double *const *seed) {
    if (n < 1) throw lbm_failure(LBM_E_INVALID, "a tracer set holds at least one point");
    for (int d = 0; d < dims; ++d) {
        if (!seed[d]) throw lbm_failure(LBM_E_INVALID, "NULL seed array");
        const double hi = (double)extent[d];
        for (long long i = 0; i < n; ++i)
            if (!(seed[d][i] >= 0.0 && seed[d][i] < hi))
                throw lbm_failure(LBM_E_INVALID, "seed " + std::to_string(i) + ": coordinate " + std::to_string(d) +
                                                     " is not finite or lies outside [0, " +
                                                     std::to_string(extent[d]) + ")");
    }
}

// The checked seeds on device dev (the current device on return); `old` is replaced only once the new set stands.
inline void begin(State *&old, int dev, int dims, long long n, const double *const *seed) {
    HIP_CHECK(hipSetDevice(dev));
    State *s = new State{dev, dims, n, nullptr};
    const hipError_t e = hipMalloc((void **)&s->pos, sizeof(double) * (size_t)dims * (size_t)n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        delete s;
        throw lbm_failure(LBM_E_NOMEM, "no device memory for the tracer set");
    }
    for (int d = 0; d < dims; ++d) {
        const hipError_t c = hipMemcpy(s->c(d), seed[d], sizeof(double) * (size_t)n, hipMemcpyHostToDevice);
        if (c != hipSuccess) {
            (void)hipFree(s->pos);
            delete s;
            HIP_CHECK(c);
        }
    }
    if (old) {
        (void)hipFree(old->pos);
        delete old;
    }
    old = s;
}

inline void end(State *&s) {
    if (!s) return;
    if (hipSetDevice(s->dev) == hipSuccess) (void)hipFree(s->pos);
    delete s;
    s = nullptr;
}

// `around(launch)` runs the launch (the D2Q9 handle brackets it with its profile events).
template <class F, class Around>
void run_advance(const F &f, const State &s, double dt, int scheme, hipStream_t st, Around &&around) {
    if (!std::isfinite(dt)) throw lbm_failure(LBM_E_INVALID, "dt must be finite");
    if (scheme != LBM_TRACER_EULER && scheme != LBM_TRACER_HEUN)
        throw lbm_failure(LBM_E_INVALID, "scheme must be LBM_TRACER_EULER or LBM_TRACER_HEUN");
    const AdvanceArgs<F> a{f, s.points<F::DIM>(), dt, scheme};
    around([&] {
        hipLaunchKernelGGL(advance_tracers<F>, dim3(blocks_for(s.n)), dim3(BLOCK), 0, st, a);
        HIP_CHECK(hipGetLastError());
    });
    HIP_CHECK(hipStreamSynchronize(st));
}

// host[d] (F::DIM + 1 entries: the velocity components, then pressure): NULL is neither computed nor copied
template <class F, class Around>
void run_sample(const F &f, const State &s, double *const *host, hipStream_t st, Around &&around) {
    constexpr int NO = F::DIM + 1;
    const int want = count_wanted(host, NO);
    const DeviceStage stage(sizeof(double) * (size_t)want * (size_t)s.n);
    SampleArgs<F> a{f, s.points<F::DIM>(), {}};
    for (int d = 0, k = 0; d < NO; ++d) a.out[d] = host[d] ? stage.as<double>() + (size_t)s.n * k++ : nullptr;
    around([&] {
        hipLaunchKernelGGL(sample_tracers<F>, dim3(blocks_for(s.n)), dim3(BLOCK), 0, st, a);
        HIP_CHECK(hipGetLastError());
    });
    HIP_CHECK(hipStreamSynchronize(st));
    for (int d = 0; d < NO; ++d)
        if (host[d]) HIP_CHECK(hipMemcpy(host[d], a.out[d], sizeof(double) * (size_t)s.n, hipMemcpyDeviceToHost));
}

// the positions (host[d], F::DIM entries, NULL skipped) and, if asked for, the blocked flags
template <class F>
void run_store(const F &f, const State &s, double *const *host, uint8_t *blocked, hipStream_t st) {
    for (int d = 0; d < F::DIM; ++d)
        if (host[d]) HIP_CHECK(hipMemcpy(host[d], s.c(d), sizeof(double) * (size_t)s.n, hipMemcpyDeviceToHost));
    if (!blocked) return;
    const DeviceStage stage((size_t)s.n);
    const FlagArgs<F> a{f, s.points<F::DIM>(), stage.as<uint8_t>()};
    hipLaunchKernelGGL(flag_tracers<F>, dim3(blocks_for(s.n)), dim3(BLOCK), 0, st, a);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipMemcpy(blocked, stage.get(), (size_t)s.n, hipMemcpyDeviceToHost));
}

// the *_ref entry points: positions must hold the invariant the kernels rely on
inline bool in_range(long long n, const double *c, int extent) {
    if (!c || extent < 1) return false;
    for (long long i = 0; i < n; ++i)
        if (!(c[i] >= 0.0 && c[i] < (double)extent)) return false;
    return true;
}

#undef LBM_HD

}  // namespace tracer
}  // namespace lbm
