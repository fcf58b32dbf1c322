// lbm_scalar.hip -- the passive scalar of the D2Q9 engine (the lbm_scalar_*
// functions of include/lbm_scalar_hip.h and lbm_thermal_hip.h): the D2Q5 step
// kernel over the lattice of one sub-domain, the buoyancy kick on that
// lattice, the engine's host side, the extern "C" functions and the host-only
// restatements lbm_scalar_step_ref and lbm_scalar_buoyancy_ref.
//
// The step kernel.  Memory-bound: per cell it must move 36 B of flow
// populations, the obstacle byte, 20 B of scalar populations read and 20 B
// written, no reuse beyond a row's neighbours, no LDS, no atomics.  One lane
// takes four consecutive cells of a row: the nine flow populations and the
// obstacle word by the access path of lbm_quad.hpp, the rest, N and S scalar
// planes by one 16-B load each (the scalar rows are padded to 4 floats and the
// sub-domain starts at a multiple of 4, so the quads of both lattices
// coincide).  The E and W planes are wanted one cell off the alignment: the
// lane loads its own aligned quad of each and takes the one missing value from
// the neighbouring lane by a cross-lane move; the lanes at the ends of a wave
// or of a row load that cell directly (the periodic image at the ends of the
// domain).  Five 16-B stores.  The last w % 4 cells of a row, and sub-domains
// that start off the alignment, go one cell at a time.  Only rho and the two
// velocity components are formed (cell_macro<true, false>: two divides, no
// sqrt).
//
// One launch per local sub-domain reads the flow through that sub-domain's
// LatticeView and the scalar at global coordinates with periodic wrap, all on
// the compute stream of the first sub-domain after a synchronisation of every
// stream: no ghost cell of either lattice exists or is read.
//
// Arithmetic: IEEE fp32, as the header writes it, no contraction
// (-ffp-contract=off), correctly rounded divide.

#include <hip/hip_runtime.h>

#include "lbm_cell_macro.hpp"
#include "lbm_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_scalar.hpp"
#include "lbm_scalar_hip.h"

namespace lbm {
namespace scalar {

// one sub-domain's flow lattice, where its cell (0, 0) lies in the domain, and the two scalar sets
struct Step2 : LatticeView {
    const float *gin;
    float *gout;
    long long gplane;
    int gsp, gx0, gy0, nx, ny;
    int quad;  // gx0 % 4 == 0: the 16-B path
    float omega;
};

namespace {

// cell (x, y) of the sub-domain, every value loaded on its own
__device__ __forceinline__ void step_one(const Step2 &a, int x, int y) {
    float c[Q];
    load_cell<Q>(a.o + (long long)y * a.pitch, a.plane, x, c);
    const bool blocked = a.obst[(long long)y * a.w + x] != 0;
    float rho;
    const CellMacro m = cell_macro<true, false>(c, blocked, a.obst_pressure, rho);
    const int gx = a.gx0 + x, gy = a.gy0 + y;
    const long long row = (long long)gy * a.gsp;
    const float p[5] = {a.gin[row + gx], a.gin[a.gplane + row + below(gx, a.nx)],
                        a.gin[2 * a.gplane + (long long)below(gy, a.ny) * a.gsp + gx],
                        a.gin[3 * a.gplane + row + above(gx, a.nx)],
                        a.gin[4 * a.gplane + (long long)above(gy, a.ny) * a.gsp + gx]};
    float out[5];
    cell2(p, blocked, m.ux, m.uy, a.omega, out);
#pragma unroll
    for (int k = 0; k < 5; ++k) a.gout[k * a.gplane + row + gx] = out[k];
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void scalar_step(Step2 a) {
    const int qpr = (a.w + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * a.h;
    const bool obst_word = (a.w & 3) == 0;
    const int lane = threadIdx.x & 63;
    // the trip count is the same for every lane of a block: the cross-lane moves below run converged
    for (long long base = (long long)blockIdx.x * BLOCK; base < total; base += (long long)gridDim.x * BLOCK) {
        const long long q = base + threadIdx.x;
        const bool active = q < total;
        const int y = active ? (int)(q / qpr) : 0;
        const int x = active ? (int)(q - (long long)y * qpr) << 2 : 0;
        const bool full = active && a.quad && x + 4 <= a.w;
        const int gx = a.gx0 + x, gy = a.gy0 + y;
        const float *row = a.gin + (long long)gy * a.gsp;
        float4 g1 = make_float4(0.f, 0.f, 0.f, 0.f), g3 = g1;
        if (full) {
            g1 = *reinterpret_cast<const float4 *>(row + a.gplane + gx);
            g3 = *reinterpret_cast<const float4 *>(row + 3 * a.gplane + gx);
        }
        // lane - 1 holds the quad to the west, lane + 1 the quad to the east, when they lie in this row
        const float west = __shfl_up(g1.w, 1, 64);
        const float east = __shfl_down(g3.x, 1, 64);
        if (full) {
            const float pw = (lane != 0 && x >= 4) ? west : row[a.gplane + below(gx, a.nx)];
            const float pe = (lane != 63 && x + 8 <= a.w) ? east : row[3 * a.gplane + (gx + 4 == a.nx ? 0 : gx + 4)];
            const float4 g0 = *reinterpret_cast<const float4 *>(row + gx);
            const float4 g2 =
                *reinterpret_cast<const float4 *>(a.gin + 2 * a.gplane + (long long)below(gy, a.ny) * a.gsp + gx);
            const float4 g4 =
                *reinterpret_cast<const float4 *>(a.gin + 4 * a.gplane + (long long)above(gy, a.ny) * a.gsp + gx);
            float4 v[Q];
            load_quad<Q>(a.o + (long long)y * a.pitch + x, a.plane, v);
            const unsigned bits = quad_map_bytes(a.obst + (long long)y * a.w + x, obst_word);
            const float4 p1 = make_float4(pw, g1.x, g1.y, g1.z);
            const float4 p3 = make_float4(g3.y, g3.z, g3.w, pe);
            float o[5][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q];
                quad_cell<Q>(v, i, c);
                const bool blocked = ((bits >> (8 * i)) & 0xffu) != 0;
                float rho;
                // as a fluid cell, whatever the map says: an obstacle cell's velocity is never used, and a
                // branch on the map here lets the compiler sink the flow loads into it, 4 B at a time
                const CellMacro m = cell_macro<true, false>(c, false, a.obst_pressure, rho);
                const float p[5] = {pick(g0, i), pick(p1, i), pick(g2, i), pick(p3, i), pick(g4, i)};
                float out[5];
                cell2(p, blocked, m.ux, m.uy, a.omega, out);
#pragma unroll
                for (int k = 0; k < 5; ++k) o[k][i] = out[k];
            }
            float *dst = a.gout + (long long)gy * a.gsp + gx;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                *reinterpret_cast<float4 *>(dst + k * a.gplane) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
        } else if (active) {
            // the ragged tail of a row, or a sub-domain off the alignment: one cell at a time
            for (int i = 0; i < 4 && x + i < a.w; ++i) step_one(a, x + i, y);
        }
    }
}

// ---- the buoyancy kick (include/lbm_thermal_hip.h) ----
//
// A streaming read-modify-write of the current flow lattice: per cell 20 B of
// scalar populations and the obstacle byte read, the eight moving flow planes
// read and written (85 B; f0 is not touched).  The scalar step's shape: four
// consecutive cells per lane, 16-B loads and stores on both lattices, the
// ragged tail and sub-domains off the alignment one cell at a time.  A lane
// needs only its own cells and owns what it writes: no LDS, no atomics, no
// cross-lane move, no race in place.  Ghost cells and pad columns are not
// touched.

// one sub-domain's flow lattice, writable, where its cell (0, 0) lies in the domain, and the current scalar set
struct Kick2 : LatticeEdit {
    const float *g;
    long long gplane;
    int gsp, gx0, gy0;
    int quad;  // gx0 % 4 == 0: the 16-B path
    float kx, ky, phi_ref;
};

namespace {

__device__ __forceinline__ void kick_one(const Kick2 &a, int x, int y) {
    const long long at = (long long)(a.gy0 + y) * a.gsp + (a.gx0 + x);
    float g[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) g[k] = a.g[k * a.gplane + at];
    const bool blocked = a.obst[(long long)y * a.w + x] != 0;
    float inc[KICK2_PAIRS];
    kick2_inc(cell_phi<5>(g), a.phi_ref, a.kx, a.ky, inc);
    float *f = a.e + (long long)y * a.pitch + x;
#pragma unroll
    for (int j = 0; j < KICK2_PAIRS; ++j) {
        float *fp = f + kick2_plus(j) * a.plane, *fm = f + kick2_minus(j) * a.plane;
        float plus = *fp, minus = *fm;
        kick_pair(plus, minus, blocked, inc[j]);
        *fp = plus;
        *fm = minus;
    }
}

}  // namespace

__global__ __launch_bounds__(BLOCK) void scalar_buoyancy(Kick2 a) {
    const int qpr = (a.w + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * a.h;
    const bool obst_word = (a.w & 3) == 0;
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * BLOCK) {
        const int y = (int)(q / qpr);
        const int x = (int)(q - (long long)y * qpr) << 2;
        if (a.quad && x + 4 <= a.w) {
            float4 gq[5];
            load_quad<5>(a.g + (long long)(a.gy0 + y) * a.gsp + (a.gx0 + x), a.gplane, gq);
            const unsigned bits = quad_map_bytes(a.obst + (long long)y * a.w + x, obst_word);
            float *f = a.e + (long long)y * a.pitch + x;
            float4 v[Q];  // v[0] stays unused: the rest speed is neither loaded nor stored
#pragma unroll
            for (int k = 1; k < Q; ++k) v[k] = *reinterpret_cast<const float4 *>(f + k * a.plane);
            float o[Q][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float g[5] = {pick(gq[0], i), pick(gq[1], i), pick(gq[2], i), pick(gq[3], i), pick(gq[4], i)};
                const bool blocked = ((bits >> (8 * i)) & 0xffu) != 0;
                float inc[KICK2_PAIRS];
                kick2_inc(cell_phi<5>(g), a.phi_ref, a.kx, a.ky, inc);
#pragma unroll
                for (int j = 0; j < KICK2_PAIRS; ++j) {
                    float plus = pick(v[kick2_plus(j)], i), minus = pick(v[kick2_minus(j)], i);
                    kick_pair(plus, minus, blocked, inc[j]);
                    o[kick2_plus(j)][i] = plus;
                    o[kick2_minus(j)][i] = minus;
                }
            }
#pragma unroll
            for (int k = 1; k < Q; ++k)
                *reinterpret_cast<float4 *>(f + k * a.plane) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
        } else {
            // the ragged tail of a row, or a sub-domain off the alignment: one cell at a time
            for (int i = 0; i < 4 && x + i < a.w; ++i) kick_one(a, x + i, y);
        }
    }
}

}  // namespace scalar
}  // namespace lbm

namespace {

scalar::State &scalar_state(lbm_handle &h) {
    if (!h.scalars) throw lbm_failure(LBM_E_STATE, "no scalar: call lbm_scalar_begin first");
    return *h.scalars;
}

scalar::Region region_of(const Sub &s) { return scalar::Region{s.obst, s.rect.x0, s.rect.y0, 0, s.w, s.h, 1}; }

}  // namespace

// ---- D2Q9 engine: host side ----

// What a feature that keeps one global array beside the lattice asks of the handle (the scalar; the forcing zones
// of lbm_forcing.hip): one device, the whole domain here, at most 16 local parts, no RCCL world > 1.
void lbm_handle::need_whole_domain(const char *what) const {
    const std::string w(what);
    if (transport == LBM_TRANSPORT_RCCL && world > 1)
        throw lbm_failure(LBM_E_INVALID, w + " on RCCL handles of more than one rank are not built");
    if ((int)subs.size() > scalar::MAX_PARTS)
        throw lbm_failure(LBM_E_INVALID, w + " on more than 16 local sub-domains are not built");
    long long cells = 0;
    for (const auto &s : subs) {
        if (s.dev != subs[0].dev)
            throw lbm_failure(LBM_E_INVALID, w + " on sub-domains of more than one device are not built");
        cells += (long long)s.w * s.h;
    }
    if (subs.empty() || cells != (long long)p.nx * p.ny)
        throw lbm_failure(LBM_E_INVALID, w + " need every sub-domain of the domain on this handle");
}

void lbm_handle::scalar_begin(float omega_s, const float *phi0) {
    need_whole_domain("scalars");
    scalar::check_omega(omega_s);
    sync_all();
    scalar::begin(scalars, subs[0].dev, 5, p.nx, p.ny, 1, omega_s, phi0);
}

void lbm_handle::scalar_set_fixed(int64_t n, const int32_t *x, const int32_t *y, const float *value) {
    scalar::State &t = scalar_state(*this);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    scalar::set_fixed<5>(t, n, x, y, nullptr, false, value, s0.s_comp,
                         [&](auto &&launch) { timed(s0, s0.s_comp, "scalar_fixed", launch); });
    prof_collect();
}

void lbm_handle::scalar_advance(int steps) {
    scalar::State &t = scalar_state(*this);
    if (steps < 0) throw lbm_failure(LBM_E_INVALID, "steps must not be negative");
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to advance the scalar over");
    if (steps == 0) return;
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    for (int n = 0; n < steps; ++n) {
        for (const auto &s : subs) {
            scalar::Step2 a{lattice_view(s)};
            a.gin = t.g[t.cur];
            a.gout = t.g[t.cur ^ 1];
            a.gplane = t.grid.plane;
            a.gsp = t.grid.sp;
            a.gx0 = s.rect.x0;
            a.gy0 = s.rect.y0;
            a.nx = p.nx;
            a.ny = p.ny;
            a.quad = s.rect.x0 % 4 == 0 ? 1 : 0;
            a.omega = t.omega;
            timed(s0, s0.s_comp, "scalar_step", [&] {
                hipLaunchKernelGGL(scalar::scalar_step, dim3(fields_blocks(s.w, s.h)), dim3(BLOCK), 0, s0.s_comp, a);
                HIP_CHECK(hipGetLastError());
            });
        }
        t.cur ^= 1;
        ++t.steps;
        if (scalar::walls_listed(t))  // the wall models (include/lbm_scalar_walls_hip.h), before the fixed list
            timed(s0, s0.s_comp, "scalar_walls", [&] { HIP_CHECK(scalar::walls_pass2d(t, t.g[t.cur], s0.s_comp)); });
        scalar::apply_fixed<5>(t, t.g[t.cur], s0.s_comp,
                               [&](auto &&launch) { timed(s0, s0.s_comp, "scalar_fixed", launch); });
    }
    HIP_CHECK(hipStreamSynchronize(s0.s_comp));
    prof_collect();
}

int64_t lbm_handle::scalar_steps() { return scalar_state(*this).steps; }

void lbm_handle::scalar_store(float *phi, float *g) {
    scalar::State &t = scalar_state(*this);
    if (!phi && !g) return;
    sync_all();
    scalar::store<5>(t, phi, g, subs[0].s_comp);
}

void lbm_handle::scalar_stats(double *total, float *min, float *max) {
    scalar::State &t = scalar_state(*this);
    if (!total && !min && !max) return;
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    double sum[1] = {0.0};
    float m[2] = {-INFINITY, -INFINITY};
    for (const auto &s : subs)
        scalar::stats_region<5>(t, region_of(s), s0.s_comp, sum, m,
                                [&](auto &&launch) { timed(s0, s0.s_comp, "scalar_stats", launch); });
    prof_collect();
    scalar::stats_out(sum, m, total, min, max);
}

void lbm_handle::scalar_end() { scalar::end(scalars); }

// The kick on the current lattice of every sub-domain.  The ghost ring is left to the next run, which rebuilds
// it first (ring_stale), as it does after a run that ended on a remainder launch; the resident kernel keeps none,
// the pipeline rebuilds its own every step, and no diagnostic reads a ghost cell.
void lbm_handle::scalar_buoyancy(float sx, float sy, float phi_ref) {
    scalar::State &t = scalar_state(*this);
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice for the scalar to act on");
    if (!(std::isfinite(sx) && std::isfinite(sy) && std::isfinite(phi_ref)))
        throw lbm_failure(LBM_E_INVALID, "the impulse and phi_ref must be finite");
    if (sx == 0.f && sy == 0.f) return;
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    for (const auto &s : subs) {
        scalar::Kick2 a{lattice_edit(s)};
        a.g = t.g[t.cur];
        a.gplane = t.grid.plane;
        a.gsp = t.grid.sp;
        a.gx0 = s.rect.x0;
        a.gy0 = s.rect.y0;
        a.quad = s.rect.x0 % 4 == 0 ? 1 : 0;
        a.kx = p.density * sx;
        a.ky = p.density * sy;
        a.phi_ref = phi_ref;
        timed(s0, s0.s_comp, "scalar_buoyancy", [&] {
            hipLaunchKernelGGL(scalar::scalar_buoyancy, dim3(fields_blocks(s.w, s.h)), dim3(BLOCK), 0, s0.s_comp, a);
            HIP_CHECK(hipGetLastError());
        });
    }
    ring_stale = true;
    HIP_CHECK(hipStreamSynchronize(s0.s_comp));
    prof_collect();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm_scalar_begin(lbm_handle *h, float omega_s, const float *phi0) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_begin(omega_s, phi0); });
}

int lbm_scalar_set_fixed(lbm_handle *h, int64_t n, const int32_t *x, const int32_t *y, const float *value) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_set_fixed(n, x, y, value); });
}

int lbm_scalar_advance(lbm_handle *h, int32_t steps) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_advance(steps); });
}

int lbm_scalar_steps(lbm_handle *h, int64_t *n) {
    if (!h || !n) return LBM_E_INVALID;
    return guarded(h, [&] { *n = h->scalar_steps(); });
}

int lbm_scalar_store(lbm_handle *h, float *phi, float *g) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_store(phi, g); });
}

int lbm_scalar_stats(lbm_handle *h, double *total, float *min, float *max) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_stats(total, min, max); });
}

int lbm_scalar_end(lbm_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_end(); });
}

int lbm_scalar_step_ref(int32_t nx, int32_t ny, float omega_s, const float *ux, const float *uy, const uint8_t *obst,
                        const float *g_in, float *g_out) {
    if (!scalar::ref_args_ok(nx, ny, 1, omega_s, {ux, uy, obst, g_in, g_out})) return LBM_E_INVALID;
    const size_t plane = (size_t)nx * ny;
    for (int y = 0; y < ny; ++y)
        for (int x = 0; x < nx; ++x) {
            const size_t row = (size_t)y * nx, i = row + x;
            const float p[5] = {g_in[i], g_in[plane + row + scalar::below(x, nx)],
                                g_in[2 * plane + (size_t)scalar::below(y, ny) * nx + x],
                                g_in[3 * plane + row + scalar::above(x, nx)],
                                g_in[4 * plane + (size_t)scalar::above(y, ny) * nx + x]};
            float out[5];
            scalar::cell2(p, obst[i] != 0, ux[i], uy[i], omega_s, out);
            for (int k = 0; k < 5; ++k) g_out[k * plane + i] = out[k];
        }
    return LBM_OK;
}

int lbm_scalar_buoyancy(lbm_handle *h, float sx, float sy, float phi_ref) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_buoyancy(sx, sy, phi_ref); });
}

int lbm_scalar_buoyancy_ref(int32_t nx, int32_t ny, float density, float sx, float sy, float phi_ref,
                            const uint8_t *obst, const float *g, float *cells) {
    if (!scalar::kick_args_ok(nx, ny, 1, {density, sx, sy, phi_ref}, {obst, g, cells})) return LBM_E_INVALID;
    if (sx == 0.f && sy == 0.f) return LBM_OK;
    const float kx = density * sx, ky = density * sy;
    const size_t plane = (size_t)nx * ny;
    for (size_t i = 0; i < plane; ++i) {
        const float gc[5] = {g[i], g[plane + i], g[2 * plane + i], g[3 * plane + i], g[4 * plane + i]};
        float inc[scalar::KICK2_PAIRS];
        scalar::kick2_inc(scalar::cell_phi<5>(gc), phi_ref, kx, ky, inc);
        float *c = cells + i * Q;
        for (int j = 0; j < scalar::KICK2_PAIRS; ++j)
            scalar::kick_pair(c[scalar::kick2_plus(j)], c[scalar::kick2_minus(j)], obst[i] != 0, inc[j]);
    }
    return LBM_OK;
}

}  // extern "C"
