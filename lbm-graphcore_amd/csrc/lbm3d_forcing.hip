// lbm3d_forcing.hip -- the forcing zones of the D3Q19 engine (the
// lbm3d_forcing_* functions of include/lbm_forcing_hip.h): the kernel that
// applies one zone to the lattice of one slab, the engine's host side, the
// extern "C" functions and the host-only restatement lbm3d_forcing_kick_ref.
//
// The kernel.  A streaming read-modify-write of the current flow lattice over
// the cells of the zone inside one slab: per cell the nineteen populations
// read (76 B), the eighteen moving ones written (72 B; f0 is read for the
// density and never written) and the obstacle byte, 149 B; the fields form
// reads seven coefficients more (177 B).  The block and grid of the buoyancy
// kick (scalar::slab_grid over the box; one wave along x, a block's waves on
// consecutive rows).  The launch covers the columns of the slab's quad grid
// around the zone's: a lane whose four cells all lie in the zone takes them
// with 16-B loads of the nineteen planes (and of the seven coefficient planes,
// which lie on the same grid: lbm_forcing.hpp) and 16-B stores of the eighteen
// moving planes; a quad the box's edge cuts and the ragged tail of a row go
// one cell at a time, and a box of fewer than four columns one cell per lane.
// A lane needs only its own cells and owns what it writes: no LDS, no atomics,
// no cross-lane move -- except, in the forms that return the impulse, the
// fixed-order fold of the block's fp64 sums (fold_block).  Ghost planes and
// pad columns are not touched.
//
// Arithmetic: IEEE fp32, as the header writes it, no contraction
// (-ffp-contract=off).

#include <hip/hip_runtime.h>

#include <algorithm>

#include "lbm3d_engine.hpp"
#include "lbm_forcing.hpp"
#include "lbm_forcing_hip.h"
#include "lbm_quad.hpp"

namespace lbm {
namespace forcing {

constexpr int WAVE = 64;  // lanes of a block along x: one wave (checked against scalar::slab_lanes_x at the launch)

// The view's box: the columns of the slab's quad grid around the zone's, the zone's rows and its planes inside the
// slab.  The zone's own columns are [lo, hi) of the box.
struct Force3 : Box3Edit {
    int lo, hi;
    float n;
    Coefs<NC3> c;
    double *sum_part;  // impulse forms: [3][blocks]
    float *max_part;   // unused maxima of the shared fold
};

namespace {

using scalar::KICK3_PAIRS;
using scalar::kick3_minus;
using scalar::kick3_plus;
using scalar::kick_pair;

// offset of the box's cell (x, y, z) inside a coefficient plane
__device__ __forceinline__ long long coef_at(const Force3 &a, int x, int y, int z) {
    return a.c.coff + ((long long)z * a.c.ch + y) * a.c.cp + x;
}

template <bool FIELDS, bool SUM>
__device__ __forceinline__ void force_one(const Force3 &a, int x, int y, int z, double (&s)[3]) {
    const int ax = a.x0 + x, ay = a.y0 + y, az = a.z0 + z;
    float *f = a.e + (long long)az * a.PL + (long long)ay * a.px + ax;
    float c[Q3];
    load_cell<Q3>(f, a.KS, 0, c);
    const bool blocked = a.obst[((long long)az * a.ny + ay) * a.nx + ax] != 0;
    float k[NC3];
#pragma unroll
    for (int j = 0; j < NC3; ++j) k[j] = FIELDS ? a.c.planes[j * a.c.cplane + coef_at(a, x, y, z)] : a.c.k[j];
    float inc[KICK3_PAIRS], m[3];
    const bool idle = force3(c, blocked, a.n, k, inc, m);
#pragma unroll
    for (int j = 0; j < KICK3_PAIRS; ++j) {
        float plus = c[kick3_plus(j)], minus = c[kick3_minus(j)];
        kick_pair(plus, minus, idle, inc[j]);
        f[kick3_plus(j) * a.KS] = plus;
        f[kick3_minus(j) * a.KS] = minus;
    }
    if (SUM) {
#pragma unroll
        for (int j = 0; j < 3; ++j) s[j] += idle ? 0.0 : (double)m[j];
    }
}

}  // namespace

template <bool FIELDS, bool SUM>
__global__ __launch_bounds__(BLOCK) void forcing_zone3d(Force3 a) {
    constexpr int ROWS = BLOCK / WAVE;
    const bool quad = a.quad != 0;
    const int cpl = quad ? 4 : 1;  // cells per lane
    const int tx = threadIdx.x & (WAVE - 1), ty = threadIdx.x / WAVE;
    const int x = (blockIdx.x * WAVE + tx) * cpl;
    const bool full = quad && x >= a.lo && x + 4 <= a.hi;
    const bool obst_word = (a.nx & 3) == 0;
    double s[3] = {0.0, 0.0, 0.0};
    if (x < a.bx) {
        for (int z = blockIdx.z; z < a.bz; z += gridDim.z) {
            for (int y = blockIdx.y * ROWS + ty; y < a.by; y += gridDim.y * ROWS) {
                if (full) {
                    const int ax = a.x0 + x, ay = a.y0 + y, az = a.z0 + z;
                    float *f = a.e + (long long)az * a.PL + (long long)ay * a.px + ax;
                    float4 v[Q3];
                    load_quad<Q3>(f, a.KS, v);
                    const unsigned bits = quad_map_bytes(a.obst + ((long long)az * a.ny + ay) * a.nx + ax, obst_word);
                    float4 kq[NC3];
                    if (FIELDS) load_quad<NC3, true>(a.c.planes + coef_at(a, x, y, z), a.c.cplane, kq);
                    float inc[4][KICK3_PAIRS];
                    bool idle[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float c[Q3];
                        quad_cell<Q3>(v, i, c);
                        float k[NC3];
#pragma unroll
                        for (int j = 0; j < NC3; ++j) k[j] = FIELDS ? pick(kq[j], i) : a.c.k[j];
                        float m[3];
                        idle[i] = force3(c, ((bits >> (8 * i)) & 0xffu) != 0, a.n, k, inc[i], m);
                        if (SUM) {
#pragma unroll
                            for (int j = 0; j < 3; ++j) s[j] += idle[i] ? 0.0 : (double)m[j];
                        }
                    }
#pragma unroll
                    for (int j = 0; j < KICK3_PAIRS; ++j) {
                        const float4 vp = v[kick3_plus(j)], vm = v[kick3_minus(j)];
                        float plus[4] = {vp.x, vp.y, vp.z, vp.w};
                        float minus[4] = {vm.x, vm.y, vm.z, vm.w};
#pragma unroll
                        for (int i = 0; i < 4; ++i) kick_pair(plus[i], minus[i], idle[i], inc[i][j]);
                        *reinterpret_cast<float4 *>(f + kick3_plus(j) * a.KS) =
                            make_float4(plus[0], plus[1], plus[2], plus[3]);
                        *reinterpret_cast<float4 *>(f + kick3_minus(j) * a.KS) =
                            make_float4(minus[0], minus[1], minus[2], minus[3]);
                    }
                } else {
                    // a quad the box's edge cuts, the ragged tail of a row, or one cell per lane
#pragma unroll 1
                    for (int i = 0; i < cpl; ++i)
                        if (x + i >= a.lo && x + i < a.hi) force_one<FIELDS, SUM>(a, x + i, y, z, s);
                }
            }
        }
    }
    if (SUM) {
        float m[1] = {0.f};
        const long long block = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        fold_block<ROWS>(s, m, block, (long long)gridDim.x * gridDim.y * gridDim.z, a.sum_part, a.max_part);
    }
}

namespace {

template <bool FIELDS>
void launch_zone(const Force3 &a, bool sum, dim3 grid, hipStream_t st) {
    if (sum)
        hipLaunchKernelGGL((forcing_zone3d<FIELDS, true>), grid, dim3(BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((forcing_zone3d<FIELDS, false>), grid, dim3(BLOCK), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

}  // namespace forcing
}  // namespace lbm

using namespace lbm;

// ---- D3Q19 engine: host side ----

void lbm3d_handle::forcing_set_zone(int zone, int x0, int y0, int z0, int w, int h, int d, const float *const *coef,
                                    const float *konst) {
    forcing::check_zone_index(zone);
    need_whole_domain("forcing zones");
    const bool keep = forcing::check_box(p.nx, p.ny, p.nz, x0, y0, z0, w, h, d);
    if (keep) forcing::check_coefs(forcing::NC3, (long long)w * h * d, coef, konst);
    if (!keep && !forcing) return;
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    if (!forcing) {
        forcing = new forcing::State;
        forcing->dev = slabs[0].dev;
    }
    if (keep)
        forcing::make_zone(forcing->z[zone], forcing::NC3, x0, y0, z0, w, h, d, coef, konst);
    else
        forcing::free_zone(forcing->z[zone]);
}

void lbm3d_handle::forcing_clear() { forcing::release(forcing); }

void lbm3d_handle::forcing_zones(int32_t *n_set, uint32_t *mask) const { forcing::zones_out(forcing, n_set, mask); }

// Zone after zone in index order, each on the current lattice of every slab it meets, then the ghost planes as
// after load_cells (refresh), exactly as after the buoyancy kick.
void lbm3d_handle::forcing_apply(float steps, double *impulse) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice for the forcing zones to act on");
    forcing::check_steps(steps);
    if (impulse) std::fill(impulse, impulse + 3 * forcing::MAX_ZONES, 0.0);
    if (steps == 0.f || !forcing::any_zone(forcing)) return;
    if (scalar::slab_lanes_x() != forcing::WAVE || scalar::slab_rows() * forcing::WAVE != forcing::BLOCK)
        throw lbm_failure(LBM_E_INTERNAL, "the forcing kernel's block is not the block slab_grid lays its grid for");
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    const hipStream_t st = slabs[0].s_comp;
    for (int i = 0; i < forcing::MAX_ZONES; ++i) {
        const forcing::Zone &z = forcing->z[i];
        if (!z.set) continue;
        double sum[3] = {0.0, 0.0, 0.0};
        float unused[1] = {0.f};
        const int qx0 = z.x0 & ~3, qx1 = std::min((z.x0 + z.w + 3) / 4 * 4, p.nx);
        for (const auto &s : slabs) {
            const int zlo = std::max(z.z0, s.z0), zhi = std::min(z.z0 + z.d, s.z0 + s.nzs);
            if (zlo >= zhi) continue;
            forcing::Force3 a{Box3Edit{box_view(s, qx0, z.y0, zlo - s.z0, qx1 - qx0, z.h, zhi - zlo), s.o[s.cur]}};
            a.lo = z.x0 - qx0;
            a.hi = a.lo + z.w;
            a.n = steps;
            for (int j = 0; j < forcing::NC3; ++j) a.c.k[j] = z.k[j];
            a.c.planes = z.dev;
            a.c.cplane = z.cplane;
            a.c.cp = z.cp;
            a.c.ch = z.h;
            a.c.coff = (long long)(zlo - z.z0) * z.h * z.cp;
            a.sum_part = nullptr;
            a.max_part = nullptr;
            const dim3 grid = scalar::slab_grid(a);
            const auto launch = [&] {
                if (z.dev)
                    forcing::launch_zone<true>(a, impulse != nullptr, grid, st);
                else
                    forcing::launch_zone<false>(a, impulse != nullptr, grid, st);
            };
            if (impulse) {
                const BlockPartials<3, 1> part((size_t)grid.x * grid.y * grid.z);
                a.sum_part = part.sums();
                a.max_part = part.maxima();
                launch();
                HIP_CHECK(hipStreamSynchronize(st));
                part.fold(sum, unused);
            } else {
                launch();
            }
        }
        if (impulse)
            for (int j = 0; j < 3; ++j) impulse[3 * i + j] = sum[j];
    }
    HIP_CHECK(hipStreamSynchronize(st));
    refresh();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm3d_forcing_set_zone(lbm3d_handle *h, int32_t zone, int32_t x0, int32_t y0, int32_t z0, int32_t w, int32_t ht,
                           int32_t d, const float *const coef[7], const float konst[7]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_set_zone(zone, x0, y0, z0, w, ht, d, coef, konst); });
}

int lbm3d_forcing_clear(lbm3d_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_clear(); });
}

int lbm3d_forcing_zones(lbm3d_handle *h, int32_t *n_set, uint32_t *mask) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_zones(n_set, mask); });
}

int lbm3d_forcing_apply(lbm3d_handle *h, float steps, double *impulse) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_apply(steps, impulse); });
}

int lbm3d_forcing_kick_ref(int32_t nx, int32_t ny, int32_t nz, const uint8_t *obst, float *cells, int32_t x0,
                           int32_t y0, int32_t z0, int32_t w, int32_t ht, int32_t d, const float *const coef[7],
                           const float konst[7], float steps, float *terms) {
    if (!forcing::ref_args_ok(forcing::NC3, nx, ny, nz, obst, cells, x0, y0, z0, w, ht, d, coef, konst, steps))
        return LBM_E_INVALID;
    if (terms) std::fill(terms, terms + (size_t)3 * w * ht * d, 0.f);
    if (steps == 0.f) return LBM_OK;
    for (int z = 0; z < d; ++z)
        for (int y = 0; y < ht; ++y)
            for (int x = 0; x < w; ++x) {
                const size_t r = ((size_t)z * ht + y) * w + x;
                const size_t i = ((size_t)(z0 + z) * ny + (y0 + y)) * nx + (x0 + x);
                float k[forcing::NC3];
                for (int j = 0; j < forcing::NC3; ++j) k[j] = forcing::ref_coef(coef, konst, j, r);
                float *c = cells + i * Q3;
                float cc[Q3];
                for (int j = 0; j < Q3; ++j) cc[j] = c[j];
                float inc[scalar::KICK3_PAIRS], m[3];
                const bool idle = forcing::force3(cc, obst[i] != 0, steps, k, inc, m);
                for (int j = 0; j < scalar::KICK3_PAIRS; ++j)
                    scalar::kick_pair(c[scalar::kick3_plus(j)], c[scalar::kick3_minus(j)], idle, inc[j]);
                if (terms && !idle)
                    for (int j = 0; j < 3; ++j) terms[3 * r + j] = m[j];
            }
    return LBM_OK;
}

}  // extern "C"
