// lbm_forcing.hip -- the forcing zones of the D2Q9 engine (the lbm_forcing_*
// functions of include/lbm_forcing_hip.h): the kernel that applies one zone to
// the lattice of one sub-domain, the engine's host side, the extern "C"
// functions and the host-only restatement lbm_forcing_kick_ref.
//
// The kernel.  A streaming read-modify-write of the current flow lattice over
// the cells of the zone inside one sub-domain, memory-bound: per cell the nine
// populations read (36 B), the eight moving ones written (32 B; f0 is read for
// the density and never written) and the obstacle byte, 69 B; the fields form
// reads five coefficients more (89 B).  The buoyancy kick's shape: one lane
// takes four consecutive cells of a row on the sub-domain's quad grid, 16-B
// loads of the nine planes (and the five coefficient planes, which lie on the
// same grid: lbm_forcing.hpp), 16-B stores of the eight moving planes, the
// obstacle bytes through quad_map_bytes.  A quad the box's edge cuts, the
// ragged tail of a row and sub-domains whose x origin is no multiple of 4 go
// one cell at a time.  A lane needs only its own cells and owns what it
// writes: no LDS, no atomics, no cross-lane move, no race in place -- except,
// in the forms that return the impulse, the fixed-order fold of the block's
// fp64 sums (fold_block).  Ghost cells and pad columns are not touched.
//
// Four compiled forms: coefficients as kernel arguments (uniform) or from the
// planes (fields), each with and without the impulse sums.
//
// Arithmetic: IEEE fp32, as the header writes it, no contraction
// (-ffp-contract=off).

#include <hip/hip_runtime.h>

#include "lbm_engine.hpp"
#include "lbm_forcing.hpp"
#include "lbm_forcing_hip.h"
#include "lbm_quad.hpp"

namespace lbm {
namespace forcing {

// One sub-domain's lattice, writable, and the zone's cells inside it, [lx0, lx1) x [ly0, ly1) in the sub-domain's
// own coordinates; the launch's quads start at column qx0.
struct Force2 : LatticeEdit {
    int lx0, lx1, ly0, ly1;
    int qx0;
    int quad;  // the sub-domain's x origin is a multiple of 4: the 16-B path
    float n;
    Coefs<NC2> c;
    double *sum_part;  // impulse forms: [2][blocks]
    float *max_part;   // unused maxima of the shared fold
};

namespace {

using scalar::KICK2_PAIRS;
using scalar::kick2_minus;
using scalar::kick2_plus;
using scalar::kick_pair;

template <bool FIELDS, bool SUM>
__device__ __forceinline__ void force_one(const Force2 &a, int x, int y, double (&s)[2]) {
    float *f = a.e + (long long)y * a.pitch + x;
    float c[Q];
    load_cell<Q>(f, a.plane, 0, c);
    const bool blocked = a.obst[(long long)y * a.w + x] != 0;
    float k[NC2];
#pragma unroll
    for (int j = 0; j < NC2; ++j)
        k[j] = FIELDS ? a.c.planes[j * a.c.cplane + (a.c.coff + (long long)y * a.c.cp + x)] : a.c.k[j];
    float inc[KICK2_PAIRS], m[2];
    const bool idle = force2(c, blocked, a.n, k, inc, m);
#pragma unroll
    for (int j = 0; j < KICK2_PAIRS; ++j) {
        float plus = c[kick2_plus(j)], minus = c[kick2_minus(j)];
        kick_pair(plus, minus, idle, inc[j]);
        f[kick2_plus(j) * a.plane] = plus;
        f[kick2_minus(j) * a.plane] = minus;
    }
    if (SUM) {
        s[0] += idle ? 0.0 : (double)m[0];
        s[1] += idle ? 0.0 : (double)m[1];
    }
}

}  // namespace

template <bool FIELDS, bool SUM>
__global__ __launch_bounds__(BLOCK) void forcing_zone(Force2 a) {
    const int qpr = (a.lx1 - a.qx0 + 3) >> 2;  // lanes' quads per row
    const long long total = (long long)qpr * (a.ly1 - a.ly0);
    const bool obst_word = (a.w & 3) == 0;
    double s[2] = {0.0, 0.0};
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < total; q += (long long)gridDim.x * BLOCK) {
        const int r = (int)(q / qpr);
        const int y = a.ly0 + r;
        const int x = a.qx0 + ((int)(q - (long long)r * qpr) << 2);
        if (a.quad && x >= a.lx0 && x + 4 <= a.lx1) {
            float *f = a.e + (long long)y * a.pitch + x;
            float4 v[Q];
            load_quad<Q>(f, a.plane, v);
            const unsigned bits = quad_map_bytes(a.obst + (long long)y * a.w + x, obst_word);
            float4 kq[NC2];
            if (FIELDS) load_quad<NC2>(a.c.planes + (a.c.coff + (long long)y * a.c.cp + x), a.c.cplane, kq);
            float o[Q][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float c[Q];
                quad_cell<Q>(v, i, c);
                float k[NC2];
#pragma unroll
                for (int j = 0; j < NC2; ++j) k[j] = FIELDS ? pick(kq[j], i) : a.c.k[j];
                float inc[KICK2_PAIRS], m[2];
                const bool idle = force2(c, ((bits >> (8 * i)) & 0xffu) != 0, a.n, k, inc, m);
#pragma unroll
                for (int j = 0; j < KICK2_PAIRS; ++j) {
                    float plus = c[kick2_plus(j)], minus = c[kick2_minus(j)];
                    kick_pair(plus, minus, idle, inc[j]);
                    o[kick2_plus(j)][i] = plus;
                    o[kick2_minus(j)][i] = minus;
                }
                if (SUM) {
                    s[0] += idle ? 0.0 : (double)m[0];
                    s[1] += idle ? 0.0 : (double)m[1];
                }
            }
#pragma unroll
            for (int k = 1; k < Q; ++k)  // the rest speed is read and never written
                *reinterpret_cast<float4 *>(f + k * a.plane) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
        } else {
            // a quad the box's edge cuts, the ragged tail of a row, or a sub-domain off the alignment
            for (int i = 0; i < 4; ++i)
                if (x + i >= a.lx0 && x + i < a.lx1) force_one<FIELDS, SUM>(a, x + i, y, s);
        }
    }
    if (SUM) {
        float m[1] = {0.f};
        fold_block<BLOCK / 64>(s, m, blockIdx.x, gridDim.x, a.sum_part, a.max_part);
    }
}

namespace {

template <bool FIELDS>
void launch_zone(const Force2 &a, bool sum, int nb, hipStream_t st) {
    if (sum)
        hipLaunchKernelGGL((forcing_zone<FIELDS, true>), dim3(nb), dim3(BLOCK), 0, st, a);
    else
        hipLaunchKernelGGL((forcing_zone<FIELDS, false>), dim3(nb), dim3(BLOCK), 0, st, a);
    HIP_CHECK(hipGetLastError());
}

}  // namespace

}  // namespace forcing
}  // namespace lbm

// ---- D2Q9 engine: host side ----

void lbm_handle::forcing_set_zone(int zone, int x0, int y0, int w, int h, const float *const *coef,
                                  const float *konst) {
    forcing::check_zone_index(zone);
    need_whole_domain("forcing zones");
    const bool keep = forcing::check_box(p.nx, p.ny, 1, x0, y0, 0, w, h, 1);
    if (keep) forcing::check_coefs(forcing::NC2, (long long)w * h, coef, konst);
    if (!keep && !forcing) return;
    sync_all();
    set_device(subs[0]);
    if (!forcing) {
        forcing = new forcing::State;
        forcing->dev = subs[0].dev;
    }
    if (keep)
        forcing::make_zone(forcing->z[zone], forcing::NC2, x0, y0, 0, w, h, 1, coef, konst);
    else
        forcing::free_zone(forcing->z[zone]);
}

void lbm_handle::forcing_clear() { forcing::release(forcing); }

void lbm_handle::forcing_zones(int32_t *n_set, uint32_t *mask) const { forcing::zones_out(forcing, n_set, mask); }

// Zone after zone in index order, each on the current lattice of every sub-domain it meets.  The ghost ring is
// left to the next run, which rebuilds it first (ring_stale), exactly as after the buoyancy kick.
void lbm_handle::forcing_apply(float steps, double *impulse) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice for the forcing zones to act on");
    forcing::check_steps(steps);
    if (impulse) std::fill(impulse, impulse + 2 * forcing::MAX_ZONES, 0.0);
    if (steps == 0.f || !forcing::any_zone(forcing)) return;
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    for (int i = 0; i < forcing::MAX_ZONES; ++i) {
        const forcing::Zone &z = forcing->z[i];
        if (!z.set) continue;
        double sum[2] = {0.0, 0.0};
        float unused[1] = {0.f};
        for (const auto &s : subs) {
            forcing::Force2 a{lattice_edit(s)};
            a.lx0 = std::max(z.x0, s.rect.x0) - s.rect.x0;
            a.lx1 = std::min(z.x0 + z.w, s.rect.x0 + s.w) - s.rect.x0;
            a.ly0 = std::max(z.y0, s.rect.y0) - s.rect.y0;
            a.ly1 = std::min(z.y0 + z.h, s.rect.y0 + s.h) - s.rect.y0;
            if (a.lx0 >= a.lx1 || a.ly0 >= a.ly1) continue;
            a.quad = s.rect.x0 % 4 == 0 ? 1 : 0;
            a.qx0 = a.quad ? a.lx0 & ~3 : a.lx0;
            a.n = steps;
            for (int j = 0; j < forcing::NC2; ++j) a.c.k[j] = z.k[j];
            a.c.planes = z.dev;
            a.c.cplane = z.cplane;
            a.c.cp = z.cp;
            a.c.ch = z.h;
            a.c.coff = (long long)(s.rect.y0 - z.y0) * z.cp + (s.rect.x0 - z.cx0);
            a.sum_part = nullptr;
            a.max_part = nullptr;
            const int nb = fields_blocks((a.lx1 - a.qx0 + 3) / 4 * 4, a.ly1 - a.ly0);
            const auto launch = [&] {
                if (z.dev)
                    forcing::launch_zone<true>(a, impulse != nullptr, nb, s0.s_comp);
                else
                    forcing::launch_zone<false>(a, impulse != nullptr, nb, s0.s_comp);
            };
            if (impulse) {
                const BlockPartials<2, 1> part((size_t)nb);
                a.sum_part = part.sums();
                a.max_part = part.maxima();
                timed(s0, s0.s_comp, "forcing", launch);
                ring_stale = true;
                HIP_CHECK(hipStreamSynchronize(s0.s_comp));
                part.fold(sum, unused);
            } else {
                timed(s0, s0.s_comp, "forcing", launch);
                ring_stale = true;
            }
        }
        if (impulse) {
            impulse[2 * i] = sum[0];
            impulse[2 * i + 1] = sum[1];
        }
    }
    HIP_CHECK(hipStreamSynchronize(s0.s_comp));
    prof_collect();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm_forcing_set_zone(lbm_handle *h, int32_t zone, int32_t x0, int32_t y0, int32_t w, int32_t ht,
                         const float *const coef[5], const float konst[5]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_set_zone(zone, x0, y0, w, ht, coef, konst); });
}

int lbm_forcing_clear(lbm_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_clear(); });
}

int lbm_forcing_zones(lbm_handle *h, int32_t *n_set, uint32_t *mask) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_zones(n_set, mask); });
}

int lbm_forcing_apply(lbm_handle *h, float steps, double *impulse) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->forcing_apply(steps, impulse); });
}

int lbm_forcing_kick_ref(int32_t nx, int32_t ny, const uint8_t *obst, float *cells, int32_t x0, int32_t y0, int32_t w,
                         int32_t ht, const float *const coef[5], const float konst[5], float steps, float *terms) {
    if (!forcing::ref_args_ok(forcing::NC2, nx, ny, 1, obst, cells, x0, y0, 0, w, ht, 1, coef, konst, steps))
        return LBM_E_INVALID;
    if (terms) std::fill(terms, terms + (size_t)2 * w * ht, 0.f);
    if (steps == 0.f) return LBM_OK;
    for (int y = 0; y < ht; ++y)
        for (int x = 0; x < w; ++x) {
            const size_t r = (size_t)y * w + x, i = (size_t)(y0 + y) * nx + (x0 + x);
            float k[forcing::NC2];
            for (int j = 0; j < forcing::NC2; ++j) k[j] = forcing::ref_coef(coef, konst, j, r);
            float *c = cells + i * Q;
            float cc[Q];
            for (int j = 0; j < Q; ++j) cc[j] = c[j];
            float inc[scalar::KICK2_PAIRS], m[2];
            const bool idle = forcing::force2(cc, obst[i] != 0, steps, k, inc, m);
            for (int j = 0; j < scalar::KICK2_PAIRS; ++j)
                scalar::kick_pair(c[scalar::kick2_plus(j)], c[scalar::kick2_minus(j)], idle, inc[j]);
            if (terms && !idle) {
                terms[2 * r] = m[0];
                terms[2 * r + 1] = m[1];
            }
        }
    return LBM_OK;
}

}  // extern "C"
