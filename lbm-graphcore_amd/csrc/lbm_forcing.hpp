// lbm_forcing.hpp -- the forcing zones of both engines (lbm_forcing.hip,
// lbm3d_forcing.hip; include/lbm_forcing_hip.h): the per-cell arithmetic,
// compiled for the device and for the host from one text, the zones a handle
// keeps and the host side both engines share (checking a zone's coefficients,
// laying them out on the device, releasing them).  The kernels, which edit
// the flow lattice through each engine's own view, are in the two .hip files.
//
// Coefficient planes.  A zone whose coefficients are not all constants keeps
// NC planes (5 or 7; a constant beside an array is materialised) of d x h
// rows of cp floats on the device, covering the columns cx0 = x0 & ~3 to
// roundup(x0 + w, 4) of the domain: the domain's own quad grid, so that a lane
// whose four cells are one aligned quad of the lattice reads each coefficient
// of them with one 16-B load.  Cell (x, y, z) of the domain, coefficient i at
// dev[i * cplane + ((z - z0) * h + (y - y0)) * cp + (x - cx0)]; the pad columns
// hold zeros and are never used.
//
// Index safety: set_zone checks the box against the domain on the host, and
// every launch covers the intersection of a checked box with one part.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "lbm3d_cell_macro.hpp"
#include "lbm_cell_macro.hpp"
#include "lbm_diag_host.hpp"
#include "lbm_forcing_hip.h"
#include "lbm_quad.hpp"
#include "lbm_scalar.hpp"

namespace lbm {
namespace forcing {

#define LBM_HD __host__ __device__ __forceinline__

constexpr int MAX_ZONES = LBM_FORCING_MAX_ZONES;
constexpr int BLOCK = scalar::BLOCK;  // lanes per block: the buoyancy kick's launch shape in both engines
constexpr int NC2 = 5, NC3 = 7;       // coefficients per cell: lam, ut, f

// ---- the per-cell arithmetic (host and device) ----

// m = l (rho ut - j) + rho g of one component
LBM_HD float pull(float l, float rho, float ut, float j, float g) { return (l * ((rho * ut) - j)) + (rho * g); }

// D2Q9, k = lam, utx, uty, fx, fy.  Forms the momentum (m) the zone adds to the cell and its four pair increments;
// returns whether the cell is idle (then nothing of it is used: kick_pair selects the loaded value).
LBM_HD bool force2(const float (&c)[9], bool blocked, float n, const float (&k)[NC2],
                   float (&inc)[scalar::KICK2_PAIRS], float (&m)[2]) {
    const float l = fminf(n * k[0], 1.f), gx = n * k[3], gy = n * k[4];
    float rho = c[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) rho += c[i];
    float jx, jy;
    cell_momentum(c, jx, jy);
    m[0] = pull(l, rho, k[1], jx, gx);
    m[1] = pull(l, rho, k[2], jy, gy);
    scalar::kick2_pairs(m[0], m[1], inc);
    return blocked || (l == 0.f && gx == 0.f && gy == 0.f);
}

// D3Q19, k = lam, utx, uty, utz, fx, fy, fz
LBM_HD bool force3(const float (&s)[19], bool blocked, float n, const float (&k)[NC3],
                   float (&inc)[scalar::KICK3_PAIRS], float (&m)[3]) {
    const float l = fminf(n * k[0], 1.f), gx = n * k[4], gy = n * k[5], gz = n * k[6];
    float rho = s[0];
#pragma unroll
    for (int i = 1; i < 19; ++i) rho += s[i];
    float jx, jy, jz;
    cell3_momentum(s, jx, jy, jz);
    m[0] = pull(l, rho, k[1], jx, gx);
    m[1] = pull(l, rho, k[2], jy, gy);
    m[2] = pull(l, rho, k[3], jz, gz);
    scalar::kick3_pairs(m[0], m[1], m[2], inc);
    return blocked || (l == 0.f && gx == 0.f && gy == 0.f && gz == 0.f);
}

// ---- what a kernel's argument block says about the coefficients ----

// The constants (uniform form), or the planes (fields form): the coefficient i of the cell (x, y, z) of the
// launch's own coordinates is planes[i * cplane + coff + (z * ch + y) * cp + x].
template <int NC>
struct Coefs {
    float k[NC];
    const float *planes;
    long long cplane, coff;
    int cp, ch;
};

// ---- the zones of a handle ----

struct Zone {
    bool set = false;
    int x0 = 0, y0 = 0, z0 = 0, w = 0, h = 0, d = 0;
    float k[NC3] = {};      // the constants (uniform form)
    float *dev = nullptr;   // the planes (fields form); NULL: uniform
    int cx0 = 0, cp = 0;
    long long cplane = 0;
};

struct State {
    int dev = 0;
    Zone z[MAX_ZONES];
};

// ---- host side both engines share ----

inline void check_steps(float steps) {
    if (!(std::isfinite(steps) && steps >= 0.f))
        throw lbm_failure(LBM_E_INVALID, "forcing: steps must be finite and not negative");
}

// nc coefficients over `cells` cells: coef[i] (coef itself may be NULL) an array of that many, or konst[i]
inline void check_coefs(int nc, long long cells, const float *const *coef, const float *konst) {
    if (!konst) throw lbm_failure(LBM_E_INVALID, "forcing: NULL constants");
    for (int i = 0; i < nc; ++i) {
        const float *a = coef ? coef[i] : nullptr;
        const long long n = a ? cells : 1;
        if (!a) a = konst + i;
        for (long long j = 0; j < n; ++j) {
            if (!std::isfinite(a[j]))
                throw lbm_failure(LBM_E_INVALID, "forcing: coefficient " + std::to_string(i) + " is not finite");
            if (i == 0 && a[j] < 0.f) throw lbm_failure(LBM_E_INVALID, "forcing: lam must not be negative");
        }
    }
}

inline void check_zone_index(int zone) {
    if (zone < 0 || zone >= MAX_ZONES)
        throw lbm_failure(LBM_E_INVALID, "forcing: the zone index lies in 0 .. " + std::to_string(MAX_ZONES - 1));
}

// a box of a domain nx x ny x nz; false: an empty one (the zone is removed)
inline bool check_box(int nx, int ny, int nz, int x0, int y0, int z0, int w, int h, int d) {
    if (w < 0 || h < 0 || d < 0) throw lbm_failure(LBM_E_INVALID, "forcing: negative extent of the zone's box");
    if (w == 0 || h == 0 || d == 0) return false;
    if (x0 < 0 || y0 < 0 || z0 < 0 || (long long)x0 + w > nx || (long long)y0 + h > ny || (long long)z0 + d > nz)
        throw lbm_failure(LBM_E_INVALID, "forcing: the zone's box leaves the domain");
    return true;
}

inline void free_zone(Zone &z) {
    (void)hipFree(z.dev);
    z = Zone{};
}

inline void release(State *&s) {
    if (!s) return;
    if (hipSetDevice(s->dev) == hipSuccess)
        for (Zone &z : s->z) free_zone(z);
    delete s;
    s = nullptr;
}

// The checked zone (box and coefficients are valid) on the current device; throws before anything of `out` changes.
inline void make_zone(Zone &out, int nc, int x0, int y0, int z0, int w, int h, int d, const float *const *coef,
                      const float *konst) {
    Zone z;
    z.set = true;
    z.x0 = x0, z.y0 = y0, z.z0 = z0, z.w = w, z.h = h, z.d = d;
    bool fields = false;
    for (int i = 0; i < nc; ++i) {
        z.k[i] = konst[i];
        fields = fields || (coef && coef[i]);
    }
    if (fields) {
        z.cx0 = x0 & ~3;
        z.cp = (x0 + w + 3) / 4 * 4 - z.cx0;
        z.cplane = (long long)d * h * z.cp;
        std::vector<float> host((size_t)nc * (size_t)z.cplane, 0.f);
        const size_t rows = (size_t)d * h;
        for (int i = 0; i < nc; ++i)
            for (size_t r = 0; r < rows; ++r) {
                float *dst = host.data() + (size_t)i * z.cplane + r * z.cp + (x0 - z.cx0);
                for (int x = 0; x < w; ++x) dst[x] = coef[i] ? coef[i][r * w + x] : konst[i];
            }
        if (hipMalloc((void **)&z.dev, sizeof(float) * host.size()) != hipSuccess) {
            (void)hipGetLastError();
            throw lbm_failure(LBM_E_NOMEM, "no device memory for the zone's coefficients");
        }
        const hipError_t e = hipMemcpy(z.dev, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(z.dev);
            HIP_CHECK(e);
        }
    }
    (void)hipFree(out.dev);
    out = z;
}

inline void zones_out(const State *s, int32_t *n_set, uint32_t *mask) {
    int n = 0;
    uint32_t m = 0;
    for (int i = 0; s && i < MAX_ZONES; ++i)
        if (s->z[i].set) {
            ++n;
            m |= 1u << i;
        }
    if (n_set) *n_set = n;
    if (mask) *mask = m;
}

inline bool any_zone(const State *s) {
    for (int i = 0; s && i < MAX_ZONES; ++i)
        if (s->z[i].set) return true;
    return false;
}

// the arguments of the *_kick_ref entry points; false: LBM_E_INVALID
inline bool ref_args_ok(int nc, int nx, int ny, int nz, const void *obst, const void *cells, int x0, int y0, int z0,
                        int w, int h, int d, const float *const *coef, const float *konst, float steps) {
    if (nx < 1 || ny < 1 || nz < 1 || !obst || !cells || !konst) return false;
    try {
        if (!check_box(nx, ny, nz, x0, y0, z0, w, h, d)) return false;
        check_coefs(nc, (long long)w * h * d, coef, konst);
        check_steps(steps);
    } catch (const lbm_failure &) {
        return false;
    }
    return true;
}

// coefficient i of cell r (row-major in the box) for the *_kick_ref entry points
inline float ref_coef(const float *const *coef, const float *konst, int i, size_t r) {
    return coef && coef[i] ? coef[i][r] : konst[i];
}

#undef LBM_HD

}  // namespace forcing
}  // namespace lbm
