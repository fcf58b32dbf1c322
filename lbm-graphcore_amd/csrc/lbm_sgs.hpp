// lbm_sgs.hpp -- the sub-grid model of both engines (lbm_sgs.hip,
// lbm3d_sgs.hip; include/lbm_sgs_hip.h): the per-cell arithmetic, compiled for
// the device and for the host from one text, the model a handle keeps and the
// host side both engines share (checking a model, laying its coefficient out
// on the device, releasing it).  The kernels, which edit the flow lattice
// through each engine's own view, are in the two .hip files.
//
// The coefficient plane.  A model whose coefficient is an array keeps rows x cp
// floats on the device, cp = roundup(nx, 4), rows = ny (ny * nz): the domain's
// own quad grid, as a forcing zone's planes (lbm_forcing.hpp), so that a lane
// whose four cells are one aligned quad of the lattice reads their
// coefficients with one 16-B load.  Cell (x, y, z) at plane[(z * ny + y) * cp
// + x]; the pad columns hold zeros and are never used.
//
// Arithmetic: IEEE fp32 in the order the header writes, no contraction
// (-ffp-contract=off), correctly rounded divide and sqrt (hipcc default).  rho
// and the velocities are written as cell_macro / cell3_macro write them, so
// they are lbm_store_fields' own.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "lbm3d_cell_macro.hpp"
#include "lbm_cell_macro.hpp"
#include "lbm_diag_host.hpp"
#include "lbm_scalar.hpp"
#include "lbm_sgs_hip.h"

namespace lbm {
namespace sgs {

#define LBM_HD __host__ __device__ __forceinline__

constexpr int BLOCK = scalar::BLOCK;     // lanes per block: the forcing zones' launch shape in both engines
constexpr float SMAG_K = 25.455844f;     // 18 sqrt 2

// ---- the per-cell arithmetic (host and device) ----

// what one application needs of the handle's omega and of n, formed once on the host in fp32
struct Model {
    int mode;
    float n, omega0, omo, aomo, tau0, nu0;
};

// the relaxation time the cell should have had
LBM_HD float tau_of(const Model &m, float coef, float pim, float rho) {
    if (m.mode == LBM_SGS_SMAGORINSKY) {
        const float a = (SMAG_K * m.n) * (coef * coef);
        return 0.5f * (m.tau0 + sqrtf((m.tau0 * m.tau0) + ((a * pim) / rho)));
    }
    const float nu1 = ((1.f / coef) - 0.5f) / 3.f;
    return (3.f * (m.nu0 + (m.n * (nu1 - m.nu0)))) + 0.5f;
}

// d and nu_add of a cell from |Pi| and rho; returns whether the cell is idle (then nothing else of it is used)
LBM_HD bool rate(const Model &m, float coef, bool blocked, float pim, float rho, float &d, float &nut) {
    const float tau = tau_of(m, coef, pim, rho);
    const float we = 1.f / tau;
    d = (m.omega0 - we) / m.omo;
    const bool off = m.mode == LBM_SGS_SMAGORINSKY ? coef == 0.f : coef == m.omega0;
    const bool idle = blocked || off || d == 0.f;
    nut = idle ? 0.f : (tau - m.tau0) / 3.f;
    return idle;
}

// the non-equilibrium parts of a pair of opposite speeds with the weight l and the velocity v along the first
LBM_HD void pair_neq(float l, float v, float csq, float cp, float cm, float &qp, float &qm) {
    qp = cp - (l * (((4.5f * v) * ((2.f / 3.f) + v)) + csq));
    qm = cm - (l * (((-4.5f * v) * ((2.f / 3.f) - v)) + csq));
}

// D2Q9.  q = c - feq(c); returns idle; d: the factor of q the cell gets; nut: nu_add (0.f when idle).
LBM_HD bool filter2(const float (&c)[9], bool blocked, const Model &m, float coef, float (&q)[9], float &d,
                    float &nut) {
    float rho = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) rho += c[k];
    float jx, jy;
    cell_momentum(c, jx, jy);
    const float ux = jx / rho, uy = jy / rho;
    const float usq = (ux * ux) + (uy * uy);
    const float csq = 1.f - (usq * 1.5f);
    const float l0 = (4.f / 9.f) * rho, l1 = rho / 9.f, l2 = rho / 36.f;
    q[0] = c[0] - (l0 * csq);
    pair_neq(l1, ux, csq, c[1], c[3], q[1], q[3]);
    pair_neq(l1, uy, csq, c[2], c[4], q[2], q[4]);
    pair_neq(l2, ux + uy, csq, c[5], c[7], q[5], q[7]);
    pair_neq(l2, (-ux) + uy, csq, c[6], c[8], q[6], q[8]);
    const float pxx = ((((q[1] + q[3]) + q[5]) + q[6]) + q[7]) + q[8];
    const float pyy = ((((q[2] + q[4]) + q[5]) + q[6]) + q[7]) + q[8];
    const float pxy = (q[5] + q[7]) - (q[6] + q[8]);
    const float p2 = ((pxx * pxx) + (pyy * pyy)) + ((pxy * pxy) * 2.f);
    return rate(m, coef, blocked, sqrtf(p2) / m.aomo, rho, d, nut);
}

// D3Q19
LBM_HD bool filter3(const float (&s)[19], bool blocked, const Model &m, float coef, float (&q)[19], float &d,
                    float &nut) {
    float rho = s[0];
#pragma unroll
    for (int k = 1; k < 19; ++k) rho += s[k];
    float jx, jy, jz;
    cell3_momentum(s, jx, jy, jz);
    const float ux = jx / rho, uy = jy / rho, uz = jz / rho;
    const float usq = ((ux * ux) + (uy * uy)) + (uz * uz);
    const float csq = 1.f - (usq * 1.5f);
    const float l0 = rho / 3.f, l1 = rho / 18.f, l2 = rho / 36.f;
    q[0] = s[0] - (l0 * csq);
    pair_neq(l1, ux, csq, s[1], s[2], q[1], q[2]);
    pair_neq(l1, uy, csq, s[3], s[4], q[3], q[4]);
    pair_neq(l2, ux + uy, csq, s[5], s[6], q[5], q[6]);
    pair_neq(l2, ux - uy, csq, s[7], s[8], q[7], q[8]);
    pair_neq(l1, uz, csq, s[9], s[14], q[9], q[14]);
    pair_neq(l2, ux + uz, csq, s[10], s[15], q[10], q[15]);
    pair_neq(l2, (-ux) + uz, csq, s[11], s[16], q[11], q[16]);
    pair_neq(l2, uy + uz, csq, s[12], s[17], q[12], q[17]);
    pair_neq(l2, (-uy) + uz, csq, s[13], s[18], q[13], q[18]);
    const float pxx = ((((((((q[1] + q[2]) + q[5]) + q[6]) + q[7]) + q[8]) + q[10]) + q[11]) + q[15]) + q[16];
    const float pyy = ((((((((q[3] + q[4]) + q[5]) + q[6]) + q[7]) + q[8]) + q[12]) + q[13]) + q[17]) + q[18];
    const float pzz = ((((((((q[9] + q[10]) + q[11]) + q[12]) + q[13]) + q[14]) + q[15]) + q[16]) + q[17]) + q[18];
    const float pxy = (q[5] + q[6]) - (q[7] + q[8]);
    const float pxz = (q[10] + q[15]) - (q[11] + q[16]);
    const float pyz = (q[12] + q[17]) - (q[13] + q[18]);
    const float p2 = (((pxx * pxx) + (pyy * pyy)) + (pzz * pzz)) +
                     ((((pxy * pxy) + (pxz * pxz)) + (pyz * pyz)) * 2.f);
    return rate(m, coef, blocked, sqrtf(p2) / m.aomo, rho, d, nut);
}

// the new value of one population: an idle cell keeps the loaded bits
LBM_HD float rescaled(float c, float q, float d, bool idle) { return idle ? c : c + (d * q); }

// per-lane statistics of an application: cells that were not idle, the sum and the maximum of their nu_add
struct Acc {
    double cells = 0.0, sum = 0.0;
    float max = 0.f;
    LBM_HD void add(bool idle, float nut) {
        cells += idle ? 0.0 : 1.0;
        sum += idle ? 0.0 : (double)nut;
        max = idle ? max : fmaxf(max, nut);
    }
};

// ---- the model of a handle ----

struct State {
    int dev = 0;
    int mode = LBM_SGS_OFF;
    float konst = 0.f;
    float *plane = nullptr;  // the coefficient plane; NULL: the constant
    int cp = 0;
    float cmin = 0.f, cmax = 0.f;  // the smallest and the largest coefficient: the range check of an application
};

// ---- host side both engines share ----

inline void check_steps(float steps) {
    if (!(std::isfinite(steps) && steps >= 0.f))
        throw lbm_failure(LBM_E_INVALID, "sub-grid model: steps must be finite and not negative");
}

inline void check_coef(int mode, float v) {
    if (!std::isfinite(v)) throw lbm_failure(LBM_E_INVALID, "sub-grid model: a coefficient is not finite");
    if (mode == LBM_SGS_SMAGORINSKY && v < 0.f)
        throw lbm_failure(LBM_E_INVALID, "sub-grid model: Cs must not be negative");
    if (mode == LBM_SGS_OMEGA && !(v > 0.f && v < 2.f))
        throw lbm_failure(LBM_E_INVALID, "sub-grid model: the rate lies in (0, 2)");
}

// mode (not OFF) and every coefficient; returns the smallest and the largest
inline void check_model(int mode, float konst, const float *coef, long long cells, float &cmin, float &cmax) {
    if (mode != LBM_SGS_SMAGORINSKY && mode != LBM_SGS_OMEGA)
        throw lbm_failure(LBM_E_INVALID, "sub-grid model: the mode is one of LBM_SGS_*");
    const float *a = coef ? coef : &konst;
    const long long n = coef ? cells : 1;
    cmin = cmax = a[0];
    for (long long i = 0; i < n; ++i) {
        check_coef(mode, a[i]);
        cmin = std::min(cmin, a[i]);
        cmax = std::max(cmax, a[i]);
    }
}

// what an application of n steps on a lattice collided with omega needs; refuses omega = 1 as lbm_store_stress does
inline Model make_model(int mode, float omega, float n) {
    Model m;
    m.mode = mode;
    m.n = n;
    m.omega0 = omega;
    (void)neq_strain_coef(omega);
    m.omo = 1.f - omega;
    m.aomo = fabsf(m.omo);
    m.tau0 = 1.f / omega;
    m.nu0 = (m.tau0 - 0.5f) / 3.f;
    return m;
}

// OMEGA: the rate every cell ends with lies in (0, 2).  tau_of is monotone in the coefficient (every operation of
// it is), so the smallest and the largest coefficient decide.
inline void check_rates(const Model &m, float cmin, float cmax) {
    if (m.mode != LBM_SGS_OMEGA) return;
    for (const float w1 : {cmin, cmax}) {
        const float we = 1.f / tau_of(m, w1, 0.f, 1.f);
        if (!(we > 0.f && we < 2.f))
            throw lbm_failure(LBM_E_INVALID,
                              "sub-grid model: " + std::to_string(m.n) + " steps towards the rate " +
                                  std::to_string(w1) + " end outside (0, 2)");
    }
}

inline void release(State *&s) {
    if (!s) return;
    if (hipSetDevice(s->dev) == hipSuccess) (void)hipFree(s->plane);
    delete s;
    s = nullptr;
}

// The checked model on the device `dev` (current); throws before anything of `out` changes.  coef: rows x nx.
inline void make_state(State *&out, int dev, int mode, float konst, const float *coef, int nx, long long rows,
                       float cmin, float cmax) {
    State z;
    z.dev = dev;
    z.mode = mode;
    z.konst = konst;
    z.cmin = cmin;
    z.cmax = cmax;
    if (coef) {
        z.cp = (nx + 3) / 4 * 4;
        std::vector<float> host((size_t)rows * z.cp, 0.f);
        for (long long r = 0; r < rows; ++r) std::copy(coef + r * nx, coef + (r + 1) * nx, host.data() + r * z.cp);
        if (hipMalloc((void **)&z.plane, sizeof(float) * host.size()) != hipSuccess) {
            (void)hipGetLastError();
            throw lbm_failure(LBM_E_NOMEM, "no device memory for the sub-grid model's coefficients");
        }
        const hipError_t e = hipMemcpy(z.plane, host.data(), sizeof(float) * host.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(z.plane);
            HIP_CHECK(e);
        }
    }
    if (!out) out = new State;
    (void)hipFree(out->plane);
    *out = z;
}

// the arguments of the *_filter_ref entry points; false: LBM_E_INVALID.  Fills the model.
inline bool ref_args_ok(int nx, int ny, int nz, const void *obst, const void *cells, float omega, int mode,
                        float konst, const float *coef, float steps, Model &m) {
    if (nx < 1 || ny < 1 || nz < 1 || !obst || !cells) return false;
    if (!(std::isfinite(omega) && omega > 0.f && omega < 2.f)) return false;
    try {
        float cmin, cmax;
        check_model(mode, konst, coef, (long long)nx * ny * nz, cmin, cmax);
        check_steps(steps);
        m = make_model(mode, omega, steps);
        if (steps != 0.f) check_rates(m, cmin, cmax);
    } catch (const lbm_failure &) {
        return false;
    }
    return true;
}

#undef LBM_HD

}  // namespace sgs
}  // namespace lbm
