// lbm_cell_macro.hpp -- the per-cell macroscopic expressions of the D2Q9
// lattice, shared by the kernels that derive them: macroscopic_fields
// (lbm_fields.hip) and accumulate_moments (lbm_averages.hip).  One definition,
// so what the averages accumulate is what lbm_store_fields gives, bit for bit.
//
// Arithmetic: IEEE fp32, evaluation order of lbmhost::macroscopic
// (host/lbm_host.hpp), no contraction (-ffp-contract=off), correctly rounded
// divide and sqrt.
#pragma once

#include <hip/hip_runtime.h>

namespace lbm {

struct CellMacro {
    float ux, uy, u, pressure;
};

// the momentum (rho u_x, rho u_y): the numerators cell_macro divides by rho
__host__ __device__ __forceinline__ void cell_momentum(const float (&c)[9], float &jx, float &jy) {
    jx = c[1] + c[5] + c[8] - (c[3] + c[6] + c[7]);
    jy = c[2] + c[5] + c[6] - (c[4] + c[7] + c[8]);
}

// need_v: u_x / u_y wanted (two divides); need_u: |u| wanted (sqrt); rho is always formed
template <bool NEED_V, bool NEED_U>
__device__ __forceinline__ CellMacro cell_macro(const float (&c)[9], bool blocked, float obst_pressure, float &rho) {
    rho = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) rho += c[k];
    CellMacro m{0.f, 0.f, 0.f, obst_pressure};
    if (blocked) return m;
    if (NEED_V) {
        float jx, jy;
        cell_momentum(c, jx, jy);
        m.ux = jx / rho;
        m.uy = jy / rho;
    }
    if (NEED_U) m.u = sqrtf((m.ux * m.ux) + (m.uy * m.uy));
    m.pressure = rho * (1.f / 3.f);
    return m;
}

}  // namespace lbm
