// lbm3d_cell_macro.hpp -- the per-cell macroscopic expressions of the D3Q19
// lattice, shared by the kernels that derive them: macroscopic_fields3d
// (lbm3d_fields.hip) and accumulate_moments (lbm3d_averages.hip).  One
// definition, so what the averages accumulate is what lbm3d_store_fields
// gives, bit for bit.
//
// Arithmetic: IEEE fp32, the expressions and order of oracle/lbm_oracle3d.c
// cell3d, no contraction (-ffp-contract=off), correctly rounded divide and sqrt.
#pragma once

#include <hip/hip_runtime.h>

namespace lbm {

struct Cell3Macro {
    float ux, uy, uz, u, pressure;
};

// the momentum (rho u_x, rho u_y, rho u_z): the numerators cell3_macro divides by rho
__host__ __device__ __forceinline__ void cell3_momentum(const float (&s)[19], float &jx, float &jy, float &jz) {
    jx = (s[1] + s[5] + s[7] + s[10] + s[16]) - (s[2] + s[6] + s[8] + s[11] + s[15]);
    jy = (s[3] + s[5] + s[8] + s[12] + s[18]) - (s[4] + s[6] + s[7] + s[13] + s[17]);
    jz = (s[9] + s[10] + s[11] + s[12] + s[13]) - (s[14] + s[15] + s[16] + s[17] + s[18]);
}

// NEED_V: a velocity component or |u| wanted (three divides); NEED_U: |u| wanted (sqrt); rho is always formed
template <bool NEED_V, bool NEED_U>
__device__ __forceinline__ Cell3Macro cell3_macro(const float (&s)[19], bool blocked, float obst_pressure,
                                                  float &rho) {
    rho = s[0];
#pragma unroll
    for (int k = 1; k < 19; ++k) rho += s[k];
    Cell3Macro m{0.f, 0.f, 0.f, 0.f, obst_pressure};
    if (blocked) return m;
    if (NEED_V) {
        float jx, jy, jz;
        cell3_momentum(s, jx, jy, jz);
        m.ux = jx / rho;
        m.uy = jy / rho;
        m.uz = jz / rho;
    }
    if (NEED_U) m.u = sqrtf(m.ux * m.ux + m.uy * m.uy + m.uz * m.uz);
    m.pressure = rho * (1.f / 3.f);
    return m;
}

}  // namespace lbm
