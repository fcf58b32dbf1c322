// lbm_transport.hpp -- what the scalar transport sums of both engines share
// (lbm_transport.hip, lbm3d_transport.hip; include/lbm_transport_hip.h): the
// per-cell terms, compiled for the device and for the host from one text, and
// the checks of the host-only restatements.  The geometry of bins, waves and
// chunks, the fold along x and the second pass are those of the flow's binned
// sums (lbm_binned.hpp).
//
// Term order (LBM_SBIN_* / LBM3D_SBIN_*), D = 2 or 3 axes:
//     0 PHI, 1 PHIPHI, 2 .. 1 + D  U?PHI, 2 + D .. 1 + 2 D  F?
// The kernels' no-flow form keeps PHI, PHIPHI and the D faces only (noflow_field).
#pragma once

#include <hip/hip_runtime.h>

#include <initializer_list>

#include "lbm_scalar.hpp"

namespace lbm {
namespace transport {

#define LBM_HD __host__ __device__ __forceinline__

constexpr int SB_FIELDS2 = 6, SB_FIELDS3 = 8;      // LBM_SBIN_FIELDS, LBM3D_SBIN_FIELDS
constexpr int SB_NOFLOW2 = 4, SB_NOFLOW3 = 5;      // sums of the no-flow form

// speed of the scalar lattice that leaves a cell along +axis (D2Q5: E, N; D3Q7: +x, +y, +z); the speed the
// neighbour on that side sends back is scalar::cell2 / cell3's opp of it (D2Q5: 3, 4; D3Q7: 2, 4, 6)
template <int D>
LBM_HD int plus_speed(int axis) {
    return D == 2 ? 1 + axis : 1 + 2 * axis;
}
template <int D>
LBM_HD int minus_speed(int axis) {
    return D == 2 ? 3 + axis : 2 + 2 * axis;
}

// What crosses the face on the high side of a cell in the next scalar step: the population the cell sends
// across less the one its neighbour sends back.  One fp32 subtraction of stored values.
LBM_HD float face_flux(float out_of_cell, float back_from_neighbour) { return out_of_cell - back_from_neighbour; }

// The terms of one cell into t (order above, 2 + 2 D entries): g its own stored populations, back[c] the
// minus-speed population of its neighbour on the high side of axis c, u its velocity as the engine's
// store_fields gives it.  The fluid terms of an obstacle cell are +0.0 by a select, never a branch (a branch on
// the map lets the compiler sink the flow loads behind the velocity into it); a sum that starts from +0.0 is
// not changed by them.
template <int D>
LBM_HD void cell_terms(const float (&g)[2 * D + 1], const float (&back)[D], bool blocked, const float (&u)[D],
                       double (&t)[2 + 2 * D]) {
    const double phi = (double)scalar::cell_phi<2 * D + 1>(g);
    t[0] = blocked ? 0.0 : phi;
    t[1] = blocked ? 0.0 : phi * phi;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        t[2 + c] = blocked ? 0.0 : (double)u[c] * phi;
        t[2 + D + c] = (double)face_flux(g[plus_speed<D>(c)], back[c]);
    }
}

// the same without the velocity terms (order PHI, PHIPHI, F?): what the kernels' no-flow form adds
template <int D>
LBM_HD void cell_terms_noflow(const float (&g)[2 * D + 1], const float (&back)[D], bool blocked, double (&t)[2 + D]) {
    const double phi = (double)scalar::cell_phi<2 * D + 1>(g);
    t[0] = blocked ? 0.0 : phi;
    t[1] = blocked ? 0.0 : phi * phi;
#pragma unroll
    for (int c = 0; c < D; ++c) t[2 + c] = (double)face_flux(g[plus_speed<D>(c)], back[c]);
}

// field index (LBM_SBIN_* / LBM3D_SBIN_*) of sum j of the no-flow form
template <int D>
LBM_HD int noflow_field(int j) {
    return j < 2 ? j : j + D;
}

#undef LBM_HD

// bits of the request: which groups of fields a call wants
template <int D>
struct Wanted {
    bool flow = false, phi = false, face[D] = {};
    int count = 0;
    explicit Wanted(double *const *out) {
        for (int f = 0; out && f < 2 + 2 * D; ++f) {
            if (!out[f]) continue;
            ++count;
            if (f < 2) phi = true;
            else if (f < 2 + D) flow = true;
            else face[f - 2 - D] = true;
        }
    }
};

// the *_terms_ref entry points
inline bool ref_args_ok(int nx, int ny, int nz, std::initializer_list<const void *> arrays) {
    if (nx < 1 || ny < 1 || nz < 1) return false;
    for (const void *p : arrays)
        if (!p) return false;
    return true;
}

}  // namespace transport
}  // namespace lbm
