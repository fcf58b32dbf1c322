// lbm3d_fields.hpp -- argument block and launcher of the D3Q19 macroscopic
// fields kernel (lbm3d_fields.hip), part of the engine's declaration (lbm3d_engine.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "lbm_views.hpp"

namespace lbm {

// Fields of the view's box (lbm_views.hpp) into the planar staging arrays
// float[bz][by][sp]; a null array is neither computed nor stored.
struct Fields3Args : Box3View {
    float *ux, *uy, *uz, *speed, *pressure;
    double *mass_part;     // stats launch: per-block fp64 sums of the cells' densities
    float *umax_part;      // stats launch: per-block max |u| over fluid cells
};

// blocks of a launch over a.bx x a.by x a.bz: also the partials a stats launch writes
int fields3d_blocks(const Fields3Args &a);
// stats = false: the requested fields; stats = true: the per-block partials
// (mass_part / umax_part hold fields3d_blocks(a) entries each)
hipError_t launch_macroscopic_fields3d(const Fields3Args &a, bool stats, hipStream_t s);

}  // namespace lbm
