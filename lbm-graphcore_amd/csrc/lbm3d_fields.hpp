// lbm3d_fields.hpp -- argument block and launcher of the D3Q19 macroscopic
// fields kernel (lbm3d_fields.hip), part of the engine's declaration (lbm3d_engine.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace lbm {

// Fields of the bx x by x bz cells at (x0, y0, z0) of one slab's current
// lattice into the planar staging arrays float[bz][by][sp]; a null array is
// neither computed nor stored.  quad (x0 % 4 == 0 and bx >= 4 required): four
// cells per lane with 16-B accesses, sp = roundup(bx, 4); else one cell per
// lane, sp = bx.
struct Fields3Args {
    const float *o;        // lattice origin: plane z = 0 of the slab
    const uint8_t *obst;   // uint8[nzs][ny][nx] of the slab
    long long PL, KS;      // plane stride, speed stride (floats)
    int px, nx, ny;        // row pitch (floats) and extents of a lattice plane
    int x0, y0, z0;        // box origin (z0 slab-local)
    int bx, by, bz;        // box extents (> 0, inside the slab)
    int quad;              // access path, see above
    int sp;                // staging row pitch (floats)
    float obst_pressure;   // pressure reported for an obstacle cell: density * (1/3)
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
