// lbm_views.hpp -- the views the diagnostics' kernel argument blocks address a
// lattice through: LatticeView (D2Q9, one sub-domain) and Box3View (D3Q19, a
// box of one slab).  FieldsArgs, GradArgs, StressArgs, Bin2Args and
// Fields3Args, Grad3Args, Stress3Args, Bin3Args derive from them; the handles
// fill them in one place (lattice_view, box_view).  Plain data, no device code.
#pragma once

#include <cstdint>

namespace lbm {

// The current D2Q9 lattice of one sub-domain: cell (x, y), speed k at
// o[k * plane + y * pitch + x], either layout.
struct LatticeView {
    const float *o;         // lattice origin (current side of the pair)
    const uint8_t *obst;    // uint8[h][w]
    long long plane;
    int pitch, w, h;
    int sp;                 // staging row pitch: roundup(w, 4)
    float obst_pressure;    // pressure reported for an obstacle cell: density * (1/3)
};

// The bx x by x bz cells at (x0, y0, z0) of one D3Q19 slab's current lattice:
// cell (x, y, z), speed k at o[k * KS + z * PL + y * px + x].  quad (x0 % 4 == 0
// and bx >= 4 required): four cells per lane with 16-B accesses, staging rows
// of sp = roundup(bx, 4) floats; else one cell per lane, sp = bx.
struct Box3View {
    const float *o;        // lattice origin: plane z = 0 of the slab
    const uint8_t *obst;   // uint8[nzs][ny][nx] of the slab
    long long PL, KS;      // plane stride, speed stride (floats)
    int px, nx, ny;        // row pitch (floats) and extents of a lattice plane
    int x0, y0, z0;        // box origin (z0 slab-local)
    int bx, by, bz;        // box extents (> 0, inside the slab)
    int quad;              // access path, see above
    int sp;                // staging row pitch (floats)
    float obst_pressure;   // pressure reported for an obstacle cell: density * (1/3)
};

// The writable counterparts, for the one kind of kernel that changes the
// current lattice in place between runs (the buoyancy kick of lbm_scalar.hip /
// lbm3d_scalar.hip, the forcing zones of lbm_forcing.hip / lbm3d_forcing.hip):
// `e` is the same origin as `o`, writable, and such a kernel
// reads and writes through it alone.  Owned cells only: the ghost cells are
// left to the engine (lbm_handle::lattice_edit, lbm3d_handle::slab_edit).
struct LatticeEdit : LatticeView {
    float *e;
};

struct Box3Edit : Box3View {
    float *e;
};

}  // namespace lbm
