// lbm3d_forces.hip -- the D3Q19 instantiation of the wall-list kernels
// (lbm_forces.hpp) behind lbm3d_wall_force, lbm3d_store_wall_force and
// lbm3d_body_forces (include/lbm_forces_hip.h); their host side is in
// lbm3d.hip, the wall list in lbm_forces.hip.
//
// A wall cell's force comes from its own 18 moving populations (what the
// bounce-back of the last step stored there), each loaded only where its link
// bit is set; the list's offsets are relative to plane z = 0 of the slab, so
// the ghost planes and either lattice of the pair need no special case.
// IEEE fp32 in the written order, no contraction: the per-cell values equal
// lio.wall_force_cells3d of the stored cells bit for bit.

#include "lbm_forces.hpp"

namespace lbm {
namespace forces {

namespace {

struct D3Q19 {
    static __device__ __forceinline__ void force(const float *p, long long ks, unsigned m, float &fx, float &fy,
                                                 float &fz) {
        float t[19];
#pragma unroll
        for (int j = 1; j < 19; ++j) t[j] = ((m >> (j - 1)) & 1u) ? p[j * ks] : 0.f;
        fx = ((t[2] + t[6] + t[8] + t[11] + t[15]) - (t[1] + t[5] + t[7] + t[10] + t[16])) * 2.f;
        fy = ((t[4] + t[6] + t[7] + t[13] + t[17]) - (t[3] + t[5] + t[8] + t[12] + t[18])) * 2.f;
        fz = ((t[14] + t[15] + t[16] + t[17] + t[18]) - (t[9] + t[10] + t[11] + t[12] + t[13])) * 2.f;
    }
};

}  // namespace

hipError_t launch_wall3d(const WallArgs &a, int kind, hipStream_t s) { return launch_wall<D3Q19>(a, kind, s); }

}  // namespace forces
}  // namespace lbm
