// lbm3d_stress.hip -- strain rate and wall shear of the D3Q19 engine from the
// non-equilibrium second moment of each cell's own populations (the lbm3d_*
// functions of include/lbm_stress_hip.h).  The kernel, then the engine's host
// side.
//
// Cell-local, so every transport and world size works.  One memory-bound pass
// over the 19 populations of the current lattice: 77 B read per cell, 4 B
// written per requested field, no LDS but the statistics' fold.  The access
// paths are macroscopic_fields3d's (Box3View::quad, lbm_quad.hpp): four
// consecutive cells of a row per lane with a float4 store per field into
// staging rows padded to 4 floats, or one cell per lane.  A
// block is 64 lanes along x by S3Y rows and walks S3Z consecutive planes;
// offsets are formed in 64 bits.
//
// The statistics read a class map (CLS_*) in place of the obstacle map, built
// on the host from the slab's ghosted map at the first statistics call.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "lbm3d_engine.hpp"
#include "lbm_quad.hpp"
#include "lbm_stress.hpp"
#include "lbm_stress_hip.h"

namespace lbm {
namespace stress {

namespace {

struct Acc {
    double sum_s2 = 0.0, sum_wall = 0.0;
    float max_s = 0.f, max_wall = 0.f;
};

template <bool STATS>
__device__ __forceinline__ Strain3 cell(const float (&c)[Q3], unsigned cls, float coef, Acc &acc) {
    const bool blocked = STATS ? cls == CLS_BLOCKED : cls != 0;
    const Strain3 s = neq_strain3(c, blocked, coef);
    if (STATS && !blocked) {
        acc.sum_s2 += (double)s.s2;
        acc.max_s = fmaxf(acc.max_s, s.strain);
        if (cls == CLS_NEAR_WALL) {
            acc.sum_wall += (double)s.strain;
            acc.max_wall = fmaxf(acc.max_wall, s.strain);
        }
    }
    return s;
}

}  // namespace

// STATS: no field is stored and a.obst is the class map; block b (x fastest,
// then y, then z) writes its partial sums and maxima (fold_block, lbm_quad.hpp).
template <bool STATS>
__global__ __launch_bounds__(S3X *S3Y) void neq_strain3d(Stress3Args a) {
    const bool quad = a.quad != 0;
    const int cpl = quad ? 4 : 1;  // cells per lane
    const int tx = threadIdx.x & (S3X - 1), ty = threadIdx.x / S3X;
    const int x = (blockIdx.x * S3X + tx) * cpl;  // box-local
    const bool obst_word = (a.nx & 3) == 0;  // every quad's four map bytes are one aligned word
    Acc acc;
    if (x < a.bx) {
        const int zend = min((int)(blockIdx.z + 1) * S3Z, a.bz);
        for (int z = blockIdx.z * S3Z; z < zend; ++z) {
            for (int y = blockIdx.y * S3Y + ty; y < a.by; y += gridDim.y * S3Y) {
                const long long lz = a.z0 + z, ly = a.y0 + y;
                const float *src = a.o + lz * a.PL + ly * a.px + (a.x0 + x);
                const uint8_t *ob = a.obst + (lz * a.ny + ly) * a.nx + (a.x0 + x);
                const long long so = ((long long)z * a.by + y) * a.sp + x;
                if (quad && x + 4 <= a.bx) {
                    float4 v[Q3];
                    load_quad<Q3>(src, a.KS, v);
                    const unsigned bits = quad_map_bytes(ob, obst_word);
                    Strain3 s[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float c[Q3];
                        quad_cell<Q3>(v, i, c);
                        s[i] = cell<STATS>(c, (bits >> (8 * i)) & 0xffu, a.coef, acc);
                    }
                    if (!STATS) {
#define LBM_ST3_STORE(I, F) \
    if (a.out[I]) *reinterpret_cast<float4 *>(a.out[I] + so) = make_float4(s[0].F, s[1].F, s[2].F, s[3].F)
                        LBM_ST3_STORE(0, sxx);
                        LBM_ST3_STORE(1, syy);
                        LBM_ST3_STORE(2, szz);
                        LBM_ST3_STORE(3, sxy);
                        LBM_ST3_STORE(4, sxz);
                        LBM_ST3_STORE(5, syz);
                        LBM_ST3_STORE(6, strain);
#undef LBM_ST3_STORE
                    }
                } else {
                    // one cell per lane, or the ragged tail of a row: its last bx % 4 cells, one at a time
                    for (int i = 0; i < cpl && x + i < a.bx; ++i) {
                        float c[Q3];
                        load_cell<Q3>(src, a.KS, i, c);
                        const Strain3 s = cell<STATS>(c, ob[i], a.coef, acc);
                        if (!STATS) {
                            if (a.out[0]) a.out[0][so + i] = s.sxx;
                            if (a.out[1]) a.out[1][so + i] = s.syy;
                            if (a.out[2]) a.out[2][so + i] = s.szz;
                            if (a.out[3]) a.out[3][so + i] = s.sxy;
                            if (a.out[4]) a.out[4][so + i] = s.sxz;
                            if (a.out[5]) a.out[5][so + i] = s.syz;
                            if (a.out[6]) a.out[6][so + i] = s.strain;
                        }
                    }
                }
            }
        }
    }
    if (STATS) {
        double s[2] = {acc.sum_s2, acc.sum_wall};
        float m[2] = {acc.max_s, acc.max_wall};
        const long long b = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
        fold_block<S3Y>(s, m, b, (long long)gridDim.x * gridDim.y * gridDim.z, a.sum_part, a.max_part);
    }
}

namespace {

dim3 stress3d_grid(const Stress3Args &a) {
    const int cpl = a.quad ? 4 : 1;
    const long long lanes = ((long long)a.bx + cpl - 1) / cpl;
    const long long gx = (lanes + S3X - 1) / S3X;
    const long long gy = std::min<long long>(((long long)a.by + S3Y - 1) / S3Y, 65535);
    const long long gz = ((long long)a.bz + S3Z - 1) / S3Z;
    return dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
}

}  // namespace

// blocks of a launch over a.bx x a.by x a.bz: also the partials a stats launch writes
int stress3d_blocks(const Stress3Args &a) {
    const dim3 g = stress3d_grid(a);
    return (int)(g.x * g.y * g.z);
}

hipError_t launch_neq_strain3d(const Stress3Args &a, bool stats, hipStream_t s) {
    const dim3 g = stress3d_grid(a);
    if (g.z > 65535) return hipErrorInvalidValue;  // a slab of more than 65535 * S3Z planes
    if (stats)
        hipLaunchKernelGGL(neq_strain3d<true>, g, dim3(S3X * S3Y), 0, s, a);
    else
        hipLaunchKernelGGL(neq_strain3d<false>, g, dim3(S3X * S3Y), 0, s, a);
    return hipGetLastError();
}

// class maps of a handle that asked for the statistics: per slab
// uint8[nzs][ny][nx] on its device, and the near-wall cells counted while building
struct State3 {
    std::vector<uint8_t *> cls;
    long long wall_cells = 0;
};

}  // namespace stress
}  // namespace lbm

// ---- D3Q19 engine: host side ----

using namespace lbm;
using lbm::stress::Stress3Args;

// the cells [x0, x0+bx) x [y0, y0+by) x [z0, z0+bz) of slab s (z0 slab-local); the output pointers stay
// null.  Refuses omega = 1.
Stress3Args lbm3d_handle::stress_args(const Slab &s, int x0, int y0, int z0, int bx, int by, int bz) const {
    Stress3Args a{box_view(s, x0, y0, z0, bx, by, bz)};
    a.coef = neq_strain_coef(p.omega);
    return a;
}

// Build the class maps at the first statistics call.  x and y wrap inside the
// slab (every slab spans the full plane); the planes beyond a slab face come
// from the image planes of obst_g (the neighbour slab's, or the periodic image).
void lbm3d_handle::stress_build() {
    if (stress) return;
    auto *st = new stress::State3();
    stress = st;  // owned by the handle from here (stress_release)
    st->cls.assign(slabs.size(), nullptr);
    try {
        const int nx = p.nx, ny = p.ny;
        const size_t plane = (size_t)nx * ny;
        for (size_t k = 0; k < slabs.size(); ++k) {
            const Slab &s = slabs[k];
            HIP_CHECK(hipSetDevice(s.dev));
            const std::vector<uint8_t> g = obst_g_host(s);
            const uint8_t *g0 = g.data() + (size_t)GZ3 * plane;  // plane z = 0 of the slab
            std::vector<uint8_t> cls((size_t)s.nzs * plane);
            for (int z = 0; z < s.nzs; ++z)
                for (int y = 0; y < ny; ++y)
                    for (int x = 0; x < nx; ++x) {
                        const size_t i = ((size_t)z * ny + y) * nx + x;
                        uint8_t c = stress::CLS_BLOCKED;
                        if (!g0[i]) {
                            c = stress::CLS_FLUID;
                            for (int dz = -1; dz <= 1; ++dz)
                                for (int dy = -1; dy <= 1; ++dy)
                                    for (int dx = -1; dx <= 1; ++dx) {
                                        const int n = dx * dx + dy * dy + dz * dz;
                                        if (n == 0 || n == 3) continue;  // the 18 lattice neighbours
                                        const int xx = (x + dx + nx) % nx, yy = (y + dy + ny) % ny;
                                        if (g0[((long long)(z + dz) * ny + yy) * nx + xx]) c = stress::CLS_NEAR_WALL;
                                    }
                            if (c == stress::CLS_NEAR_WALL) ++st->wall_cells;
                        }
                        cls[i] = c;
                    }
            HIP_CHECK(hipMalloc(&st->cls[k], cls.size() + 256));
            HIP_CHECK(hipMemcpy(st->cls[k], cls.data(), cls.size(), hipMemcpyHostToDevice));
        }
    } catch (...) {
        stress_release();  // a later call builds again
        throw;
    }
}

void lbm3d_handle::stress_release() {
    if (!stress) return;
    for (size_t k = 0; k < stress->cls.size() && k < slabs.size(); ++k)
        if (stress->cls[k] && hipSetDevice(slabs[k].dev) == hipSuccess) (void)hipFree(stress->cls[k]);
    delete stress;
    stress = nullptr;
}

// The LBM3D_STRESS_* fields of the box's cells into the packed planar host
// arrays float[b.nz][b.ny][b.nx] (a NULL entry is neither computed nor
// staged), slab by slab as store_fields_box.
void lbm3d_handle::store_stress_box(const lbm3d_box &b, float *const *host) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to derive the strain rate from");
    check_box(b);
    const int want = count_wanted(host, LBM3D_STRESS_FIELDS);
    if (want == 0) return;
    stress_args(slabs.at(0), 0, 0, 0, 1, 1, 1);  // omega = 1 is refused before anything is launched or written
    sync_all();
    for (auto &s : slabs) {
        int zlo, zhi;
        if (!slab_planes(s, b, zlo, zhi)) continue;
        HIP_CHECK(hipSetDevice(s.dev));
        Stress3Args a = stress_args(s, b.x0, b.y0, zlo - s.z0, b.nx, b.ny, zhi - zlo);
        const size_t rows = (size_t)a.by * a.bz;
        const PlanarStage stage(want, rows * a.sp);
        for (int i = 0, n = 0; i < LBM3D_STRESS_FIELDS; ++i)
            if (host[i]) a.out[i] = stage.field(n++);
        HIP_CHECK(stress::launch_neq_strain3d(a, false, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(host, LBM3D_STRESS_FIELDS, box_span(b, zlo), (size_t)a.sp, (size_t)b.nx, rows);
    }
}

// Sum of S:S (fp64) and the largest strain over the local fluid cells; count,
// fp64 sum and maximum of the strain over the near-wall ones, from the kernel's
// per-block partials (BlockPartials, lbm_diag_host.hpp), slab after slab.
void lbm3d_handle::stress_stats(double *sum_s2, float *max_strain, int64_t *wall_cells, double *sum_wall_strain,
                                float *max_wall_strain) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take statistics of");
    if (!sum_s2 && !max_strain && !wall_cells && !sum_wall_strain && !max_wall_strain) return;
    stress_args(slabs.at(0), 0, 0, 0, 1, 1, 1);
    sync_all();
    stress_build();
    double sum[2] = {0.0, 0.0};  // s2, near-wall strain
    float max[2] = {0.f, 0.f};   // strain, near-wall strain
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        Stress3Args a = stress_args(s, 0, 0, 0, p.nx, p.ny, s.nzs);
        a.obst = stress->cls[k];
        const BlockPartials<2, 2> part((size_t)stress::stress3d_blocks(a));
        a.sum_part = part.sums();
        a.max_part = part.maxima();
        HIP_CHECK(stress::launch_neq_strain3d(a, true, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        part.fold(sum, max);
    }
    if (sum_s2) *sum_s2 = sum[0];
    if (max_strain) *max_strain = max[0];
    if (wall_cells) *wall_cells = stress->wall_cells;
    if (sum_wall_strain) *sum_wall_strain = sum[1];
    if (max_wall_strain) *max_wall_strain = max[1];
}
