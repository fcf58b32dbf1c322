// lbm3d_forces.hip -- the D3Q19 instantiation of the wall-list kernels
// (lbm_forces.hpp) behind lbm3d_wall_force, lbm3d_store_wall_force and
// lbm3d_body_forces (include/lbm_forces_hip.h), and the D3Q19 engine's host
// side of them (list build from obst_g, totals, per-body sums, the planar
// map); the wall list itself is in lbm_forces.hip.
//
// A wall cell's force comes from its own 18 moving populations (what the
// bounce-back of the last step stored there), each loaded only where its link
// bit is set; the list's offsets are relative to plane z = 0 of the slab, so
// the ghost planes and either lattice of the pair need no special case.
// IEEE fp32 in the written order, no contraction: the per-cell values equal
// lio.wall_force_cells3d of the stored cells bit for bit.

#include <climits>

#include "lbm3d_engine.hpp"

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

// ---- D3Q19 engine: host side ----

using namespace lbm;

// slab s's obstacle map with its three image planes each side, back on the host
std::vector<uint8_t> lbm3d_handle::obst_g_host(const Slab &s) const {
    std::vector<uint8_t> g((size_t)(s.nzs + 2 * GZ3) * p.ny * p.nx);
    HIP_CHECK(hipMemcpy(g.data(), s.obst_g, g.size(), hipMemcpyDeviceToHost));
    return g;
}

// Wall lists at the first force call, row-major per slab.  Links across a
// slab face come from the image planes of obst_g (the neighbour slab's
// planes, or the periodic wrap); x and y wrap inside the plane.
void lbm3d_handle::walls_build() {
    if (walls_built) return;
    // speed order of lbm3d_hip.h, j = 1..18
    static const int EX[19] = {0, 1, -1, 0, 0, 1, -1, 1, -1, 0, 1, -1, 0, 0, 0, -1, 1, 0, 0};
    static const int EY[19] = {0, 0, 0, 1, -1, 1, -1, -1, 1, 0, 0, 0, 1, -1, 0, 0, 0, -1, 1};
    static const int EZ[19] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    walls.assign(slabs.size(), forces::WallList());
    try {
        for (size_t k = 0; k < slabs.size(); ++k) {
            const Slab &s = slabs[k];
            HIP_CHECK(hipSetDevice(s.dev));
            const size_t plane = (size_t)p.ny * p.nx;
            if ((long long)s.nzs * (long long)plane > (long long)INT_MAX)
                throw lbm_failure(LBM_E_INVALID, "slab too large for a wall list");
            const std::vector<uint8_t> g = obst_g_host(s);
            forces::WallList &wl = walls[k];
            wl.dims = 3;
            for (int z = 0; z < s.nzs; ++z)
                for (int y = 0; y < p.ny; ++y) {
                    const uint8_t *row = g.data() + (size_t)(z + GZ3) * plane + (size_t)y * p.nx;
                    for (int x = 0; x < p.nx; ++x) {
                        if (!row[x]) continue;
                        unsigned m = 0;
                        for (int j = 1; j < Q3; ++j) {
                            const int xx = (x + EX[j] + p.nx) % p.nx, yy = (y + EY[j] + p.ny) % p.ny;
                            if (!g[(size_t)(z + EZ[j] + GZ3) * plane + (size_t)yy * p.nx + xx]) m |= 1u << (j - 1);
                        }
                        if (m) wl.add((long long)z * PL + (long long)y * px + x, (unsigned)(z * plane + (size_t)y * p.nx + x), m);
                    }
                }
            HIP_CHECK(wl.upload(0));
        }
    } catch (...) {
        walls_release();  // a later call builds again
        throw;
    }
    walls_built = true;
}

void lbm3d_handle::walls_release() {
    for (size_t k = 0; k < walls.size() && k < slabs.size(); ++k)
        if (hipSetDevice(slabs[k].dev) == hipSuccess) walls[k].release();
    walls.clear();
    walls_built = false;
    wall_bodies = 0;
}

void lbm3d_handle::wall_force(double *fx, double *fy, double *fz, int64_t *links) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take wall forces of");
    sync_all();
    walls_build();
    double f[3] = {0.0, 0.0, 0.0};
    long long nl = 0;
    for (size_t k = 0; k < slabs.size(); ++k) {
        Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        const forces::WallList &wl = walls[k];
        HIP_CHECK(wl.launch(forces::WALL_TOTAL, wl.args(s.o[s.cur], KS), s.s_comp));
        HIP_CHECK(wl.fetch_total(s.s_comp, f, nl));  // slab after slab, blocks in order
    }
    if (fx) *fx = f[0];
    if (fy) *fy = f[1];
    if (fz) *fz = f[2];
    if (links) *links = nl;
}

// per-cell forces into planar host arrays float[nz][ny][nx]: the wall cells
// scattered into zeroed staging arrays of the slab, copied to its planes
void lbm3d_handle::store_wall_force(float *const (&host)[3]) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take wall forces of");
    const int want = count_wanted(host, 3);
    if (want == 0) return;
    sync_all();
    walls_build();
    for (size_t k = 0; k < slabs.size(); ++k) {
        Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        const forces::WallList &wl = walls[k];
        forces::WallArgs a = wl.args(s.o[s.cur], KS);
        const size_t rows = (size_t)s.nzs * p.ny;
        const PlanarStage stage(want, rows * p.nx);
        HIP_CHECK(hipMemsetAsync(stage.get(), 0, stage.bytes(), s.s_comp));
        float **dev[3] = {&a.mx, &a.my, &a.mz};
        for (int i = 0, n = 0; i < 3; ++i)
            if (host[i]) *dev[i] = stage.field(n++);
        HIP_CHECK(wl.launch(forces::WALL_MAP, a, s.s_comp));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
        stage.copy_out(host, 3, HostSpan{(size_t)s.z0 * p.ny * p.nx, (size_t)p.nx}, (size_t)p.nx, (size_t)p.nx, rows);
    }
}

void lbm3d_handle::set_bodies(const int32_t *labels, int32_t nbodies) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice: load cells before setting bodies");
    if ((labels && nbodies <= 0) || (!labels && nbodies != 0))
        throw lbm_failure(LBM_E_INVALID, "labels with nbodies <= 0, or NULL labels with nbodies != 0");
    sync_all();
    walls_build();
    if (!labels) {
        if (wall_bodies == 0) return;
        for (size_t k = 0; k < slabs.size(); ++k) {
            HIP_CHECK(hipSetDevice(slabs[k].dev));
            walls[k].h_body.clear();
            HIP_CHECK(walls[k].upload(0));
        }
        wall_bodies = 0;
        return;
    }
    // every blocked cell's label is checked before anything changes
    const size_t plane = (size_t)p.ny * p.nx;
    std::vector<std::vector<int>> body(slabs.size());
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        const std::vector<uint8_t> g = obst_g_host(s);
        const int32_t *lab = labels + (size_t)s.z0 * plane;
        const uint8_t *ob = g.data() + (size_t)GZ3 * plane;
        for (size_t c = 0; c < (size_t)s.nzs * plane; ++c)
            if (ob[c] && lab[c] >= nbodies) throw lbm_failure(LBM_E_INVALID, "label >= nbodies on a blocked cell");
        const forces::WallList &wl = walls[k];
        body[k].resize(wl.h_cell.size());
        for (size_t i = 0; i < wl.h_cell.size(); ++i) body[k][i] = lab[wl.h_cell[i]] < 0 ? -1 : lab[wl.h_cell[i]];
    }
    for (size_t k = 0; k < slabs.size(); ++k) {
        HIP_CHECK(hipSetDevice(slabs[k].dev));
        walls[k].h_body.swap(body[k]);
        HIP_CHECK(walls[k].upload(nbodies));
    }
    wall_bodies = nbodies;
}

void lbm3d_handle::body_forces(double *fx, double *fy, double *fz, int64_t *links, int32_t nbodies) {
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to take wall forces of");
    if (!walls_built || wall_bodies == 0 || wall_bodies != nbodies)
        throw lbm_failure(LBM_E_STATE, "lbm3d_body_forces: no bodies set, or set with another nbodies");
    sync_all();
    for (int b = 0; b < nbodies; ++b) {
        if (fx) fx[b] = 0.0;
        if (fy) fy[b] = 0.0;
        if (fz) fz[b] = 0.0;
        if (links) links[b] = 0;
    }
    for (size_t k = 0; k < slabs.size(); ++k) {
        Slab &s = slabs[k];
        HIP_CHECK(hipSetDevice(s.dev));
        const forces::WallList &wl = walls[k];
        HIP_CHECK(wl.launch(forces::WALL_BODIES, wl.args(s.o[s.cur], KS), s.s_comp));
        HIP_CHECK(wl.fetch_bodies(s.s_comp, fx, fy, fz, links));  // slab after slab
    }
}
