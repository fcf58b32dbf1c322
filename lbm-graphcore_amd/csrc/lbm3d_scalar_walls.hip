// lbm3d_scalar_walls.hip -- wall models of the D3Q19 engine's passive scalar
// and the per-body wall flux (the lbm3d_scalar_* functions of
// include/lbm_scalar_walls_hip.h): the D3Q7 instantiation of the kernels of
// lbm_scalar_walls.hpp, the engine's host side, the extern "C" functions and
// the host-only restatement lbm3d_scalar_walls_ref.  What both engines share
// outside templates is in lbm_scalar_walls.hip.
//
// At most six floats per wall cell, gated by the link bits; one list over the
// whole domain, whatever the slabs.  IEEE fp32 in the written order, no
// contraction: pass and per-cell flux equal lio.scalar_apply_walls3d and
// lio.scalar_wall_flux_cells3d bit for bit.

#include "lbm_scalar_walls.hpp"

#include "lbm3d_engine.hpp"

namespace lbm {
namespace scalar {

hipError_t walls_pass3d(const State &s, float *g, hipStream_t st) { return launch_pass<7>(s, g, st); }

}  // namespace scalar
}  // namespace lbm

using namespace lbm;

namespace {

scalar::State &walls_state(lbm3d_handle &h) {
    if (!h.scalars) throw lbm_failure(LBM_E_STATE, "no scalar: call lbm3d_scalar_begin first");
    return *h.scalars;
}

const auto run_directly = [](auto &&launch) { launch(); };  // no profile classes on this engine

}  // namespace

// ---- D3Q19 engine: host side ----

// the obstacle map of the whole domain, assembled from the slabs' maps
std::vector<uint8_t> lbm3d_handle::obst_host() const {
    const size_t plane = (size_t)p.ny * p.nx;
    std::vector<uint8_t> full(plane * p.nz, 0);
    for (const auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipMemcpy(full.data() + (size_t)s.z0 * plane, s.obst, plane * s.nzs, hipMemcpyDeviceToHost));
    }
    return full;
}

void lbm3d_handle::scalar_set_walls(const int32_t *labels, int32_t nbodies, const int32_t *kind, const float *value) {
    scalar::State &t = walls_state(*this);
    sync_all();
    scalar::set_walls<7>(t, labels, nbodies, kind, value, [&] {
        std::vector<uint8_t> ob = obst_host();
        HIP_CHECK(hipSetDevice(t.dev));
        return ob;
    });
}

void lbm3d_handle::scalar_wall_flux(double *q, int64_t *links) {
    scalar::State &t = walls_state(*this);
    sync_all();
    scalar::wall_flux_total<7>(t, slabs[0].s_comp, q, links, run_directly);
}

void lbm3d_handle::scalar_body_flux(double *q, int64_t *links, int32_t nbodies) {
    scalar::State &t = walls_state(*this);
    sync_all();
    scalar::wall_flux_bodies<7>(t, slabs[0].s_comp, q, links, nbodies, run_directly);
}

void lbm3d_handle::scalar_store_wall_flux(float *q) {
    scalar::State &t = walls_state(*this);
    sync_all();
    scalar::wall_flux_store<7>(t, slabs[0].s_comp, q, run_directly);
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm3d_scalar_set_walls(lbm3d_handle *h, const int32_t *labels, int32_t nbodies, const int32_t *kind,
                           const float *value) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_set_walls(labels, nbodies, kind, value); });
}

int lbm3d_scalar_wall_flux(lbm3d_handle *h, double *q, int64_t *links) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_wall_flux(q, links); });
}

int lbm3d_scalar_body_flux(lbm3d_handle *h, double *q, int64_t *links, int32_t nbodies) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_body_flux(q, links, nbodies); });
}

int lbm3d_scalar_store_wall_flux(lbm3d_handle *h, float *q) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_store_wall_flux(q); });
}

int lbm3d_scalar_walls_ref(int32_t nx, int32_t ny, int32_t nz, const uint8_t *obst, const int32_t *labels,
                           int32_t nbodies, const int32_t *kind, const float *value, float *g, float *q) {
    return scalar::walls_ref<7>(nx, ny, nz, obst, labels, nbodies, kind, value, g, q);
}

}  // extern "C"
