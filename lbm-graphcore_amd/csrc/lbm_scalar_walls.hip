// lbm_scalar_walls.hip -- wall models of the D2Q9 engine's passive scalar and
// the per-body wall flux (the lbm_scalar_* functions of
// include/lbm_scalar_walls_hip.h): the D2Q5 instantiation of the kernels of
// lbm_scalar_walls.hpp, what both engines share outside templates, the
// engine's host side, the extern "C" functions and the host-only restatement
// lbm_scalar_walls_ref.
//
// An obstacle cell's stored scalar populations are what the step's bounce-back
// left there, and the fluid cell along link k pulls g_k in the next step: the
// pass rewrites at most four floats per wall cell, the flux is a gather of at
// most four, both gated by the link bits.  The list holds offsets inside a
// scalar plane, the same on both sets of the ping-pong pair.
//
// Arithmetic: IEEE fp32 in the written order, no contraction
// (-ffp-contract=off): pass and per-cell flux equal lio.scalar_apply_walls and
// lio.scalar_wall_flux_cells bit for bit.

#include "lbm_scalar_walls.hpp"

#include "lbm_engine.hpp"

namespace lbm {
namespace scalar {

void walls_free(Walls *w) {
    if (!w) return;
    w->list.release();
    (void)hipFree(w->body);
    (void)hipFree(w->tab);
    delete w;
}

bool walls_listed(const State &s) { return s.walls && s.walls->nlab > 0; }

hipError_t walls_pass2d(const State &s, float *g, hipStream_t st) { return launch_pass<5>(s, g, st); }

}  // namespace scalar
}  // namespace lbm

namespace {

scalar::State &walls_state(lbm_handle &h) {
    if (!h.scalars) throw lbm_failure(LBM_E_STATE, "no scalar: call lbm_scalar_begin first");
    return *h.scalars;
}

}  // namespace

// ---- D2Q9 engine: host side ----

// the obstacle map of the whole domain, assembled from the sub-domains' maps
std::vector<uint8_t> lbm_handle::obst_host() const {
    std::vector<uint8_t> full((size_t)p.nx * p.ny, 0);
    for (const auto &s : subs) {
        set_device(s);
        HIP_CHECK(hipMemcpy2D(full.data() + (size_t)s.rect.y0 * p.nx + s.rect.x0, (size_t)p.nx, s.obst, (size_t)s.w,
                              (size_t)s.w, (size_t)s.h, hipMemcpyDeviceToHost));
    }
    return full;
}

void lbm_handle::scalar_set_walls(const int32_t *labels, int32_t nbodies, const int32_t *kind, const float *value) {
    scalar::State &t = walls_state(*this);
    sync_all();
    scalar::set_walls<5>(t, labels, nbodies, kind, value, [&] {
        std::vector<uint8_t> ob = obst_host();
        HIP_CHECK(hipSetDevice(t.dev));
        return ob;
    });
}

void lbm_handle::scalar_wall_flux(double *q, int64_t *links) {
    scalar::State &t = walls_state(*this);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    scalar::wall_flux_total<5>(t, s0.s_comp, q, links,
                               [&](auto &&launch) { timed(s0, s0.s_comp, "scalar_wall_flux", launch); });
    prof_collect();
}

void lbm_handle::scalar_body_flux(double *q, int64_t *links, int32_t nbodies) {
    scalar::State &t = walls_state(*this);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    scalar::wall_flux_bodies<5>(t, s0.s_comp, q, links, nbodies,
                                [&](auto &&launch) { timed(s0, s0.s_comp, "scalar_wall_flux bodies", launch); });
    prof_collect();
}

void lbm_handle::scalar_store_wall_flux(float *q) {
    scalar::State &t = walls_state(*this);
    sync_all();
    prof_drop();
    const Sub &s0 = subs[0];
    set_device(s0);
    scalar::wall_flux_store<5>(t, s0.s_comp, q,
                               [&](auto &&launch) { timed(s0, s0.s_comp, "scalar_wall_flux map", launch); });
    prof_collect();
}

// ---- C ABI and the host-only restatement ----

extern "C" {

int lbm_scalar_set_walls(lbm_handle *h, const int32_t *labels, int32_t nbodies, const int32_t *kind,
                         const float *value) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_set_walls(labels, nbodies, kind, value); });
}

int lbm_scalar_wall_flux(lbm_handle *h, double *q, int64_t *links) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_wall_flux(q, links); });
}

int lbm_scalar_body_flux(lbm_handle *h, double *q, int64_t *links, int32_t nbodies) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_body_flux(q, links, nbodies); });
}

int lbm_scalar_store_wall_flux(lbm_handle *h, float *q) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->scalar_store_wall_flux(q); });
}

int lbm_scalar_walls_ref(int32_t nx, int32_t ny, const uint8_t *obst, const int32_t *labels, int32_t nbodies,
                         const int32_t *kind, const float *value, float *g, float *q) {
    return scalar::walls_ref<5>(nx, ny, 1, obst, labels, nbodies, kind, value, g, q);
}

}  // extern "C"
