// lbm_tracers.hip -- Lagrangian tracers and point probes of the D2Q9 engine
// (the lbm_tracer_* functions of include/lbm_tracers_hip.h): the kernels and
// per-point functions of lbm_tracers.hpp over the lattices of the handle's
// sub-domains, the engine's host side, and the host-only restatements
// lbm_tracer_advance_ref / lbm_tracer_sample_ref over planar fields.
//
// One launch per call on the compute stream of the first sub-domain, after a
// synchronisation of every stream: the views of all local sub-domains travel
// in the kernel argument block, and a point reads each corner from whichever
// sub-domain owns it, never from a ghost ring.
//
// Arithmetic: cell values in IEEE fp32 as lbm_fields.hip forms them, the rest
// fp64, no contraction (-ffp-contract=off), correctly rounded divide.

#include <hip/hip_runtime.h>

#include "lbm_engine.hpp"
#include "lbm_tracers.hpp"
#include "lbm_tracers_hip.h"

namespace {

tracer::Dev2 tracer_field(const lbm_handle &h) {
    tracer::Dev2 f{};
    f.nviews = (int)h.subs.size();
    f.nx = h.p.nx;
    f.ny = h.p.ny;
    for (int k = 0; k < f.nviews; ++k) f.view[k] = tracer::View2{h.lattice_view(h.subs[k]), h.subs[k].rect.x0, h.subs[k].rect.y0};
    return f;
}

tracer::State &tracer_set(lbm_handle &h) {
    if (!h.tracers) throw lbm_failure(LBM_E_STATE, "no tracer set: call lbm_tracer_begin first");
    return *h.tracers;
}

}  // namespace

// ---- D2Q9 engine: host side ----

void lbm_handle::tracer_begin(int64_t n, const double *x, const double *y) {
    if (transport == LBM_TRANSPORT_RCCL && world > 1)
        throw lbm_failure(LBM_E_INVALID, "tracer sets on RCCL handles of more than one rank are not built");
    if ((int)subs.size() > tracer::MAX_VIEWS)
        throw lbm_failure(LBM_E_INVALID, "tracer sets on more than 16 local sub-domains are not built");
    long long cells = 0;
    for (const auto &s : subs) {
        if (s.dev != subs[0].dev)
            throw lbm_failure(LBM_E_INVALID, "tracer sets on sub-domains of more than one device are not built");
        cells += (long long)s.w * s.h;
    }
    if (subs.empty() || cells != (long long)p.nx * p.ny)
        throw lbm_failure(LBM_E_INVALID, "tracer sets need every sub-domain of the domain on this handle");
    const double *const seed[2] = {x, y};
    const int extent[2] = {p.nx, p.ny};
    tracer::check_seeds(2, extent, n, seed);
    sync_all();
    tracer::begin(tracers, subs[0].dev, 2, n, seed);
}

int64_t lbm_handle::tracer_count() const { return tracers ? tracers->n : 0; }

void lbm_handle::tracer_advance(double dt, int scheme) {
    tracer::State &t = tracer_set(*this);
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to advance the tracers in");
    sync_all();
    prof_drop();
    const Sub &s = subs[0];
    set_device(s);
    tracer::run_advance(tracer_field(*this), t, dt, scheme, s.s_comp,
                        [&](auto &&launch) { timed(s, s.s_comp, "advance_tracers", launch); });
    prof_collect();
}

void lbm_handle::tracer_sample(double *ux, double *uy, double *pressure) {
    tracer::State &t = tracer_set(*this);
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to sample");
    double *const host[3] = {ux, uy, pressure};
    if (count_wanted(host, 3) == 0) return;
    sync_all();
    prof_drop();
    const Sub &s = subs[0];
    set_device(s);
    tracer::run_sample(tracer_field(*this), t, host, s.s_comp,
                       [&](auto &&launch) { timed(s, s.s_comp, "sample_tracers", launch); });
    prof_collect();
}

void lbm_handle::tracer_store(double *x, double *y, uint8_t *blocked) {
    tracer::State &t = tracer_set(*this);
    sync_all();
    const Sub &s = subs[0];
    set_device(s);
    double *const host[2] = {x, y};
    tracer::run_store(tracer_field(*this), t, host, blocked, s.s_comp);
}

void lbm_handle::tracer_end() { tracer::end(tracers); }

// ---- host-only restatements over planar fields ----

extern "C" {

int lbm_tracer_advance_ref(int32_t nx, int32_t ny, const float *ux, const float *uy, int64_t n, double *x, double *y,
                           double dt, int32_t scheme) {
    if (n < 0 || !ux || !uy || !std::isfinite(dt) || (scheme != LBM_TRACER_EULER && scheme != LBM_TRACER_HEUN) ||
        !tracer::in_range(n, x, nx) || !tracer::in_range(n, y, ny))
        return LBM_E_INVALID;
    const tracer::Planar2 f{ux, uy, nullptr, nx, ny};
    for (int64_t i = 0; i < n; ++i) tracer::advance2(f, x[i], y[i], dt, scheme);
    return LBM_OK;
}

int lbm_tracer_sample_ref(int32_t nx, int32_t ny, const float *ux, const float *uy, const float *pressure, int64_t n,
                          const double *x, const double *y, double *out_ux, double *out_uy, double *out_p) {
    if (n < 0 || (out_ux && !ux) || (out_uy && !uy) || (out_p && !pressure) || !tracer::in_range(n, x, nx) ||
        !tracer::in_range(n, y, ny))
        return LBM_E_INVALID;
    const tracer::Planar2 f{ux, uy, pressure, nx, ny};
    for (int64_t i = 0; i < n; ++i) {
        const tracer::Val2 v = tracer::interp2(f, x[i], y[i]);
        if (out_ux) out_ux[i] = v.ux;
        if (out_uy) out_uy[i] = v.uy;
        if (out_p) out_p[i] = v.p;
    }
    return LBM_OK;
}

}  // extern "C"
