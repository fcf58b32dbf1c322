// lbm3d_tracers.hip -- Lagrangian tracers and point probes of the D3Q19 engine
// (the lbm3d_tracer_* functions of include/lbm_tracers_hip.h): the kernels and
// per-point functions of lbm_tracers.hpp over the lattices of the handle's z
// slabs, the engine's host side, and the host-only restatements
// lbm3d_tracer_advance_ref / lbm3d_tracer_sample_ref over planar fields.
//
// One launch per call on the compute stream of the first slab, after a
// synchronisation of every stream: the views of all local slabs travel in the
// kernel argument block, and a point reads each corner plane from whichever
// slab owns it, never from a ghost plane.  Offsets are formed in 64 bits
// (512^3 x 19 floats exceeds 2^31).
//
// Arithmetic: cell values in IEEE fp32 as lbm3d_fields.hip forms them, the
// rest fp64, no contraction (-ffp-contract=off), correctly rounded divide.

#include <hip/hip_runtime.h>

#include "lbm3d_engine.hpp"
#include "lbm_tracers.hpp"
#include "lbm_tracers_hip.h"

using namespace lbm;

namespace {

tracer::Dev3 tracer_field(const lbm3d_handle &h) {
    tracer::Dev3 f{};
    f.nviews = (int)h.slabs.size();
    f.nx = h.p.nx;
    f.ny = h.p.ny;
    f.nz = h.p.nz;
    for (int k = 0; k < f.nviews; ++k) {
        const Slab &s = h.slabs[k];
        f.view[k] = tracer::View3{h.box_view(s, 0, 0, 0, h.p.nx, h.p.ny, s.nzs), s.z0};
    }
    return f;
}

tracer::State &tracer_set(lbm3d_handle &h) {
    if (!h.tracers) throw lbm_failure(LBM_E_STATE, "no tracer set: call lbm3d_tracer_begin first");
    return *h.tracers;
}

const auto run_directly = [](auto &&launch) { launch(); };  // no profile classes on this engine

}  // namespace

// ---- D3Q19 engine: host side ----

void lbm3d_handle::tracer_begin(int64_t n, const double *x, const double *y, const double *z) {
    if (transport == LBM_TRANSPORT_RCCL && world > 1)
        throw lbm_failure(LBM_E_INVALID, "tracer sets on RCCL handles of more than one rank are not built");
    if ((int)slabs.size() > tracer::MAX_VIEWS)
        throw lbm_failure(LBM_E_INVALID, "tracer sets on more than 16 local slabs are not built");
    int planes = 0;
    for (const auto &s : slabs) {
        if (s.dev != slabs[0].dev)
            throw lbm_failure(LBM_E_INVALID, "tracer sets on slabs of more than one device are not built");
        planes += s.nzs;
    }
    if (slabs.empty() || planes != p.nz)
        throw lbm_failure(LBM_E_INVALID, "tracer sets need every slab of the domain on this handle");
    const double *const seed[3] = {x, y, z};
    const int extent[3] = {p.nx, p.ny, p.nz};
    tracer::check_seeds(3, extent, n, seed);
    sync_all();
    tracer::begin(tracers, slabs[0].dev, 3, n, seed);
}

int64_t lbm3d_handle::tracer_count() const { return tracers ? tracers->n : 0; }

void lbm3d_handle::tracer_advance(double dt, int scheme) {
    tracer::State &t = tracer_set(*this);
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to advance the tracers in");
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    tracer::run_advance(tracer_field(*this), t, dt, scheme, slabs[0].s_comp, run_directly);
}

void lbm3d_handle::tracer_sample(double *const (&host)[4]) {
    tracer::State &t = tracer_set(*this);
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to sample");
    if (count_wanted(host, 4) == 0) return;
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    tracer::run_sample(tracer_field(*this), t, host, slabs[0].s_comp, run_directly);
}

void lbm3d_handle::tracer_store(double *const (&host)[3], uint8_t *blocked) {
    tracer::State &t = tracer_set(*this);
    sync_all();
    HIP_CHECK(hipSetDevice(slabs[0].dev));
    tracer::run_store(tracer_field(*this), t, host, blocked, slabs[0].s_comp);
}

void lbm3d_handle::tracer_end() { tracer::end(tracers); }

// ---- host-only restatements over planar fields ----

extern "C" {

int lbm3d_tracer_advance_ref(int32_t nx, int32_t ny, int32_t nz, const float *ux, const float *uy, const float *uz,
                             int64_t n, double *x, double *y, double *z, double dt, int32_t scheme) {
    if (n < 0 || !ux || !uy || !uz || !std::isfinite(dt) ||
        (scheme != LBM_TRACER_EULER && scheme != LBM_TRACER_HEUN) || !tracer::in_range(n, x, nx) ||
        !tracer::in_range(n, y, ny) || !tracer::in_range(n, z, nz))
        return LBM_E_INVALID;
    const tracer::Planar3 f{ux, uy, uz, nullptr, nx, ny, nz};
    for (int64_t i = 0; i < n; ++i) tracer::advance3(f, x[i], y[i], z[i], dt, scheme);
    return LBM_OK;
}

int lbm3d_tracer_sample_ref(int32_t nx, int32_t ny, int32_t nz, const float *ux, const float *uy, const float *uz,
                            const float *pressure, int64_t n, const double *x, const double *y, const double *z,
                            double *out_ux, double *out_uy, double *out_uz, double *out_p) {
    if (n < 0 || (out_ux && !ux) || (out_uy && !uy) || (out_uz && !uz) || (out_p && !pressure) ||
        !tracer::in_range(n, x, nx) || !tracer::in_range(n, y, ny) || !tracer::in_range(n, z, nz))
        return LBM_E_INVALID;
    const tracer::Planar3 f{ux, uy, uz, pressure, nx, ny, nz};
    for (int64_t i = 0; i < n; ++i) {
        const tracer::Val3 v = tracer::interp3(f, x[i], y[i], z[i]);
        if (out_ux) out_ux[i] = v.ux;
        if (out_uy) out_uy[i] = v.uy;
        if (out_uz) out_uz[i] = v.uz;
        if (out_p) out_p[i] = v.p;
    }
    return LBM_OK;
}

}  // extern "C"
