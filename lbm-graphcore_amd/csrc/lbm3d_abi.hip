// lbm3d_abi.hip -- the extern "C" functions of include/lbm3d_hip.h,
// include/lbm3d_fields_hip.h and the D3Q19 functions of
// include/lbm_forces_hip.h, include/lbm_averages_hip.h and
// include/lbm_gradients_hip.h, include/lbm_stress_hip.h and
// include/lbm_binned_hip.h and include/lbm_tracers_hip.h over the engine
// (lbm3d_engine.hpp), and the posting order of its RCCL ghost exchange.

#include "lbm3d_engine.hpp"
#include "lbm_averages_hip.h"
#include "lbm_binned_hip.h"
#include "lbm_gradients_hip.h"
#include "lbm_stress_hip.h"
#include "lbm_tracers_hip.h"

namespace lbm {
std::array<lbm_xfer, 4> slab_posts(int rank, int world, long long floats) {
    const int up = (rank + 1) % world, down = (rank + world - 1) % world;
    return {lbm_xfer{LBM_XFER_SEND, 0, up, 0, floats}, lbm_xfer{LBM_XFER_SEND, 1, down, 0, floats},
            lbm_xfer{LBM_XFER_RECV, 1, down, 0, floats}, lbm_xfer{LBM_XFER_RECV, 0, up, 0, floats}};
}
}  // namespace lbm

using namespace lbm;

namespace {
thread_local std::string g_err3;
}  // namespace

extern "C" {

int lbm3d_create(const lbm3d_params *params, const uint8_t *obstacles, const lbm_config *config, lbm3d_handle **out) {
    if (!params || !out) return LBM_E_INVALID;
    *out = nullptr;
    auto *h = new (std::nothrow) lbm3d_handle();
    if (!h) return LBM_E_NOMEM;
    lbm_config dflt{};
    dflt.parts = 1;
    const int rc = guarded(h, [&] { h->create(params, obstacles, config ? *config : dflt); });
    if (rc != LBM_OK) {
        g_err3 = h->err;
        h->destroy();
        delete h;
        return rc;
    }
    *out = h;
    return LBM_OK;
}

int lbm3d_init_equilibrium(lbm3d_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->init_equilibrium(); });
}

int lbm3d_load_cells(lbm3d_handle *h, const float *cells_aos) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->load_cells(cells_aos); });
}

int lbm3d_run_steps(lbm3d_handle *h, int32_t steps) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->run_steps(steps); });
}

int lbm3d_store(lbm3d_handle *h, float *cells_aos, float *av_vels, int32_t n_av) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->store(cells_aos, av_vels, n_av); });
}

int lbm3d_store_fields(lbm3d_handle *h, float *ux, float *uy, float *uz, float *speed, float *pressure) {
    if (!h) return LBM_E_INVALID;
    const lbm3d_box all{0, 0, 0, h->p.nx, h->p.ny, h->p.nz};
    return lbm3d_store_fields_box(h, &all, ux, uy, uz, speed, pressure);
}

int lbm3d_store_fields_box(lbm3d_handle *h, const lbm3d_box *box, float *ux, float *uy, float *uz, float *speed,
                           float *pressure) {
    if (!h || !box) return LBM_E_INVALID;
    float *const host[5] = {ux, uy, uz, speed, pressure};
    return guarded(h, [&] { h->store_fields_box(*box, host); });
}

int lbm3d_field_stats(lbm3d_handle *h, double *mass, float *max_speed) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->field_stats(mass, max_speed); });
}

int lbm3d_wall_force(lbm3d_handle *h, double *fx, double *fy, double *fz, int64_t *links) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->wall_force(fx, fy, fz, links); });
}

int lbm3d_store_wall_force(lbm3d_handle *h, float *fx, float *fy, float *fz) {
    if (!h) return LBM_E_INVALID;
    float *const host[3] = {fx, fy, fz};
    return guarded(h, [&] { h->store_wall_force(host); });
}

int lbm3d_set_bodies(lbm3d_handle *h, const int32_t *labels, int32_t nbodies) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->set_bodies(labels, nbodies); });
}

int lbm3d_body_forces(lbm3d_handle *h, double *fx, double *fy, double *fz, int64_t *links, int32_t nbodies) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->body_forces(fx, fy, fz, links, nbodies); });
}

int lbm3d_avg_begin(lbm3d_handle *h, int32_t moments) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->avg_begin(moments); });
}

int lbm3d_avg_sample(lbm3d_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->avg_sample(); });
}

int lbm3d_avg_samples(lbm3d_handle *h, int64_t *n) {
    if (!h || !n) return LBM_E_INVALID;
    return guarded(h, [&] { *n = h->avg_samples(); });
}

int lbm3d_avg_store_sums(lbm3d_handle *h, double *const out[LBM3D_AVG_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->avg_store_sums(out); });
}

int lbm3d_avg_store(lbm3d_handle *h, float *const out[LBM3D_AVG_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->avg_store(out); });
}

int lbm3d_avg_end(lbm3d_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->avg_end(); });
}

int lbm3d_store_gradients(lbm3d_handle *h, float *const out[LBM3D_GRAD_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    const lbm3d_box all{0, 0, 0, h->p.nx, h->p.ny, h->p.nz};
    return lbm3d_store_gradients_box(h, &all, out);
}

int lbm3d_store_gradients_box(lbm3d_handle *h, const lbm3d_box *box, float *const out[LBM3D_GRAD_FIELDS]) {
    if (!h || !box) return LBM_E_INVALID;
    return guarded(h, [&] { h->store_gradients_box(*box, out); });
}

int lbm3d_gradient_stats(lbm3d_handle *h, double *sum_w2, double *sum_s2, float *max_w, float *max_div) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->gradient_stats(sum_w2, sum_s2, max_w, max_div); });
}

int lbm3d_store_stress(lbm3d_handle *h, float *const out[LBM3D_STRESS_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    const lbm3d_box all{0, 0, 0, h->p.nx, h->p.ny, h->p.nz};
    return lbm3d_store_stress_box(h, &all, out);
}

int lbm3d_store_stress_box(lbm3d_handle *h, const lbm3d_box *box, float *const out[LBM3D_STRESS_FIELDS]) {
    if (!h || !box) return LBM_E_INVALID;
    return guarded(h, [&] { h->store_stress_box(*box, out); });
}

int lbm3d_stress_stats(lbm3d_handle *h, double *sum_s2, float *max_strain, int64_t *wall_cells,
                       double *sum_wall_strain, float *max_wall_strain) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->stress_stats(sum_s2, max_strain, wall_cells, sum_wall_strain, max_wall_strain); });
}

int lbm3d_store_binned(lbm3d_handle *h, int32_t bw, int32_t bh, int32_t bd, double *const out[LBM3D_BIN_FIELDS]) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->store_binned(bw, bh, bd, out); });
}

int lbm3d_bin_fluid_cells(lbm3d_handle *h, int32_t bw, int32_t bh, int32_t bd, int64_t *count) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->bin_fluid_cells(bw, bh, bd, count); });
}

int lbm3d_tracer_begin(lbm3d_handle *h, int64_t n, const double *x, const double *y, const double *z) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->tracer_begin(n, x, y, z); });
}

int lbm3d_tracer_count(lbm3d_handle *h, int64_t *n) {
    if (!h || !n) return LBM_E_INVALID;
    return guarded(h, [&] { *n = h->tracer_count(); });
}

int lbm3d_tracer_advance(lbm3d_handle *h, double dt, int32_t scheme) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->tracer_advance(dt, scheme); });
}

int lbm3d_tracer_sample(lbm3d_handle *h, double *ux, double *uy, double *uz, double *pressure) {
    if (!h) return LBM_E_INVALID;
    double *const host[4] = {ux, uy, uz, pressure};
    return guarded(h, [&] { h->tracer_sample(host); });
}

int lbm3d_tracer_store(lbm3d_handle *h, double *x, double *y, double *z, uint8_t *blocked) {
    if (!h) return LBM_E_INVALID;
    double *const host[3] = {x, y, z};
    return guarded(h, [&] { h->tracer_store(host, blocked); });
}

int lbm3d_tracer_end(lbm3d_handle *h) {
    if (!h) return LBM_E_INVALID;
    return guarded(h, [&] { h->tracer_end(); });
}

int lbm3d_last_run_seconds(lbm3d_handle *h, double *seconds) {
    if (!h || !seconds) return LBM_E_INVALID;
    *seconds = h->last_seconds;
    return LBM_OK;
}

int lbm3d_run_stats(lbm3d_handle *h, int32_t *three_step_passes, int32_t *two_step_passes,
                    int32_t *one_step_launches, int32_t *pair_kernel) {
    if (!h) return LBM_E_INVALID;
    if (three_step_passes) *three_step_passes = h->run_three;
    if (two_step_passes) *two_step_passes = h->run_two;
    if (one_step_launches) *one_step_launches = h->run_one;
    if (pair_kernel) *pair_kernel = h->pair ? 1 : 0;
    return LBM_OK;
}

int32_t lbm3d_numerics(lbm3d_handle *h) {
    if (!h) return -1;
    return h->tolerance && h->use_two() ? 1 : 0;  // only the passes run cell3dt
}

int64_t lbm3d_total_free_cells(lbm3d_handle *h) { return h ? h->free_cells : -1; }

int lbm3d_local_slabs(lbm3d_handle *h, int32_t *z0, int32_t *nz, int32_t max_slabs, int32_t *n_out) {
    if (!h) return LBM_E_INVALID;
    const int n = (int)h->slabs.size();
    if (n_out) *n_out = n;
    for (int i = 0; i < n && i < max_slabs; ++i) {
        if (z0) z0[i] = h->slabs[i].z0;
        if (nz) nz[i] = h->slabs[i].nzs;
    }
    return LBM_OK;
}

int lbm3d_exchange_schedule(int32_t nx, int32_t ny, int32_t nz, int32_t parts, int32_t rank, int32_t planes,
                            lbm_xfer *out, int32_t max_out, int32_t *n_out) {
    if (!n_out || nx < 1 || ny < 1 || parts < 1 || parts > nz || rank < 0 || rank >= parts || planes < 1 ||
        planes > 3)
        return LBM_E_INVALID;
    const long long KS = (long long)ny * ((nx + 15) / 16 * 16);  // the engine's speed stride (64-byte rows)
    const auto v = slab_posts(rank, parts, planes == 1 ? 5 * KS : (long long)planes * Q3 * KS);
    *n_out = (int32_t)v.size();
    if (out) {
        if (max_out < (int32_t)v.size()) return LBM_E_INVALID;
        for (size_t i = 0; i < v.size(); ++i) out[i] = v[i];
    }
    return LBM_OK;
}

const char *lbm3d_last_error(lbm3d_handle *h) { return h ? h->err.c_str() : g_err3.c_str(); }

void lbm3d_destroy(lbm3d_handle *h) {
    if (!h) return;
    try {
        h->destroy();
    } catch (...) {
    }
    delete h;
}

}  // extern "C"
