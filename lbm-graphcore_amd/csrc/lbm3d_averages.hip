// lbm3d_averages.hip -- time-averaged fields and Reynolds stresses of the
// D3Q19 engine on the device (the lbm3d_avg_* functions of
// include/lbm_averages_hip.h): the kernels of lbm_moments.hpp over the cell
// expressions macroscopic_fields3d compiles (lbm3d_cell_macro.hpp), then the
// engine's host side.
//
// A sample is one accumulate_moments launch per slab on its compute stream,
// over the ny * nzs rows of the slab's current lattice (rows start 16-B
// aligned: px is a multiple of 16 floats, KS and PL multiples of 4); nothing
// goes to the host.

#include <hip/hip_runtime.h>

#include "lbm3d_cell_macro.hpp"
#include "lbm3d_engine.hpp"
#include "lbm_averages_hip.h"
#include "lbm_moments.hpp"

namespace lbm {
namespace avg {

struct D3Q19Sample {
    static constexpr int Q = 19, NV = 3;
    static __device__ __forceinline__ void sample(const float (&c)[Q], bool blocked, float obst_pressure,
                                                  float (&m)[NV + 1]) {
        float rho;
        const Cell3Macro v = cell3_macro<true, false>(c, blocked, obst_pressure, rho);
        m[0] = v.ux;
        m[1] = v.uy;
        m[2] = v.uz;
        m[3] = v.pressure;
    }
};

}  // namespace avg
}  // namespace lbm

using namespace lbm;

// ---- D3Q19 engine: host side ----

void lbm3d_handle::avg_begin(int moments) {
    std::vector<avg::Part> parts;
    for (const auto &s : slabs) {
        if ((long long)p.ny * s.nzs > (long long)INT_MAX) throw lbm_failure(LBM_E_INVALID, "slab too large to average");
        avg::Part q;
        q.dev = s.dev;
        q.st = s.s_comp;
        q.w = p.nx;
        q.rows = p.ny * s.nzs;
        q.sp = (p.nx + 3) / 4 * 4;
        q.host_off = (size_t)s.z0 * p.ny * p.nx;
        q.host_pitch = (size_t)p.nx;
        parts.push_back(q);
    }
    sync_all();
    avg::begin(averages, avg::D3Q19Sample::NV, moments, std::move(parts));
}

void lbm3d_handle::avg_sample() {
    if (!averages) throw lbm_failure(LBM_E_STATE, "not averaging: call lbm3d_avg_begin first");
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to sample");
    sync_all();
    for (size_t k = 0; k < slabs.size(); ++k) {
        const Slab &s = slabs[k];
        const avg::Part &q = averages->parts[k];
        HIP_CHECK(hipSetDevice(s.dev));
        const avg::MomentArgs a{s.o[s.cur], s.obst, PL, KS, px, q.w, p.ny, q.rows, q.sp, p.density * (1.f / 3.f),
                                q.acc, q.fstride()};
        HIP_CHECK(avg::launch_accumulate<avg::D3Q19Sample>(a, averages->moments == 3, s.s_comp));
    }
    for (const auto &s : slabs) {
        HIP_CHECK(hipSetDevice(s.dev));
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    averages->n++;
}

int64_t lbm3d_handle::avg_samples() const { return averages ? averages->n : 0; }

void lbm3d_handle::avg_store_sums(double *const *out) {
    sync_all();
    avg::store_sums(averages, out);
}

void lbm3d_handle::avg_store(float *const *out) {
    sync_all();
    avg::store_means(averages, out, [&](size_t, const avg::Part &q, const avg::MeansArgs &m) {
        HIP_CHECK(avg::launch_means<avg::D3Q19Sample>(m, q.w, q.rows, q.st));
    });
}

void lbm3d_handle::avg_end() {
    if (!averages) return;
    averages->release();
    delete averages;
    averages = nullptr;
}
