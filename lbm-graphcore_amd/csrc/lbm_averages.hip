// lbm_averages.hip -- time-averaged fields and Reynolds stresses of the D2Q9
// engine on the device (the lbm_avg_* functions of
// include/lbm_averages_hip.h): the kernels of lbm_moments.hpp over the cell
// expressions macroscopic_fields compiles (lbm_cell_macro.hpp), then the
// engine's host side.
//
// A sample is one accumulate_moments launch per sub-domain on its compute
// stream, over the current side of the lattice pair in either layout (origin,
// plane and pitch as macroscopic_fields takes them); nothing goes to the host.

#include <hip/hip_runtime.h>

#include "lbm_averages_hip.h"
#include "lbm_cell_macro.hpp"
#include "lbm_engine.hpp"
#include "lbm_moments.hpp"

namespace lbm {
namespace avg {

struct D2Q9Sample {
    static constexpr int Q = 9, NV = 2;
    static __device__ __forceinline__ void sample(const float (&c)[Q], bool blocked, float obst_pressure,
                                                  float (&m)[NV + 1]) {
        float rho;
        const CellMacro v = cell_macro<true, false>(c, blocked, obst_pressure, rho);
        m[0] = v.ux;
        m[1] = v.uy;
        m[2] = v.pressure;
    }
};

}  // namespace avg
}  // namespace lbm

// ---- D2Q9 engine: host side ----

void lbm_handle::avg_begin(int moments) {
    std::vector<avg::Part> parts;
    for (const auto &s : subs) {
        avg::Part q;
        q.dev = s.dev;
        q.st = s.s_comp;
        q.w = s.w;
        q.rows = s.h;
        q.sp = (int)round_up(s.w, 4);
        q.host_off = (size_t)s.rect.y0 * p.nx + s.rect.x0;
        q.host_pitch = (size_t)p.nx;
        parts.push_back(q);
    }
    sync_all();
    avg::begin(averages, avg::D2Q9Sample::NV, moments, std::move(parts));
}

void lbm_handle::avg_sample() {
    if (!averages) throw lbm_failure(LBM_E_STATE, "not averaging: call lbm_avg_begin first");
    if (!loaded) throw lbm_failure(LBM_E_STATE, "no lattice to sample");
    sync_all();
    prof_drop();
    for (size_t k = 0; k < subs.size(); ++k) {
        const Sub &s = subs[k];
        const avg::Part &q = averages->parts[k];
        set_device(s);
        const LatticeView f = lattice_view(s);
        const avg::MomentArgs a{f.o, f.obst, 0, f.plane, f.pitch, f.w, f.h, f.h, f.sp, f.obst_pressure, q.acc, q.fstride()};
        timed(s, s.s_comp, "accumulate_moments", [&] {
            HIP_CHECK(avg::launch_accumulate<avg::D2Q9Sample>(a, averages->moments == 3, s.s_comp));
        });
    }
    for (const auto &s : subs) {
        set_device(s);
        HIP_CHECK(hipStreamSynchronize(s.s_comp));
    }
    prof_collect();
    averages->n++;
}

int64_t lbm_handle::avg_samples() const { return averages ? averages->n : 0; }

void lbm_handle::avg_store_sums(double *const *out) {
    sync_all();
    avg::store_sums(averages, out);
}

void lbm_handle::avg_store(float *const *out) {
    sync_all();
    prof_drop();
    avg::store_means(averages, out, [&](size_t k, const avg::Part &q, const avg::MeansArgs &m) {
        const Sub &s = subs[k];
        timed(s, s.s_comp, "moment_means", [&] { HIP_CHECK(avg::launch_means<avg::D2Q9Sample>(m, q.w, q.rows, s.s_comp)); });
    });
    prof_collect();
}

void lbm_handle::avg_end() {
    if (!averages) return;
    averages->release();
    delete averages;
    averages = nullptr;
}
