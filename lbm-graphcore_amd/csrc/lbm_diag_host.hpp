// lbm_diag_host.hpp -- the host paths the diagnostics of both engines share
// (fields, wall-force fields, averages, gradients, strain): counting the
// requested outputs, the staging of planar float fields and their copy into
// the caller's arrays, the per-block partials of a statistics launch and
// their fold, and the coefficient of the non-equilibrium strain rate.
// Launching stays with the caller, between construction and the copy or fold.
#pragma once

#include <algorithm>
#include <cstring>
#include <memory>

#include "lbm_common.hpp"

namespace lbm {

// the non-NULL entries of an array of n output pointers (a NULL array: none)
template <class P>
int count_wanted(P *const *out, int n) {
    int want = 0;
    for (int i = 0; out && i < n; ++i) want += out[i] ? 1 : 0;
    return want;
}

// where one part's rows lie in the caller's planar arrays: first entry and row pitch, in entries
struct HostSpan {
    size_t off, pitch;
};

// Staging of `want` planar float fields of field_floats entries each on the
// current device: the k-th requested output owns field(k).
class PlanarStage {
    DeviceStage mem_;
    size_t field_floats_, bytes_;

public:
    PlanarStage(int want, size_t field_floats)
        : mem_(sizeof(float) * field_floats * want), field_floats_(field_floats),
          bytes_(sizeof(float) * field_floats * want) {}
    float *field(int k) const { return mem_.as<float>() + field_floats_ * k; }
    void *get() const { return mem_.get(); }
    size_t bytes() const { return bytes_; }
    // Every requested field (host[i] non-NULL, i < n, in order) to host[i] + to.off:
    // `rows` rows of `row` floats, stage_pitch floats apart in the staging array
    // and to.pitch apart at the caller's.  Unpadded on both sides: one contiguous copy.
    void copy_out(float *const *host, int n, HostSpan to, size_t stage_pitch, size_t row, size_t rows) const {
        for (int i = 0, k = 0; i < n; ++i) {
            if (!host[i]) continue;
            const float *from = field(k++);
            if (to.pitch == row && stage_pitch == row)
                HIP_CHECK(hipMemcpy(host[i] + to.off, from, sizeof(float) * row * rows, hipMemcpyDeviceToHost));
            else
                HIP_CHECK(hipMemcpy2D(host[i] + to.off, sizeof(float) * to.pitch, from, sizeof(float) * stage_pitch,
                                      sizeof(float) * row, rows, hipMemcpyDeviceToHost));
        }
    }
};

// The partials a statistics launch of nb blocks leaves on the current device:
// [NS][nb] fp64 sums, then [NM][nb] fp32 maxima.
template <int NS, int NM>
class BlockPartials {
    DeviceStage mem_;
    size_t nb_;

public:
    explicit BlockPartials(size_t nb) : mem_((sizeof(double) * NS + sizeof(float) * NM) * nb), nb_(nb) {}
    double *sums() const { return mem_.as<double>(); }
    float *maxima() const { return reinterpret_cast<float *>(sums() + NS * nb_); }
    // Once the launch has completed: block 0 .. nb - 1 into the caller's running
    // totals.  Called sub-domain after sub-domain, so the same lattice always
    // gives the same bits.
    void fold(double (&sum)[NS], float (&max)[NM]) const {
        // one copy of the whole block into an uninitialised buffer; the floats start where the doubles end
        const size_t bytes = (sizeof(double) * NS + sizeof(float) * NM) * nb_;
        const std::unique_ptr<double[]> buf(new double[(bytes + sizeof(double) - 1) / sizeof(double)]);
        HIP_CHECK(hipMemcpy(buf.get(), mem_.get(), bytes, hipMemcpyDeviceToHost));
        const double *s = buf.get();
        const char *m = reinterpret_cast<const char *>(s + NS * nb_);
        for (size_t b = 0; b < nb_; ++b) {
            for (int j = 0; j < NS; ++j) sum[j] += s[j * nb_ + b];
            for (int j = 0; j < NM; ++j) {
                float v;
                memcpy(&v, m + sizeof(float) * (j * nb_ + b), sizeof(float));
                max[j] = std::max(max[j], v);
            }
        }
    }
};

// coefficient of the non-equilibrium strain rate, formed once in fp32; refuses omega = 1
inline float neq_strain_coef(float omega) {
    const float omo = 1.f - omega;
    if (omo == 0.f)
        throw lbm_failure(LBM_E_INVALID,
                          "omega = 1: the post-collision lattice carries no non-equilibrium part to take the strain "
                          "rate from");
    return (-1.5f * omega) / omo;
}

}  // namespace lbm
