// lbm_common.hpp -- what the D2Q9 engine (lbm_engine.hpp) and the D3Q19 engine
// (lbm3d_engine.hpp) share on the host: the failure type behind the LBM_E_*
// return codes, the HIP / RCCL call checks, the catch-all of the extern "C"
// layers, and the owner of a device staging allocation.  What the diagnostics
// build on it (planar staging, block partials) is in lbm_diag_host.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <new>
#include <stdexcept>
#include <string>

#include "lbm_hip.h"

namespace lbm {

struct lbm_failure : std::runtime_error {
    int code;
    lbm_failure(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

#define HIP_CHECK(expr)                                                                                  \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess)                                                                            \
            throw lbm::lbm_failure(LBM_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

#define NCCL_CHECK(expr)                                                                                 \
    do {                                                                                                 \
        ncclResult_t r_ = (expr);                                                                        \
        if (r_ != ncclSuccess)                                                                           \
            throw lbm::lbm_failure(LBM_E_RCCL, std::string(#expr) + ": " + ncclGetErrorString(r_));      \
    } while (0)

// run f; a failure becomes its LBM_E_* code and the handle's error text
template <class H, class F>
int guarded(H *h, F &&f) {
    try {
        f();
        return LBM_OK;
    } catch (const lbm_failure &e) {
        if (h) h->err = e.what();
        return e.code;
    } catch (const std::bad_alloc &) {
        if (h) h->err = "host allocation failed";
        return LBM_E_NOMEM;
    } catch (const std::exception &e) {
        if (h) h->err = e.what();
        return LBM_E_INTERNAL;
    } catch (...) {
        if (h) h->err = "unknown failure";
        return LBM_E_INTERNAL;
    }
}

// a device staging allocation of the current device, freed when it leaves scope
class DeviceStage {
    void *p_ = nullptr;

public:
    explicit DeviceStage(size_t bytes) { HIP_CHECK(hipMalloc(&p_, bytes)); }
    ~DeviceStage() { (void)hipFree(p_); }
    DeviceStage(const DeviceStage &) = delete;
    DeviceStage &operator=(const DeviceStage &) = delete;
    void *get() const { return p_; }
    template <class T>
    T *as() const { return static_cast<T *>(p_); }
};

}  // namespace lbm
