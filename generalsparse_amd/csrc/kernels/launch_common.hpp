// kernels/launch_common.hpp -- what the upload and the launch files (device_plan.hip,
// gather_launch.hip, mfma_launch.hip, sddmm_launch.hip, set_values_launch.hip and, through ks_dispatch.hpp, ks_launch.hip,
// ks_w8_launch.hip, ks_tm_launch.hip) share: the HIP error check, the dynamic-LDS opt-in and the
// dispatch on a plan's dtype.
#pragma once

#include "../host/gs_plan.hpp"

#include <map>
#include <mutex>
#include <string>
#include <utility>

#define HIP_OK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) throw gs_error(std::string(#x) + ": " + hipGetErrorString(e_), -3); \
    } while (0)

namespace gs {

template <class KERN>
void grant_lds(int device, KERN kern, size_t bytes) {
    // dynamic LDS above 64 KB is opted into once per kernel and device
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> granted;
    std::lock_guard<std::mutex> l(mu);
    size_t &g = granted[{device, reinterpret_cast<const void *>(kern)}];
    if (g < bytes) {
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)bytes));
        g = bytes;
    }
}

// calls f with a value of the dtype's element type (float, gsk::f16 or gsk::bf16), for a launch templated on it
template <class F>
void by_dtype(int dtype, F &&f) {
    if (dtype == kF32) f(float{});
    else if (dtype == kBF16) f(__bf16{});
    else f(_Float16{});
}

}  // namespace gs
