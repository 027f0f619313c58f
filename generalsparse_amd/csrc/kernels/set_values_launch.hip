// set_values_launch.hip -- launches of k_set_values (hip_code/set_values.hpp): the device-side value
// update behind gs_plan_set_values.  One object holds the fp16 and the bf16 instantiation.
#include "../hip_code/set_values.hpp"
#include "launch_common.hpp"

#include <algorithm>

namespace gs {

void launch_set_values(int dtype, void *tval, const uint32_t *src, const float *values, uint64_t n_groups, hipStream_t s) {
    GS_CHECK(dtype == kF16 || dtype == kBF16, "k_set_values writes f16 and bf16 values");
    GS_CHECK(tval && src && values && n_groups >= 1 && n_groups < (1ull << 32), "k_set_values: bad arguments");
    GS_CHECK((uintptr_t)tval % 16 == 0 && (uintptr_t)src % 16 == 0, "k_set_values: the value array and the map are 16-byte aligned");
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((n_groups + 255) / 256, 4096);
    if (dtype == kBF16)
        hipLaunchKernelGGL(gsk::k_set_values<gsk::bf16>, dim3(blocks), dim3(256), 0, s, (uint16_t *)tval, src, values, n_groups);
    else
        hipLaunchKernelGGL(gsk::k_set_values<gsk::f16>, dim3(blocks), dim3(256), 0, s, (uint16_t *)tval, src, values, n_groups);
    HIP_OK(hipGetLastError());
}

}  // namespace gs
