// hip_code/set_values.hpp -- k_set_values: A's values of an uploaded k_mfma_ks plan rewritten in place
// from a device array of new fp32 values (gs_plan_set_values).  Instantiated by kernels/set_values_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// a slot of the value array that holds no entry (host/device_layout.hpp kNoValue)
constexpr uint32_t kSetNoValue = 0xffffffffu;

// fp32 -> the plan dtype's 16-bit word, with the bits of the upload's host conversion (device_layout.cc
// f32_to_f16_bits / f32_to_bf16_bits): round to nearest even, subnormals kept, overflow to Inf.
// f16: the hardware conversion (v_cvt_f16_f32: the same rounding, a NaN keeps its upper payload bits quiet).
// bf16: the host's integer arithmetic, so that a NaN keeps its upper bits with the quiet bit set whatever
// the hardware conversion makes of its payload
template <class T>
__device__ __forceinline__ uint32_t set_value_bits(float f) {
    if constexpr (std::is_same<T, bf16>::value) {
        const uint32_t x = __float_as_uint(f);
        if ((x & 0x7fffffffu) > 0x7f800000u) return (x >> 16) | 0x0040u;
        return (x + 0x7fffu + ((x >> 16) & 1u)) >> 16;
    } else {
        const f16 h = (f16)f;
        uint16_t b;
        __builtin_memcpy(&b, &h, 2);
        return b;
    }
}

// ---------------------------------------------------------------------------
// k_set_values -- tval: the plan's value array, 8 16-bit words per entry group (ks_tiles::val), n_groups
// groups; src: 8 u32 per group, the index into `values` of the entry each slot holds or kSetNoValue
// (host/device_layout.hpp value_map); values: fp32, in the order of the plan's pattern.
// Destination order: one lane per group loads the group's 8 sources as two 16-byte loads, gathers up
// to 8 floats (a slot without an entry: 0), converts and stores the group's 16 bytes in one store -- no
// 2-byte scattered stores, no atomics; every word of tval is written exactly once, nothing else is.
// 256-thread workgroups, grid-stride over the groups (the launch caps the grid, as combine_parts does).
// Per group 32 B of map and at most 32 B of gathered values are read and 16 B written.
// ---------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void k_set_values(uint16_t *__restrict__ tval, const uint32_t *__restrict__ src,
                                                    const float *__restrict__ values, uint64_t n_groups) {
    for (uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (uint64_t)gridDim.x * 256) {
        const u32x4 *sp = reinterpret_cast<const u32x4 *>(src + g * 8);
        const u32x4 s[2] = {ld_once(sp), ld_once(sp + 1)};
        u32x4 out;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t i = s[j >> 2][j & 3];
            const float f = i != kSetNoValue ? values[i] : 0.0f;
            const uint32_t w = set_value_bits<T>(f);
            if (j & 1) out[j >> 1] |= w << 16;
            else out[j >> 1] = w;
        }
        *reinterpret_cast<u32x4 *>(tval + g * 8) = out;
    }
}

}  // namespace gsk
