// sddmm_launch.hip -- launches of k_sddmm_tm (hip_code/sddmm.hpp): the sampled product behind gs_sddmm.
// One object holds the fp16 and the bf16 instantiations (two column types each).
#include "../hip_code/sddmm.hpp"
#include "launch_common.hpp"

namespace gs {

namespace {

template <class ET, class CI>
void launch_sddmm_k(const void *G, const void *X, const uint32_t *rp, const void *cols, float *out, uint32_t n, uint64_t M,
                    uint64_t K, hipStream_t s) {
    constexpr int RT = gsk::kSddmmRT, CT = gsk::kSddmmCT, W = gsk::kSddmmWaves;
    const uint64_t gx = (M + 16u * RT - 1) / (16u * RT), strips = (K + 16u * CT - 1) / (16u * CT), gy = (strips + W - 1) / W;
    GS_CHECK(gx <= 0x7fffffffull && gy <= 65535ull, "k_sddmm_tm: the matrix is outside one grid");
    // 16-byte loads along the feature index: a row stride and a base that are multiples of 16 bytes
    const uint32_t flags = (M % 8 == 0 && (uintptr_t)G % 16 == 0 ? 1u : 0u) | (K % 8 == 0 && (uintptr_t)X % 16 == 0 ? 2u : 0u);
    hipLaunchKernelGGL((gsk::k_sddmm_tm<ET, CI, RT, CT, W>), dim3((uint32_t)gx, (uint32_t)gy), dim3(64 * W), 0, s, (const ET *)G,
                       (const ET *)X, rp, (const CI *)cols, out, n, (uint32_t)M, (uint32_t)K, flags);
    HIP_OK(hipGetLastError());
}

template <class ET>
void launch_sddmm_et(int col_bytes, const void *G, const void *X, const uint32_t *rp, const void *cols, float *out, uint32_t n,
                     uint64_t M, uint64_t K, hipStream_t s) {
    if (col_bytes == 2) launch_sddmm_k<ET, uint16_t>(G, X, rp, cols, out, n, M, K, s);
    else launch_sddmm_k<ET, uint32_t>(G, X, rp, cols, out, n, M, K, s);
}

}  // namespace

void launch_sddmm(int dtype, int col_bytes, const void *G, const void *X, const uint32_t *rp, const void *cols, float *out,
                  uint32_t n, uint64_t M, uint64_t K, hipStream_t s) {
    GS_CHECK(dtype == kF16 || dtype == kBF16, "k_sddmm_tm runs f16 and bf16 operands");
    GS_CHECK((col_bytes == 2 || col_bytes == 4) && n >= 1 && M >= 1 && K >= 1 && M < 0xffffff00ull && K < 0xffffff00ull,
             "k_sddmm_tm: bad geometry");
    if (dtype == kBF16) launch_sddmm_et<gsk::bf16>(col_bytes, G, X, rp, cols, out, n, M, K, s);
    else launch_sddmm_et<gsk::f16>(col_bytes, G, X, rp, cols, out, n, M, K, s);
}

}  // namespace gs
