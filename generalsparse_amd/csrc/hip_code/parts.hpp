// hip_code/parts.hpp -- the element-wise companions of the other families: k_combine_parts
// (parent-indexed sub-matrices), k_add_parts (MP_COL_PARTS), k_finalize_rows (fp32 workspace
// rows), k_epilogue (the epilogue as a post-pass) and k_tm_in / k_tm_out (the transposes around a plan's
// SpMM on gs_linear's three-launch path).  Instantiated by kernels/device_plan.hip
// and kernels/gather_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// rows listed (shared between BMTs, or empty): C = fp16(workspace), workspace
// re-zeroed for the next launch (companion of k_bitmap_segment with ws and of
// k_row_chunks)
// parent-indexed sub-matrices (row_nz_matrix_div_operator): C row r of the divided range is
// the sum, in sub-matrix order, of row r of every scratch output that has a row r
template <class VT>
__global__ __launch_bounds__(256) void k_combine_parts(const VT *const *__restrict__ parts,
                                                       const uint32_t *__restrict__ rows, uint32_t n,
                                                       VT *__restrict__ C, uint64_t total, uint32_t N) {
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        const uint64_t r = e / N;
        float s = 0.f;
        for (uint32_t q = 0; q < n; q++)
            if (r < rows[q]) s += (float)parts[q][e];
        C[e] = (VT)s;
    }
}

// MP_COL_PARTS: C += the fp32 outputs of column partitions 1..n-1, added in partition order
// (deterministic), C rounded once
struct mp_part_outs {
    const float *p[8];
};
template <class VT>
__global__ __launch_bounds__(256) void k_add_parts(VT *__restrict__ C, mp_part_outs parts, uint32_t n, uint64_t total) {
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (uint64_t)gridDim.x * 256) {
        float s = (float)C[e];
        for (uint32_t q = 0; q < n; q++) s += parts.p[q][e];
        C[e] = (VT)s;
    }
}

template <class VT>
__global__ __launch_bounds__(256) void k_finalize_rows(const uint32_t *__restrict__ rows, uint32_t n_rows,
                                                       float *__restrict__ ws, VT *__restrict__ C, uint32_t N) {
    const size_t total = (size_t)n_rows * N;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t idx = (size_t)rows[e / N] * N + e % N;
        C[idx] = (VT)ws[idx];
        ws[idx] = 0.f;
    }
}

// The epilogue as a post-pass, in place on C (total = rows x N elements): what every launch that
// k_mfma_ks does not fuse runs after its last kernel.  acc = float(C) as the family wrote it, so a
// 16-bit plan rounds twice (an fp32 plan gives the fused path's bits).  Grid-stride; vec: 16-byte
// accesses (N * sizeof(VT) a multiple of 16 and C, the residual 16-byte aligned: a piece never
// crosses a row), else one element per item.  Row e / N selects the bias.
template <class VT>
__global__ __launch_bounds__(256) void k_epilogue(VT *__restrict__ C, epilogue epi, uint64_t total, uint32_t N,
                                                  uint32_t vec) {
    constexpr int CF = 16 / (int)sizeof(VT);
    const uint64_t first = (uint64_t)blockIdx.x * 256 + threadIdx.x, stride = (uint64_t)gridDim.x * 256;
    const VT *__restrict__ res = static_cast<const VT *>(epi.residual);
    if (vec) {
        for (uint64_t v = first; v < total / CF; v += stride) {
            const uint64_t e = v * CF, row = e / N;
            float x[CF], r[CF] = {};
            load_f32<VT, CF>(C + e, x);
            if (res) load_f32<VT, CF>(res + e, r);
#pragma unroll
            for (int k = 0; k < CF; k++) x[k] = epilogue_apply(epi, x[k], row, r[k]);
            store_f32<VT, CF>(C + e, x);
        }
        return;
    }
    for (uint64_t e = first; e < total; e += stride)
        C[e] = (VT)epilogue_apply(epi, (float)C[e], e / N, res ? (float)res[e] : 0.f);
}

// The two ends of gs_linear's three-launch path (token-major activations around a plan's ordinary
// SpMM): LDS-tiled transposes, a 32 x 32 tile per 256-thread workgroup (rows of 33 words: the
// column reads are conflict-free), both sides of a tile read and written along their rows.
// k_tm_in: B (K x N) = X^T, X: N x K.  blockIdx.x: the tile along K, blockIdx.y: along N.
template <class VT>
__global__ __launch_bounds__(256) void k_tm_in(const VT *__restrict__ X, VT *__restrict__ B, uint32_t K, uint32_t N) {
    __shared__ VT tile[32][33];  // (the elements move as they are)
    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
    const uint32_t k0 = blockIdx.x * 32u, n0 = blockIdx.y * 32u;
    for (uint32_t r = ty; r < 32u; r += 8u)
        if (n0 + r < N && k0 + tx < K) tile[r][tx] = X[(size_t)(n0 + r) * K + k0 + tx];
    __syncthreads();
    for (uint32_t r = ty; r < 32u; r += 8u)
        if (k0 + r < K && n0 + tx < N) B[(size_t)(k0 + r) * N + n0 + tx] = tile[tx][r];
}

// k_tm_out: Y (N x M) = epilogue(C)^T, C: M x N as the plan's SpMM wrote it (acc = float(C): a 16-bit
// plan rounds twice, as behind k_epilogue); bias[m] per row of C, the residual N x M as Y, read at
// Y's index.  blockIdx.x: the tile along M, blockIdx.y: along N.
template <class VT>
__global__ __launch_bounds__(256) void k_tm_out(const VT *__restrict__ C, VT *__restrict__ Y, epilogue epi, uint32_t M,
                                                uint32_t N) {
    __shared__ float tile[32][33];
    const uint32_t tx = threadIdx.x & 31u, ty = threadIdx.x >> 5;
    const uint32_t m0 = blockIdx.x * 32u, n0 = blockIdx.y * 32u;
    const VT *__restrict__ res = static_cast<const VT *>(epi.residual);
    for (uint32_t r = ty; r < 32u; r += 8u)
        if (m0 + r < M && n0 + tx < N) tile[r][tx] = (float)C[(size_t)(m0 + r) * N + n0 + tx];
    __syncthreads();
    for (uint32_t r = ty; r < 32u; r += 8u)
        if (n0 + r < N && m0 + tx < M) {
            const size_t at = (size_t)(n0 + r) * M + m0 + tx;
            Y[at] = (VT)epilogue_apply(epi, tile[tx][r], m0 + tx, res ? (float)res[at] : 0.f);
        }
}

}  // namespace gsk
