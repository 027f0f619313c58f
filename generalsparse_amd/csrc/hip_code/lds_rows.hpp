// hip_code/lds_rows.hpp -- K4 with B chunks staged in LDS, one workgroup per BMTB: k_lds_rows,
// k_lds_rows_dma and k_lds_rows_rs, with their helpers (fma_mix, fma_row_mix, static_for,
// lds_dma16).  Instantiated by kernels/gather_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// v_fma_mix_f32: fp32 += fp16 * fp16 with the conversions folded into the FMA
// (no v_cvt_f32_f16).  VS/BS select the low (0) or high (1) half of the packed
// operand.
// ---------------------------------------------------------------------------
template <int VS, int BS>
__device__ __forceinline__ float fma_mix(uint32_t v_h2, uint32_t b_h2, float c) {
    float d;
    if constexpr (VS == 0 && BS == 0)
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,0,0] op_sel_hi:[1,1,0]" : "=v"(d) : "v"(v_h2), "v"(b_h2), "v"(c));
    else if constexpr (VS == 0 && BS == 1)
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,0] op_sel_hi:[1,1,0]" : "=v"(d) : "v"(v_h2), "v"(b_h2), "v"(c));
    else if constexpr (VS == 1 && BS == 0)
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,1,0]" : "=v"(d) : "v"(v_h2), "v"(b_h2), "v"(c));
    else
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "=v"(d) : "v"(v_h2), "v"(b_h2), "v"(c));
    return d;
}

// acc[0..CF) += v * b (CF fp16 values packed in b_words), v = half VS of v_word
template <int CF, int VS>
__device__ __forceinline__ void fma_row_mix(float (&acc)[CF], uint32_t v_word, const uint32_t *b_words) {
#pragma unroll
    for (int m = 0; m < CF / 2; m++) {
        acc[2 * m] = fma_mix<VS, 0>(v_word, b_words[m], acc[2 * m]);
        acc[2 * m + 1] = fma_mix<VS, 1>(v_word, b_words[m], acc[2 * m + 1]);
    }
}

// ---------------------------------------------------------------------------
// K4 on an LDS-stationary B (tblock_warp_total plan, MI355X layout):
// workgroup g owns BMTB g (<= rpw_max rows); wave w owns BMW g.first_BMW + w
// (<= MAXR rows).  K is cut into nc chunks of KC columns.  Per chunk the
// workgroup stages
//   * B[kc0 : kc0+KC, 0:N]   -> LDS, rows padded to RSB bytes (bank spread),
//   * the BMTB's A entries whose columns fall in the chunk -> LDS, right after
//     it: [cols u16 | vals].  They are stored chunk-major at upload (tile
//     layout [BMTB][chunk][row][entries], 16-bit chunk-local columns, rows
//     padded to 4 entries, segments to 8), so staging is one contiguous copy,
// with the global loads of chunk j+1 issued into registers before computing
// chunk j and written to LDS after the compute barrier.  Every B-row read of
// the inner loop is then an LDS ds_read_b128 instead of an L1/L2 gather: B
// crosses L2->CU once per workgroup instead of once per nonzero.  Accumulators
// of the wave's rows stay in registers across all chunks.
// ---------------------------------------------------------------------------
// compile-time unrolled loop: the index is a constant in every body, so
// register arrays indexed by it stay in VGPRs (no scratch)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// K split (ksp > 1, LDS_KSPLIT): workgroup u = g * ksp + q walks the chunks [q * ncs, +ncs) of
// BMTB g only, publishes its rows' fp32 partials and the last of the ksp workgroups sums them in q
// order (deterministic) -- for plans with too few BMTBs to fill the CUs (upload rule).
template <class VT, int CF, int MAXR, int MAXU>
__global__ __launch_bounds__(1024) void k_lds_rows(
    const uint32_t *__restrict__ bmtb_first_row,  // n_bmtb+1
    const uint32_t *__restrict__ bmw_of_bmtb,     // n_bmtb+1
    const uint32_t *__restrict__ bmw_first_row,   // n_bmw+1
    const uint32_t *__restrict__ seg_start,       // n_bmtb*nc+1: entry offset of (g, j)
    const uint32_t *__restrict__ seg_row_off,     // n_bmtb*nc*(rpw_max+1): row starts inside (g, j)
    const uint16_t *__restrict__ tcol, const VT *__restrict__ tval, const VT *__restrict__ B, VT *__restrict__ C,
    uint32_t K, uint32_t N, uint32_t X, uint32_t KC, uint32_t nc, uint32_t RSB, uint32_t rpw_max, uint32_t seg_cap,
    uint32_t row_base, uint32_t ksp = 1, uint32_t ncs = 0, float *__restrict__ slabs = nullptr,
    uint32_t *__restrict__ arrivals = nullptr) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    typedef typename raw_vec<CF * sizeof(VT)>::t RB;
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    const uint32_t lane = tid & 63u, wib = tid >> 6;
    const uint32_t xl = lane & (X - 1u), slot = lane / X, S = 64u / X;
    // K split (LDS_KSPLIT): workgroup u = g * ksp + q walks chunks [q * ncs, +ncs) of BMTB g
    const uint32_t g = ksp > 1u ? blockIdx.x / ksp : blockIdx.x, q = ksp > 1u ? blockIdx.x % ksp : 0u;
    const uint32_t j0 = q * (ksp > 1u ? ncs : 0u), j1 = ksp > 1u ? min(nc, j0 + ncs) : nc;
    const uint32_t r_first = bmtb_first_row[g];
    const uint32_t bmw = bmw_of_bmtb[g] + wib;
    uint32_t t0 = 0, nt = 0;
    if (bmw < bmw_of_bmtb[g + 1]) {
        t0 = bmw_first_row[bmw] - r_first;
        nt = bmw_first_row[bmw + 1] - bmw_first_row[bmw];
    }
    const uint32_t UB = X;  // 16-B units per B row (CF * sizeof(VT) == 16)
    const uint32_t lgUB = __builtin_ctz(UB);
    const uint32_t lA = KC * RSB;                        // LDS byte offset of the A segment
    const uint32_t lR = lA + seg_cap * (2u + (uint32_t)sizeof(VT));  // row offsets
    uint32_t *lRp = reinterpret_cast<uint32_t *>(lds + lR);
    const uint32_t c0 = xl * CF;
    const uint32_t cb = c0 * (uint32_t)sizeof(VT);
    const uint32_t ridx = min(tid, rpw_max);

    u32x4 stage[MAXU];  // native vectors (HIP's uint4 is a union struct that defeats SROA)
    uint32_t stage_r;
    uint32_t s_lo = seg_start[g * nc + j0], s_hi = seg_start[g * nc + j0 + 1];

    float acc[MAXR][CF];
#pragma unroll
    for (int t = 0; t < MAXR; t++)
#pragma unroll
        for (int k = 0; k < CF; k++) acc[t][k] = 0.f;

    // issue the global loads of chunk j into registers.  Branch-free: the three
    // source streams are one base per unit picked by a select (B rows, A cols,
    // A vals); units past the end re-read B's first unit.
#define GS_STAGE_LOAD(j, s0, s1)                                                                         \
    {                                                                                                  \
        const uint32_t kc0_ = (j) * KC;                                                                \
        const uint32_t UBt_ = min(KC, K - kc0_) * UB;                                                  \
        const uint32_t len_ = (s1) - (s0);                                                             \
        const uint32_t UAc_ = UBt_ + len_ / 8u, UAe_ = UAc_ + len_ * (uint32_t)sizeof(VT) / 16u;       \
        const unsigned char *pB_ = reinterpret_cast<const unsigned char *>(B + (size_t)kc0_ * N);      \
        const unsigned char *pC_ = reinterpret_cast<const unsigned char *>(tcol + (s0));               \
        const unsigned char *pV_ = reinterpret_cast<const unsigned char *>(tval + (s0));               \
        _Pragma("unroll") for (int I = 0; I < MAXU; I++) {                                             \
            const uint32_t u = tid + I * nthr;                                                         \
            const bool inB = u < UBt_, inC = u < UAc_, live = u < UAe_;                                \
            const unsigned char *base = inB ? static_cast<const unsigned char *>(pB_)                  \
                                      : inC ? static_cast<const unsigned char *>(pC_)                  \
                                      : live ? static_cast<const unsigned char *>(pV_)                 \
                                             : static_cast<const unsigned char *>(pB_);                \
            const uint32_t off = inB ? u : inC ? u - UBt_ : live ? u - UAc_ : 0u;                      \
            stage[I] = *reinterpret_cast<const u32x4 *>(base + (size_t)off * 16u);                     \
        }                                                                                              \
        stage_r = seg_row_off[(size_t)(g * nc + (j)) * (rpw_max + 1) + ridx];                          \
    }

    GS_STAGE_LOAD(j0, s_lo, s_hi);
    for (uint32_t j = j0; j < j1; j++) {
        // registers -> LDS (B rows at RSB stride, A segment contiguous)
        {
            const uint32_t UBt = min(KC, K - j * KC) * UB;
            const uint32_t UAe = UBt + (s_hi - s_lo) * (2u + (uint32_t)sizeof(VT)) / 16u;
#pragma unroll
            for (int I = 0; I < MAXU; I++) {
                const uint32_t u = tid + I * nthr;
                const uint32_t db = (u >> lgUB) * RSB + (u & (UB - 1u)) * 16u;
                const uint32_t da = lA + (u - UBt) * 16u;
                if (u < UAe) *reinterpret_cast<u32x4 *>(lds + (u < UBt ? db : da)) = stage[I];
            }
            if (tid <= rpw_max) lRp[tid] = stage_r;
        }
        __syncthreads();
        const uint32_t len = s_hi - s_lo;
        if (j + 1 < j1) {  // in flight during this chunk's compute
            const uint32_t n_lo = s_hi, n_hi = seg_start[g * nc + j + 2];
            GS_STAGE_LOAD(j + 1, n_lo, n_hi);
            s_lo = n_lo;
            s_hi = n_hi;
        }
        const unsigned char *lAc = lds + lA;
        const unsigned char *lAv = lds + lA + len * 2u;
#pragma unroll
        for (int t = 0; t < MAXR; t++) {
            if ((uint32_t)t < nt) {
                const uint32_t e0 = lRp[t0 + t], e1 = lRp[t0 + t + 1];
                for (uint32_t p0 = e0 + slot * 4u; p0 < e1; p0 += S * 4u) {
                    const uint2 craw = *reinterpret_cast<const uint2 *>(lAc + p0 * 2u);
                    const uint32_t cc[4] = {craw.x & 0xffffu, craw.x >> 16, craw.y & 0xffffu, craw.y >> 16};
                    RB braw[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        // 24-bit LDS byte offsets (KC * RSB <= 160 KB): one v_mad_u32_u24
                        const uint32_t ob = __umul24(cc[q], RSB) + cb;
                        braw[q] = *reinterpret_cast<const RB *>(lds + ob);
                    }
                    if constexpr (sizeof(VT) == 2) {
                        const uint2 vraw = *reinterpret_cast<const uint2 *>(lAv + p0 * 2u);
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            uint32_t bw[CF / 2];
                            __builtin_memcpy(bw, &braw[q], sizeof(RB));
                            const uint32_t vw = (q < 2) ? vraw.x : vraw.y;
                            if (q & 1) fma_row_mix<CF, 1>(acc[t], vw, bw);
                            else fma_row_mix<CF, 0>(acc[t], vw, bw);
                        }
                    } else {
                        const float4 vv = *reinterpret_cast<const float4 *>(lAv + p0 * 4u);
                        const float vq[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            float bt[CF];
                            __builtin_memcpy(bt, &braw[q], sizeof(RB));
#pragma unroll
                            for (int k = 0; k < CF; k++) acc[t][k] = __builtin_fmaf(vq[q], bt[k], acc[t][k]);
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
#undef GS_STAGE_LOAD
#pragma unroll
    for (int t = 0; t < MAXR; t++)
        if ((uint32_t)t < nt) wave_reduce_slots<CF>(acc[t], (int)X);
    if (ksp <= 1u) {
#pragma unroll
        for (int t = 0; t < MAXR; t++)
            if ((uint32_t)t < nt && slot == 0) store_f32<VT, CF>(C + (size_t)(r_first + t0 + t + row_base) * N + c0, acc[t]);
        return;
    }
    // K-split hand-off (k_mfma_ks's drain form, MI355X_MICROARCH.md §Correctness boundaries: sc1
    // stores, every storing wave's vmcnt(0), a barrier, one agent-scope arrival add; the last
    // adder loads the other slabs with sc1 loads): slab (g, q) holds the BMTB's rows x N fp32
    // partials of K range q; the last of the S workgroups sums them in q order (its own from
    // registers: the same bits it stored), so C is the same whichever workgroup arrives last
    const size_t slab_rows = (size_t)rpw_max;
    if (slot == 0) {
#pragma unroll
        for (int t = 0; t < MAXR; t++) {
            if ((uint32_t)t < nt) {
                float *dst = slabs + (((size_t)g * ksp + q) * slab_rows + t0 + t) * N + c0;
#pragma unroll
                for (int k = 0; k < CF; k += 4) {
                    const f4v v = {acc[t][k], acc[t][k + 1], acc[t][k + 2], acc[t][k + 3]};
                    __asm__ volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst + k), "v"(v) : "memory");
                }
            }
        }
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t *flag = lRp;  // the row offsets are no longer read
    if (tid == 0) *flag = __hip_atomic_fetch_add(arrivals + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != ksp - 1u) return;
    if (tid == 0) __hip_atomic_store(arrivals + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot != 0) return;
#pragma unroll
    for (int t = 0; t < MAXR; t++) {
        if ((uint32_t)t < nt) {
            float sum[CF];
#pragma unroll
            for (int k = 0; k < CF; k++) sum[k] = 0.f;
            for (uint32_t qq = 0; qq < ksp; qq++) {
                if (qq == q) {
#pragma unroll
                    for (int k = 0; k < CF; k++) sum[k] += acc[t][k];
                    continue;
                }
                const float *src = slabs + (((size_t)g * ksp + qq) * slab_rows + t0 + t) * N + c0;
#pragma unroll
                for (int k = 0; k < CF; k++) sum[k] += __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            store_f32<VT, CF>(C + (size_t)(r_first + t0 + t + row_base) * N + c0, sum);
        }
    }
}


// ---------------------------------------------------------------------------
// k_lds_rows_dma -- k_lds_rows for fp32 B at N = 32 (LDS_DMA): B rows sit in LDS at 128 B, exactly
// their HBM image, so each chunk's B rows and A segment (u16 columns, fp32 values) go to LDS by
// LDS-DMA (global_load_lds_dwordx4: no register staging, no ds_write phase) into one of two
// buffers: chunk j+1 lands while chunk j is computed, one barrier per chunk.  A wave's row offsets
// in the chunk come from scalar loads.  Same compute loop, K split and slab combine as k_lds_rows;
// entries are in the parity-paired order (conflict-free B reads).
// ---------------------------------------------------------------------------
template <int MAXR>
__global__ __launch_bounds__(1024) void k_lds_rows_dma(
    const uint32_t *__restrict__ bmtb_first_row, const uint32_t *__restrict__ bmw_of_bmtb,
    const uint32_t *__restrict__ bmw_first_row, const uint32_t *__restrict__ seg_start,
    const uint32_t *__restrict__ seg_row_off, const uint16_t *__restrict__ tcol, const float *__restrict__ tval,
    const float *__restrict__ B, float *__restrict__ C, uint32_t K, uint32_t KC, uint32_t nc, uint32_t rpw_max,
    uint32_t seg_cap, uint32_t row_base, uint32_t ksp, uint32_t ncs, float *__restrict__ slabs,
    uint32_t *__restrict__ arrivals) {
    constexpr uint32_t N = 32, CF = 4, X = 8, S = 8, RSB = 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, nwv = nthr >> 6;
    const uint32_t lane = tid & 63u, wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t xl = lane & (X - 1u), slot = lane / X;
    const uint32_t g = ksp > 1u ? blockIdx.x / ksp : blockIdx.x, q = ksp > 1u ? blockIdx.x % ksp : 0u;
    const uint32_t j0 = q * (ksp > 1u ? ncs : 0u), j1 = ksp > 1u ? min(nc, j0 + ncs) : nc;
    const uint32_t r_first = bmtb_first_row[g];
    const uint32_t bmw = bmw_of_bmtb[g] + wib;
    uint32_t t0 = 0, nt = 0;
    if (bmw < bmw_of_bmtb[g + 1]) {
        t0 = bmw_first_row[bmw] - r_first;
        nt = bmw_first_row[bmw + 1] - bmw_first_row[bmw];
    }
    t0 = __builtin_amdgcn_readfirstlane(t0);
    nt = __builtin_amdgcn_readfirstlane(nt);
    // one buffer: B rows [0, KC*128), columns [cap*2), values [cap*4)
    const uint32_t lB = KC * RSB, lV = lB + seg_cap * 2u, szBuf = lV + seg_cap * 4u;
    const uint32_t c0 = xl * CF, cb = c0 * 4u;
    float acc[MAXR][CF];
#pragma unroll
    for (int t = 0; t < MAXR; t++)
#pragma unroll
        for (int k = 0; k < CF; k++) acc[t][k] = 0.f;
    // LDS-DMA of chunk j into buffer b: every wave takes 1 KB blocks (64 lanes x 16 B) of the three
    // contiguous source ranges in turn; lanes past a range's end are masked off
    auto issue = [&](uint32_t j, uint32_t b) {
        unsigned char *dst = lds + b * szBuf;
        const uint32_t kc0 = j * KC, rows = min(KC, K - kc0);
        const uint32_t s0 = seg_start[g * nc + j], len = seg_start[g * nc + j + 1] - s0;
        const unsigned char *srcs[3] = {reinterpret_cast<const unsigned char *>(B + (size_t)kc0 * N),
                                        reinterpret_cast<const unsigned char *>(tcol + s0),
                                        reinterpret_cast<const unsigned char *>(tval + s0)};
        const uint32_t units[3] = {rows * (RSB / 16u), len / 8u, len / 4u};
        const uint32_t dofs[3] = {0u, lB, lV};
#pragma unroll
        for (int r = 0; r < 3; r++) {
            for (uint32_t ib = wib; ib * 64u < units[r]; ib += nwv) {
                const uint32_t u = ib * 64u + lane;
                if (u < units[r])
                    __builtin_amdgcn_global_load_lds((const void *)(srcs[r] + (size_t)u * 16u),
                                                     (__attribute__((address_space(3))) void *)(dst + dofs[r] + ib * 1024u), 16, 0, 0);
            }
        }
    };
    issue(j0, 0u);
    __syncthreads();  // vmcnt(0): chunk j0 landed
    for (uint32_t j = j0; j < j1; j++) {
        const uint32_t b = (j - j0) & 1u;
        if (j + 1 < j1) issue(j + 1, b ^ 1u);  // lands while chunk j is computed
        const unsigned char *lAc = lds + b * szBuf + lB;
        const unsigned char *lAv = lds + b * szBuf + lV;
        const unsigned char *lBb = lds + b * szBuf;
        const uint32_t *ro = seg_row_off + (size_t)(g * nc + j) * (rpw_max + 1) + t0;  // this wave's row offsets
#pragma unroll
        for (int t = 0; t < MAXR; t++) {
            if ((uint32_t)t < nt) {
                const uint32_t e0 = ro[t], e1 = ro[t + 1];
                for (uint32_t p0 = e0 + slot * 4u; p0 < e1; p0 += S * 4u) {
                    const uint2 craw = *reinterpret_cast<const uint2 *>(lAc + p0 * 2u);
                    const uint32_t cc[4] = {craw.x & 0xffffu, craw.x >> 16, craw.y & 0xffffu, craw.y >> 16};
                    uint4 braw[4];
#pragma unroll
                    for (int qq = 0; qq < 4; qq++) braw[qq] = *reinterpret_cast<const uint4 *>(lBb + cc[qq] * RSB + cb);
                    const float4 vv = *reinterpret_cast<const float4 *>(lAv + p0 * 4u);
                    const float vq[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
                    for (int qq = 0; qq < 4; qq++) {
                        float bt[CF];
                        __builtin_memcpy(bt, &braw[qq], 16);
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[t][k] = __builtin_fmaf(vq[qq], bt[k], acc[t][k]);
                    }
                }
            }
        }
        __syncthreads();  // chunk j+1 landed (every wave's vmcnt(0)), chunk j consumed
    }
#pragma unroll
    for (int t = 0; t < MAXR; t++)
        if ((uint32_t)t < nt) wave_reduce_slots<CF>(acc[t], (int)X);
    if (ksp <= 1u) {
#pragma unroll
        for (int t = 0; t < MAXR; t++)
            if ((uint32_t)t < nt && slot == 0) store_f32<float, CF>(C + (size_t)(r_first + t0 + t + row_base) * N + c0, acc[t]);
        return;
    }
    // K-split hand-off: as k_lds_rows (sc1 slab stores, vmcnt(0), barrier, one arrival add)
    const size_t slab_rows = (size_t)rpw_max;
    if (slot == 0) {
#pragma unroll
        for (int t = 0; t < MAXR; t++) {
            if ((uint32_t)t < nt) {
                float *dst = slabs + (((size_t)g * ksp + q) * slab_rows + t0 + t) * N + c0;
                const f4v v = {acc[t][0], acc[t][1], acc[t][2], acc[t][3]};
                __asm__ volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(v) : "memory");
            }
        }
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t *flag = reinterpret_cast<uint32_t *>(lds);
    if (tid == 0) *flag = __hip_atomic_fetch_add(arrivals + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != ksp - 1u) return;
    if (tid == 0) __hip_atomic_store(arrivals + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (slot != 0) return;
#pragma unroll
    for (int t = 0; t < MAXR; t++) {
        if ((uint32_t)t < nt) {
            float sum[CF] = {0.f, 0.f, 0.f, 0.f};
            for (uint32_t qq = 0; qq < ksp; qq++) {
                if (qq == q) {
#pragma unroll
                    for (int k = 0; k < CF; k++) sum[k] += acc[t][k];
                    continue;
                }
                const float *src = slabs + (((size_t)g * ksp + qq) * slab_rows + t0 + t) * N + c0;
#pragma unroll
                for (int k = 0; k < CF; k++) sum[k] += __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            store_f32<float, CF>(C + (size_t)(r_first + t0 + t + row_base) * N + c0, sum);
        }
    }
}

// ---------------------------------------------------------------------------
// k_lds_rows_rs -- k_lds_rows_dma with one row per slot (fp32, N = 32, BMWs of 5..8 rows): slot s of
// a wave walks row s of its BMW four entries at a time (its 8 lanes x 16 B cover the row of C), so
// a row's chunk segment costs ceil(len / 4) iterations of the slot instead of ceil(len / 32) of the
// whole wave per row (k_lds_rows_dma: a 72-entry segment runs 3 iterations = 96 slots, 75% used),
// and no cross-slot reduction is left at the end.  Taller BMTBs (64 rows in 8-row BMWs) also cut
// the B rows a CU stages per nonzero.  Bank order (device_plan.hip, rowslot): slots {0, 1, 4, 5}
// take entries of column parity k & 1, slots {2, 3, 6, 7} the opposite, so the ds_read_b128 lane
// groups (slots {0,3} and {1,2} of each half-wave) read rows of opposite parity while both kinds
// last.  A slot's row offsets in the chunk come by vector loads (one per chunk, issued with the
// chunk's DMA).  The columns arrive as LDS byte offsets of their B rows (column x 128, device_plan.hip).
// Same DMA double buffer, K split and slab combine as k_lds_rows_dma.
// The chunks' DMA is issued by inline asm (lds_dma16): with the builtin, hipcc's wait inserter puts a
// vmcnt(0) before every LDS read of the issuing wave (the DMA writes LDS), so each wave would wait
// for its share of chunk j+1 before computing chunk j; the kernel retires the DMA itself with
// vmcnt(0) right before each chunk barrier, the only point where the other buffer changes hands.
// (RS: rows per slot, 1; a template so that every translation unit's copy is one symbol)
// ---------------------------------------------------------------------------
// The asm writes M0, so M0 is on its clobber list: the compiler then keeps no M0 value of its own
// (LDS-DMA builtins, readlane / movrel indices) live across it.  M0 is a reserved register, and hipcc
// warns about any reserved register on a clobber list; that warning is off for this function alone.
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void lds_dma16(const void *src, const unsigned char *dst) {
    const uint32_t la = __builtin_amdgcn_readfirstlane(
        (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned char *)dst);
    __asm__ volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(la) : "memory", "m0");
}
#pragma clang diagnostic pop
template <int RS = 1>
__global__ __launch_bounds__(1024) void k_lds_rows_rs(
    const uint32_t *__restrict__ bmtb_first_row, const uint32_t *__restrict__ bmw_of_bmtb,
    const uint32_t *__restrict__ bmw_first_row, const uint32_t *__restrict__ seg_start,
    const uint32_t *__restrict__ seg_row_off, const uint16_t *__restrict__ tcol, const float *__restrict__ tval,
    const float *__restrict__ B, float *__restrict__ C, uint32_t K, uint32_t KC, uint32_t nc, uint32_t rpw_max,
    uint32_t seg_cap, uint32_t row_base, uint32_t ksp, uint32_t ncs, float *__restrict__ slabs,
    uint32_t *__restrict__ arrivals) {
    constexpr uint32_t N = 32, CF = 4, X = 8, RSB = 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, nwv = nthr >> 6;
    const uint32_t lane = tid & 63u, wib = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t xl = lane & (X - 1u), slot = lane / X;
    const uint32_t g = ksp > 1u ? blockIdx.x / ksp : blockIdx.x, q = ksp > 1u ? blockIdx.x % ksp : 0u;
    const uint32_t j0 = q * (ksp > 1u ? ncs : 0u), j1 = ksp > 1u ? min(nc, j0 + ncs) : nc;
    const uint32_t r_first = bmtb_first_row[g];
    const uint32_t bmw = bmw_of_bmtb[g] + wib;
    uint32_t t0 = 0, nt = 0;
    if (bmw < bmw_of_bmtb[g + 1]) {
        t0 = bmw_first_row[bmw] - r_first;
        nt = bmw_first_row[bmw + 1] - bmw_first_row[bmw];
    }
    t0 = __builtin_amdgcn_readfirstlane(t0);
    nt = __builtin_amdgcn_readfirstlane(nt);
    const bool has_row = slot < nt;
    const uint32_t rl = t0 + (has_row ? slot : 0u);  // this slot's row in the BMTB (rl + 1 <= rpw_max)
    const uint32_t lB = KC * RSB, lV = lB + seg_cap * 2u, szBuf = lV + seg_cap * 4u;
    const uint32_t cb = xl * 16u;
    float acc[CF] = {0.f, 0.f, 0.f, 0.f};
    auto issue = [&](uint32_t j, uint32_t b) {
        unsigned char *dst = lds + b * szBuf;
        const uint32_t kc0 = j * KC, rows = min(KC, K - kc0);
        const uint32_t s0 = seg_start[g * nc + j], len = seg_start[g * nc + j + 1] - s0;
        const unsigned char *srcs[3] = {reinterpret_cast<const unsigned char *>(B + (size_t)kc0 * N),
                                        reinterpret_cast<const unsigned char *>(tcol + s0),
                                        reinterpret_cast<const unsigned char *>(tval + s0)};
        const uint32_t units[3] = {rows * (RSB / 16u), len / 8u, len / 4u};
        const uint32_t dofs[3] = {0u, lB, lV};
#pragma unroll
        for (int r = 0; r < 3; r++) {
            for (uint32_t ib = wib; ib * 64u < units[r]; ib += nwv) {
                const uint32_t u = ib * 64u + lane;
                if (u < units[r]) lds_dma16(srcs[r] + (size_t)u * 16u, dst + dofs[r] + ib * 1024u);
            }
        }
    };
    // the slot's row bounds in chunk j (segment-relative entry indices)
    auto row_off = [&](uint32_t j) {
        const uint32_t *ro = seg_row_off + (size_t)(g * nc + j) * (rpw_max + 1) + rl;
        return make_uint2(ro[0], ro[1]);
    };
    uint2 ro_n = row_off(j0);
    issue(j0, 0u);
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // chunk j0 landed
    for (uint32_t j = j0; j < j1; j++) {
        const uint32_t b = (j - j0) & 1u;
        const uint2 ro = ro_n;
        if (j + 1 < j1) {
            ro_n = row_off(j + 1);
            issue(j + 1, b ^ 1u);  // lands while chunk j is computed
        }
        const unsigned char *lAc = lds + b * szBuf + lB;
        const unsigned char *lAv = lds + b * szBuf + lV;
        const unsigned char *lBb = lds + b * szBuf + cb;
        if (has_row) {
            for (uint32_t p0 = ro.x; p0 < ro.y; p0 += 4u) {
                const uint2 craw = *reinterpret_cast<const uint2 *>(lAc + p0 * 2u);
                const uint32_t cc[4] = {craw.x & 0xffffu, craw.x >> 16, craw.y & 0xffffu, craw.y >> 16};
                uint4 braw[4];
#pragma unroll
                for (int qq = 0; qq < 4; qq++) braw[qq] = *reinterpret_cast<const uint4 *>(lBb + cc[qq]);  // byte offsets
                const float4 vv = *reinterpret_cast<const float4 *>(lAv + p0 * 4u);
                const float vq[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
                for (int qq = 0; qq < 4; qq++) {
                    float bt[CF];
                    __builtin_memcpy(bt, &braw[qq], 16);
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] = __builtin_fmaf(vq[qq], bt[k], acc[k]);
                }
            }
        }
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();  // chunk j+1 landed (every wave's vmcnt(0)), chunk j consumed
    }
    const uint32_t c0 = xl * CF;
    if (ksp <= 1u) {
        if (has_row) store_f32<float, CF>(C + (size_t)(r_first + rl + row_base) * N + c0, acc);
        return;
    }
    // K-split hand-off: as k_lds_rows_dma (sc1 slab stores, vmcnt(0), barrier, one arrival add)
    const size_t slab_rows = (size_t)rpw_max;
    if (has_row) {
        float *dst = slabs + (((size_t)g * ksp + q) * slab_rows + rl) * N + c0;
        const f4v v = {acc[0], acc[1], acc[2], acc[3]};
        __asm__ volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(dst), "v"(v) : "memory");
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t *flag = reinterpret_cast<uint32_t *>(lds);
    if (tid == 0) *flag = __hip_atomic_fetch_add(arrivals + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (*flag != ksp - 1u) return;
    if (tid == 0) __hip_atomic_store(arrivals + g, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!has_row) return;
    float sum[CF] = {0.f, 0.f, 0.f, 0.f};
    for (uint32_t qq = 0; qq < ksp; qq++) {
        if (qq == q) {
#pragma unroll
            for (int k = 0; k < CF; k++) sum[k] += acc[k];
            continue;
        }
        const float *src = slabs + (((size_t)g * ksp + qq) * slab_rows + rl) * N + c0;
#pragma unroll
        for (int k = 0; k < CF; k++) sum[k] += __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    store_f32<float, CF>(C + (size_t)(r_first + rl + row_base) * N + c0, sum);
}

}  // namespace gsk
