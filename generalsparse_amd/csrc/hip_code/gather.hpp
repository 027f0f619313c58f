// hip_code/gather.hpp -- the gather families: k_thread_total (K1), k_warp_rows and k_warp_rows_mc
// (K4), k_block_rows (K6), k_bitmap_segment (K2+K3) and k_row_chunks (K5/K7).  B rows are gathered
// through L1/L2.  Instantiated by kernels/gather_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// K1 thread_total: the row-sorted, col-padded plan (sort_operator +
// fixed_interval_row_direction_thread_blocking_operator(1,...,scf) +
// thread_total_reduce_operator).  BMT b covers sorted row b; X lanes own its
// dense columns; the row's nnz are walked SCF at a time with one vector load
// of cols and one of vals (the reference's Load() of col4/val4,
// total_BMT_result_reduce_to_one_register_token.cc:807-898).  Sorted rows
// b >= n_bmt are the trailing empty rows: their C rows are zero-filled here
// instead of relying on a memset.
// ---------------------------------------------------------------------------
template <class VT, class CT, int CF, int SCF, bool FX>
__device__ __forceinline__ void thread_total_body(const uint32_t *__restrict__ first_nz,  // n_bmt+1
                                                      const idx_formula f_nz,
                                                      const uint32_t *__restrict__ order,     // n_rows: sorted->orig
                                                      const idx_formula f_order,
                                                      const CT *__restrict__ col, const VT *__restrict__ val,
                                                      const VT *__restrict__ B, VT *__restrict__ C, uint32_t n_bmt,
                                                      uint32_t n_rows, uint32_t N, uint32_t X, uint32_t row_base) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t xl = lane & (X - 1u);
    const uint32_t groups_per_block = blockDim.x / X;
    // plain block order: the rows are sorted by length, so XCD-contiguous ranges would
    // give one XCD all the longest rows (measured slower on C1)
    const uint32_t g = blockIdx.x * groups_per_block + threadIdx.x / X;
    const uint32_t stride = gridDim.x * groups_per_block;
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t rr = g; rr < n_rows; rr += stride) {
            float acc[CF];
#pragma unroll
            for (int k = 0; k < CF; k++) acc[k] = 0.f;
            if (rr < n_bmt) {
                uint32_t b, e;
                idx_range<FX>(first_nz, f_nz, rr, b, e);
                typedef typename raw_vec<CF * sizeof(VT)>::t RB;
                for (uint32_t p = b; p < e; p += SCF) {
                    CT cc[SCF];
                    VT vv[SCF];
                    load_raw<CT, SCF>(col + p, cc);
                    load_raw<VT, SCF>(val + p, vv);
                    RB braw[SCF];
#pragma unroll
                    for (int j = 0; j < SCF; j++) braw[j] = *reinterpret_cast<const RB *>(B + (size_t)cc[j] * N + c0);
#pragma unroll
                    for (int j = 0; j < SCF; j++) {
                        VT bt[CF];
                        __builtin_memcpy(bt, &braw[j], sizeof(RB));
                        const float v = (float)vv[j];
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] = __builtin_fmaf(v, (float)bt[k], acc[k]);
                    }
                }
            }
            if (cok) store_f32<VT, CF>(C + (size_t)(idx_at<FX>(order, f_order, rr) + row_base) * N + c0, acc);
        }
    }
}

template <class VT, class CT, int CF, int SCF>
__global__ __launch_bounds__(256) void k_thread_total(const uint32_t *__restrict__ first_nz, const idx_formula f_nz,
                                                      const uint32_t *__restrict__ order, const idx_formula f_order,
                                                      const CT *__restrict__ col, const VT *__restrict__ val,
                                                      const VT *__restrict__ B, VT *__restrict__ C, uint32_t n_bmt,
                                                      uint32_t n_rows, uint32_t N, uint32_t X, uint32_t row_base) {
    if (f_nz.kind == IDX_ARRAY && f_order.kind == IDX_ARRAY)
        thread_total_body<VT, CT, CF, SCF, false>(first_nz, f_nz, order, f_order, col, val, B, C, n_bmt, n_rows, N, X, row_base);
    else
        thread_total_body<VT, CT, CF, SCF, true>(first_nz, f_nz, order, f_order, col, val, B, C, n_bmt, n_rows, N, X, row_base);
}

// ---------------------------------------------------------------------------
// K4 warp_total over BMWs (fixed_interval_row_direction_warp_blocking_operator
// or balanced_interval_row_direction_warp_blocking_operator, optionally inside
// BMTBs) + warp_total_reduce_operator.  One wave per BMW; the BMW's rows are
// processed in order; each row's nnz are split over the S = 64/X slots in
// SCF-aligned chunks (row_ptr is padded so the aligned over-read stays in
// bounds and is masked), then reduced with xor shuffles.  With a BMTB level,
// workgroup g owns BMWs [bmw_of_bmtb[g], bmw_of_bmtb[g+1]) and its waves stride
// over them (keeps a BMTB's rows on one CU / XCD).
// ---------------------------------------------------------------------------
// a gathered B piece, all zero bits unless `keep`: an entry outside its row (the aligned over-read,
// a padding chunk) is masked in its B operand as well as in its value, so that a non-finite B
// value of a column the row does not hold never reaches the row (0 x Inf = NaN)
template <class RB>
__device__ __forceinline__ RB kept_piece(RB r, bool keep) {
    if constexpr (sizeof(RB) < 4) {
        return keep ? r : (RB)0;
    } else {
        uint32_t w[sizeof(RB) / 4];
        __builtin_memcpy(w, &r, sizeof(RB));
        const uint32_t m = keep ? 0xffffffffu : 0u;
#pragma unroll
        for (uint32_t k = 0; k < sizeof(RB) / 4; k++) w[k] &= m;
        __builtin_memcpy(&r, w, sizeof(RB));
        return r;
    }
}

template <class VT, class CT, int CF, int SCF, bool KEEP = true>
__device__ __forceinline__ void wave_row(const uint32_t b, const uint32_t e, const CT *__restrict__ col,
                                         const VT *__restrict__ val, const VT *__restrict__ B, uint32_t N,
                                         uint32_t c0, uint32_t slot, uint32_t S, float (&acc)[CF]) {
    // Slot-owned SCF-entry chunks, SCF-aligned so cols and vals come in one
    // 16-byte load each; entries outside [b, e) (aligned over-read into the
    // neighbouring rows / zero padding, always valid column indices) are
    // masked by zeroing their value and their B piece (kept_piece; KEEP = false,
    // k_warp_rows_mc: the value only), never by a branch, so all SCF B-row
    // gathers of a chunk are in flight together.  The next chunk's A loads are
    // issued before this chunk's gathers (software pipelining).
    typedef typename raw_vec<CF * sizeof(VT)>::t RB;
    const uint32_t a = b & ~(uint32_t)(SCF - 1);
    uint32_t p0 = a + slot * SCF;
    CT cn[SCF];
    VT vn[SCF];
    if (p0 < e) {
        load_raw<CT, SCF>(col + p0, cn);
        load_raw<VT, SCF>(val + p0, vn);
    }
    while (p0 < e) {
        CT cc[SCF];
        VT vv[SCF];
#pragma unroll
        for (int j = 0; j < SCF; j++) { cc[j] = cn[j]; vv[j] = vn[j]; }
        const uint32_t pn = p0 + S * SCF;
        if (pn < e) {
            load_raw<CT, SCF>(col + pn, cn);
            load_raw<VT, SCF>(val + pn, vn);
        }
        RB braw[SCF];
#pragma unroll
        for (int j = 0; j < SCF; j++) braw[j] = *reinterpret_cast<const RB *>(B + (size_t)cc[j] * N + c0);
#pragma unroll
        for (int j = 0; j < SCF; j++) {
            const uint32_t p = p0 + j;
            const float v = (p >= b && p < e) ? (float)vv[j] : 0.f;
            VT bt[CF];
            if constexpr (KEEP) {
                const RB bk = kept_piece(braw[j], p >= b && p < e);
                __builtin_memcpy(bt, &bk, sizeof(RB));
            } else {
                __builtin_memcpy(bt, &braw[j], sizeof(RB));
            }
#pragma unroll
            for (int k = 0; k < CF; k++) acc[k] = __builtin_fmaf(v, (float)bt[k], acc[k]);
        }
        p0 = pn;
    }
}

#ifndef GS_WR_MAXCH  // A/B builds only (make var VAR_FLAGS=...): chunk capacity and waves per SIMD of k_warp_rows_mc
#define GS_WR_MAXCH 3
#endif
#ifndef GS_WR_WPE
#define GS_WR_WPE 4
#endif
constexpr uint32_t kWarpRowsMaxChunks = GS_WR_MAXCH;  // k_warp_rows_mc: SCF-chunks per slot in one grouped pass (WARP_ROWS_CHUNKS)

template <class VT, class CT, int CF, int SCF, bool FX, uint32_t MC = 1>
__device__ __forceinline__ void warp_rows_body(const uint32_t *__restrict__ bmw_first_row,  // n_bmw+1
                                                   const idx_formula f_row,
                                                   const uint32_t *__restrict__ bmw_of_bmtb,    // n_bmtb+1 or null
                                                   const idx_formula f_bmw,                     // kind ARRAY + null: no BMTB level
                                                   const uint32_t *__restrict__ row_ptr,        // rows+1 (CSR)
                                                   const CT *__restrict__ col, const VT *__restrict__ val,
                                                   const VT *__restrict__ B, VT *__restrict__ C, uint32_t n_bmw,
                                                   uint32_t N, uint32_t X, uint32_t row_base, uint32_t G, uint32_t nch) {
    // G slots per row (a power of two <= S): the wave takes S/G consecutive rows of the BMW at
    // a time, so rows much shorter than S*SCF nonzeros do not leave most slots idle (C1: rows
    // of ~37 nonzeros against 128-nonzero wave passes at N = 8)
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t xl = lane & (X - 1u);
    const uint32_t S0 = 64u / X;
    const uint32_t S = G < S0 ? G : S0, RP = S0 / S;
    const uint32_t slot = (lane / X) % S, grp = (lane / X) / S;
    const uint32_t wib = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    uint32_t w_begin, w_end, w_step;
    if (bmw_of_bmtb || f_bmw.kind != IDX_ARRAY) {
        const uint32_t t = xcd_block(blockIdx.x, gridDim.x);
        idx_range<FX>(bmw_of_bmtb, f_bmw, t, w_begin, w_end);
        w_begin += wib;
        w_step = wpb;
    } else {
        w_begin = xcd_block(blockIdx.x, gridDim.x) * wpb + wib;
        w_end = n_bmw;
        w_step = gridDim.x * wpb;
    }
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t w = w_begin; w < w_end; w += w_step) {
            uint32_t r_begin, r_end;
            idx_range<FX>(bmw_first_row, f_row, w, r_begin, r_end);
            if (RP > 1 && r_end - r_begin <= 63u) {
                // grouped passes, software-pipelined: the BMW's row starts in one load (lane i
                // holds row_ptr[r_begin + i]); a pass gives each slot up to nch SCF-chunks of its
                // row at once (all their A loads, then all their B gathers in flight: one gather
                // round trip per pass, not one per chunk), and pass ps+1's chunks are loaded before
                // the gathers of pass ps, so a pass waits on one gather latency, not three
                typedef typename raw_vec<CF * sizeof(VT)>::t RB;
                const uint32_t nr = r_end - r_begin, npass = (nr + RP - 1) / RP;
                const uint32_t rpv = lane <= nr ? row_ptr[r_begin + lane] : 0u;
                auto bounds = [&](uint32_t ps, uint32_t &b, uint32_t &e) {  // rows past the end: b == e
                    const uint32_t i = ps * RP + grp;
                    b = (uint32_t)__shfl((int)rpv, (int)min(i, nr), 64);
                    e = (uint32_t)__shfl((int)rpv, (int)min(i + 1u, nr), 64);
                };
                auto fma_chunk = [&](uint32_t q, uint32_t b, uint32_t e, const VT (&vv)[SCF], const RB (&braw)[SCF],
                                     float (&acc)[CF]) {
#pragma unroll
                    for (int j = 0; j < SCF; j++) {
                        const float v = (q + j >= b && q + j < e) ? (float)vv[j] : 0.f;
                        VT bt[CF];
                        // (k_warp_rows_mc, MC > 1, masks the value only: the selects on the B piece
                        // cost C1 3.9%, DESIGN.md section 3 "Non-finite B on the gather families")
                        if constexpr (MC == 1) {
                            const RB bk = kept_piece(braw[j], q + j >= b && q + j < e);
                            __builtin_memcpy(bt, &bk, sizeof(RB));
                        } else {
                            __builtin_memcpy(bt, &braw[j], sizeof(RB));
                        }
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] = __builtin_fmaf(v, (float)bt[k], acc[k]);
                    }
                };
                auto chunk = [&](uint32_t q, uint32_t b, uint32_t e, const CT (&cc)[SCF], const VT (&vv)[SCF],
                                 float (&acc)[CF]) {
                    RB braw[SCF];
#pragma unroll
                    for (int j = 0; j < SCF; j++) braw[j] = *reinterpret_cast<const RB *>(B + (size_t)cc[j] * N + c0);
                    fma_chunk(q, b, e, vv, braw, acc);
                };
                // chunk c of a pass: entries p + c*S*SCF .. (chunks past the row: column 0, value 0)
                CT cn[MC][SCF];
                VT vn[MC][SCF];
                auto load_pass = [&](uint32_t p, uint32_t e) {
#pragma unroll
                    for (uint32_t c = 0; c < MC; c++) {
                        if (c >= nch) break;
                        const uint32_t q = p + c * S * SCF;
                        if (q < e) {
                            load_raw<CT, SCF>(col + q, cn[c]);
                            load_raw<VT, SCF>(val + q, vn[c]);
                        } else {
#pragma unroll
                            for (int j = 0; j < SCF; j++) { cn[c][j] = (CT)0; vn[c][j] = (VT)0.f; }
                        }
                    }
                };
                uint32_t b, e;
                bounds(0u, b, e);
                uint32_t p = (b & ~(uint32_t)(SCF - 1)) + slot * SCF;
                load_pass(p, e);
                for (uint32_t ps = 0; ps < npass; ps++) {
                    CT cc[MC][SCF];
                    VT vv[MC][SCF];
#pragma unroll
                    for (uint32_t c = 0; c < MC; c++)
#pragma unroll
                        for (int j = 0; j < SCF; j++) { cc[c][j] = cn[c][j]; vv[c][j] = vn[c][j]; }
                    const uint32_t cb = b, ce = e, cp = p;
                    if (ps + 1 < npass) {
                        bounds(ps + 1u, b, e);
                        p = (b & ~(uint32_t)(SCF - 1)) + slot * SCF;
                        load_pass(p, e);
                    }
                    float acc[CF];
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] = 0.f;
                    if (cp < ce) {
                        // every chunk's gathers before any chunk's FMAs
                        RB braw[MC][SCF];
#pragma unroll
                        for (uint32_t c = 0; c < MC; c++) {
                            if (c >= nch) break;
#pragma unroll
                            for (int j = 0; j < SCF; j++)
                                braw[c][j] = *reinterpret_cast<const RB *>(B + (size_t)cc[c][j] * N + c0);
                        }
#pragma unroll
                        for (uint32_t c = 0; c < MC; c++) {
                            if (c >= nch) break;
                            fma_chunk(cp + c * S * SCF, cb, ce, vv[c], braw[c], acc);
                        }
                        for (uint32_t q = cp + nch * S * SCF; q < ce; q += S * SCF) {  // rest of a long row
                            CT cq[SCF];
                            VT vq[SCF];
                            load_raw<CT, SCF>(col + q, cq);
                            load_raw<VT, SCF>(val + q, vq);
                            chunk(q, cb, ce, cq, vq, acc);
                        }
                    }
                    for (uint32_t off = X; off < X * S; off <<= 1) {
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] += __shfl_xor(acc[k], (int)off, 64);
                    }
                    const uint32_t r = r_begin + ps * RP + grp;
                    if (slot == 0 && cok && r < r_end) store_f32<VT, CF>(C + (size_t)(r + row_base) * N + c0, acc);
                }
                continue;
            }
            for (uint32_t r0 = r_begin; r0 < r_end; r0 += RP) {
                const uint32_t r = r0 + grp;
                const bool live = r < r_end;
                float acc[CF];
#pragma unroll
                for (int k = 0; k < CF; k++) acc[k] = 0.f;
                if (live) wave_row<VT, CT, CF, SCF, MC == 1>(row_ptr[r], row_ptr[r + 1], col, val, B, N, c0, slot, S, acc);
                for (uint32_t off = X; off < X * S; off <<= 1) {
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] += __shfl_xor(acc[k], (int)off, 64);
                }
                if (slot == 0 && cok && live) store_f32<VT, CF>(C + (size_t)(r + row_base) * N + c0, acc);
            }
        }
    }
}

template <class VT, class CT, int CF, int SCF, uint32_t MC>
__device__ __forceinline__ void warp_rows_kernel(const uint32_t *__restrict__ bmw_first_row, const idx_formula f_row,
                                                 const uint32_t *__restrict__ bmw_of_bmtb, const idx_formula f_bmw,
                                                 const uint32_t *__restrict__ row_ptr, const CT *__restrict__ col,
                                                 const VT *__restrict__ val, const VT *__restrict__ B, VT *__restrict__ C,
                                                 uint32_t n_bmw, uint32_t N, uint32_t X, uint32_t row_base, uint32_t G,
                                                 uint32_t nch) {
    nch = nch < 1u ? 1u : (nch > MC ? MC : nch);
    if (f_row.kind == IDX_ARRAY && f_bmw.kind == IDX_ARRAY)
        warp_rows_body<VT, CT, CF, SCF, false, MC>(bmw_first_row, f_row, bmw_of_bmtb, f_bmw, row_ptr, col, val, B, C, n_bmw,
                                                   N, X, row_base, G, nch);
    else
        warp_rows_body<VT, CT, CF, SCF, true, MC>(bmw_first_row, f_row, bmw_of_bmtb, f_bmw, row_ptr, col, val, B, C, n_bmw,
                                                  N, X, row_base, G, nch);
}

// one SCF-chunk per slot and pass (registers as the plan needs them)
template <class VT, class CT, int CF, int SCF>
__global__ __launch_bounds__(256) void k_warp_rows(const uint32_t *__restrict__ bmw_first_row, const idx_formula f_row,
                                                   const uint32_t *__restrict__ bmw_of_bmtb, const idx_formula f_bmw,
                                                   const uint32_t *__restrict__ row_ptr, const CT *__restrict__ col,
                                                   const VT *__restrict__ val, const VT *__restrict__ B, VT *__restrict__ C,
                                                   uint32_t n_bmw, uint32_t N, uint32_t X, uint32_t row_base,
                                                   uint32_t G = 64) {
    warp_rows_kernel<VT, CT, CF, SCF, 1>(bmw_first_row, f_row, bmw_of_bmtb, f_bmw, row_ptr, col, val, B, C, n_bmw, N, X,
                                         row_base, G, 1u);
}

// up to kWarpRowsMaxChunks SCF-chunks per slot and pass, at most 128 VGPRs (four waves per SIMD):
// launched for fp32 values, u16 columns and 4-entry chunks of 16-B B pieces (C1: fp32, N = 8), the
// instantiations that fit 128 registers without spilling
template <class VT, class CT, int CF, int SCF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(GS_WR_WPE))) void k_warp_rows_mc(
    const uint32_t *__restrict__ bmw_first_row, const idx_formula f_row, const uint32_t *__restrict__ bmw_of_bmtb,
    const idx_formula f_bmw, const uint32_t *__restrict__ row_ptr, const CT *__restrict__ col, const VT *__restrict__ val,
    const VT *__restrict__ B, VT *__restrict__ C, uint32_t n_bmw, uint32_t N, uint32_t X, uint32_t row_base, uint32_t G,
    uint32_t nch) {
    static_assert(SCF <= 4 && CF * sizeof(VT) <= 16, "k_warp_rows_mc: 4-entry chunks, B pieces of at most 16 B");
    warp_rows_kernel<VT, CT, CF, SCF, kWarpRowsMaxChunks>(bmw_first_row, f_row, bmw_of_bmtb, f_bmw, row_ptr, col, val, B, C,
                                                          n_bmw, N, X, row_base, G, nch);
}

// ---------------------------------------------------------------------------
// K6 tblock_total: one 256-thread workgroup per BMTB (fixed row-direction
// TBLOCK blocking + tblock_total_reduce_operator; the reference reduces every
// row of the BMTB over blockDim.y with __syncthreads,
// total_block_reduce_to_one_register_token.cc:374-480).  Here the BMTB's rows
// are taken in windows of kBrWindow: the 4S slots (X column lanes each) walk the
// window's rows slot-per-row and store the short ones (<= kBrSlot nonzeros)
// directly; medium rows (<= solo) are listed and each taken by one wave (its S
// slots split the row, one xor-shuffle reduction, no barrier); longer rows are
// listed in LDS and then reduced by the whole workgroup (all 4S slots split the
// row, registers, then one LDS round of four wave partials).  Short-row BMTBs
// (balanced_block_total on power-law graphs: hundreds of 1-10 nnz rows) cost three
// barriers per window instead of two per row; a medium row no longer serialises
// its slot's wave (one dependent gather round per 4 nonzeros); long-row BMTBs keep
// the cooperative path.
// ---------------------------------------------------------------------------
constexpr uint32_t kBrWindow = 1024;  // rows per window (the long/medium row lists' capacity)
constexpr uint32_t kBrSlot = 8;       // a row of at most this many nonzeros is one slot's
constexpr uint32_t kBrSolo = 512;     // ... at most this many one wave's (more: the workgroup's)

template <class VT, class CT, int CF, int SCF, bool FX>
__device__ __forceinline__ void block_rows_body(const uint32_t *__restrict__ bmtb_first_row,  // n_bmtb+1
                                                    const idx_formula f_row,
                                                    const uint32_t *__restrict__ row_ptr,
                                                    const CT *__restrict__ col, const VT *__restrict__ val,
                                                    const VT *__restrict__ B, VT *__restrict__ C, uint32_t n_bmtb,
                                                    uint32_t N, uint32_t X, uint32_t row_base,
                                                    float (*part)[64][CF],  // [4][64][CF] in LDS
                                                    uint32_t *long_rows,    // [kBrWindow + 1] in LDS
                                                    uint32_t *med_rows,     // [kBrWindow + 1] in LDS
                                                    uint32_t solo) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    const uint32_t xl = lane & (X - 1u);
    const uint32_t S = 64u / X;
    const uint32_t slot = wib * S + lane / X;  // 0 .. 4S-1
    uint32_t *n_long = long_rows + kBrWindow;
    uint32_t *n_med = med_rows + kBrWindow;
    const uint32_t one = min(solo, kBrSlot);  // slot-per-row bound
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t t = xcd_block(blockIdx.x, gridDim.x); t < n_bmtb; t += gridDim.x) {
            uint32_t r_begin, r_end;
            idx_range<FX>(bmtb_first_row, f_row, t, r_begin, r_end);
            for (uint32_t w0 = r_begin; w0 < r_end; w0 += kBrWindow) {
                const uint32_t w1 = min(r_end, w0 + kBrWindow);
                if (threadIdx.x == 0) {
                    *n_long = 0u;
                    *n_med = 0u;
                }
                __syncthreads();
                // slot-per-row over the window; medium and long rows are listed.  The next
                // row's bounds are loaded before this row's entries (one dependent round trip
                // less per row: a slot walks hundreds of short rows in a 17,864-row BMTB)
                uint32_t rbn = 0, ren = 0;
                if (w0 + slot < w1) {
                    rbn = row_ptr[w0 + slot];
                    ren = row_ptr[w0 + slot + 1];
                }
                for (uint32_t r = w0 + slot; r < w1; r += 4u * S) {
                    const uint32_t rb = rbn, re = ren;
                    if (r + 4u * S < w1) {
                        rbn = row_ptr[r + 4u * S];
                        ren = row_ptr[r + 4u * S + 1];
                    }
                    if (re - rb <= one) {
                        float acc[CF];
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] = 0.f;
                        wave_row<VT, CT, CF, SCF>(rb, re, col, val, B, N, c0, 0u, 1u, acc);
                        if (cok) store_f32<VT, CF>(C + (size_t)(r + row_base) * N + c0, acc);
                    } else if (xl == 0u) {
                        if (re - rb <= solo) med_rows[atomicAdd(n_med, 1u)] = r;
                        else long_rows[atomicAdd(n_long, 1u)] = r;
                    }
                }
                __syncthreads();
                // medium rows: one wave each (its S slots split the row)
                const uint32_t nm = *n_med;
                for (uint32_t i = wib; i < nm; i += 4u) {
                    const uint32_t r = med_rows[i];
                    float acc[CF];
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] = 0.f;
                    wave_row<VT, CT, CF, SCF>(row_ptr[r], row_ptr[r + 1], col, val, B, N, c0, lane / X, S, acc);
                    wave_reduce_slots<CF>(acc, (int)X);
                    if (lane < X && cok) store_f32<VT, CF>(C + (size_t)(r + row_base) * N + c0, acc);
                }
                const uint32_t nl = *n_long;
                for (uint32_t i = 0; i < nl; i++) {  // the window's long rows, the whole workgroup each
                    const uint32_t r = long_rows[i];
                    float acc[CF];
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] = 0.f;
                    wave_row<VT, CT, CF, SCF>(row_ptr[r], row_ptr[r + 1], col, val, B, N, c0, slot, 4 * S, acc);
                    wave_reduce_slots<CF>(acc, (int)X);
                    if (lane < X) {
#pragma unroll
                        for (int k = 0; k < CF; k++) part[wib][lane][k] = acc[k];
                    }
                    __syncthreads();
                    if (wib == 0 && lane < X && cok) {
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] = part[0][lane][k] + part[1][lane][k] + part[2][lane][k] + part[3][lane][k];
                        store_f32<VT, CF>(C + (size_t)(r + row_base) * N + c0, acc);
                    }
                    __syncthreads();
                }
                __syncthreads();  // every thread has read n_long before the next window resets it
            }
        }
    }
}

template <class VT, class CT, int CF, int SCF>
__global__ __launch_bounds__(256) void k_block_rows(const uint32_t *__restrict__ bmtb_first_row, const idx_formula f_row,
                                                    const uint32_t *__restrict__ row_ptr, const CT *__restrict__ col,
                                                    const VT *__restrict__ val, const VT *__restrict__ B, VT *__restrict__ C,
                                                    uint32_t n_bmtb, uint32_t N, uint32_t X, uint32_t row_base,
                                                    uint32_t solo = kBrSolo) {
    __shared__ float part[4][64][CF];
    __shared__ uint32_t long_rows[kBrWindow + 1];
    __shared__ uint32_t med_rows[kBrWindow + 1];
    if (f_row.kind == IDX_ARRAY)
        block_rows_body<VT, CT, CF, SCF, false>(bmtb_first_row, f_row, row_ptr, col, val, B, C, n_bmtb, N, X, row_base, part,
                                                long_rows, med_rows, solo);
    else
        block_rows_body<VT, CT, CF, SCF, true>(bmtb_first_row, f_row, row_ptr, col, val, B, C, n_bmtb, N, X, row_base, part,
                                               long_rows, med_rows, solo);
}

// ---------------------------------------------------------------------------
// K2 + K3 bitmap segments (fixed_interval_nnz_direction_thread_blocking_operator
// (32) + thread_bit_map_operator (+ warp_segment_reduce_operator)).  Slot s of
// wave w walks BMT w*S+s.  Row starts come from the BMT's row-start mask (the
// plan's thread_bit_map without the forced BMW heads, thread_bit_map.cc:45-71),
// segment rows from segment_ptr + segment_empty_row_indices
// (segment_ptr.cc / segment_empty_row_indices.cc).  Segments that start and
// end inside the BMT are complete and stored; the open head/tail partials of
// the wave's slots are merged in slot order through LDS (the K3 segmented
// combine, warp_segment_reduce_token.cc:26-444) and added with one atomic per
// row run.  C must be zeroed first.
// ---------------------------------------------------------------------------
template <class VT, class CT, int CF, int SCF, bool FX>
__device__ __forceinline__ void bitmap_segment_body(const uint32_t *__restrict__ bmt_first_nz,   // n_bmt+1
                                                        const idx_formula f_nz,
                                                        const uint32_t *__restrict__ bmt_first_row,  // n_bmt+1
                                                        const idx_formula f_row,
                                                        const uint64_t *__restrict__ row_start_mask, // n_bmt
                                                        const uint32_t *__restrict__ seg_ptr,        // n_bmt
                                                        const uint32_t *__restrict__ seg_row_off,    // segments
                                                        const CT *__restrict__ col, const VT *__restrict__ val,
                                                        const VT *__restrict__ B, VT *__restrict__ C, uint32_t n_bmt,
                                                        uint32_t N, uint32_t X, uint32_t row_base,
                                                        float *__restrict__ ws,
                                                        uint32_t (*open_row)[64][2]) {  // [4][64][2] in LDS
    // ws != nullptr (fp16 C): rows shared between BMTs accumulate in an fp32
    // workspace (k_finalize_rows rounds them to C once); else atomics go to C.
    // per wave: up to 2 open partials per slot (head, tail), S <= 64
    extern __shared__ float dyn[];  // [4 waves][S slots][2][X lanes][CF]
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wib = threadIdx.x >> 6;
    const uint32_t xl = lane & (X - 1u);
    const uint32_t slot = lane / X;
    const uint32_t S = 64u / X;
    float *my_dyn = dyn + (size_t)wib * S * 2 * X * CF;
    const uint32_t waves_total = gridDim.x * (blockDim.x >> 6);
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t w = xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + wib; w * S < n_bmt; w += waves_total) {
            const uint32_t bt = w * S + slot;
            uint32_t head_row = 0xffffffffu, tail_row = 0xffffffffu;
            float head_acc[CF], acc[CF];
#pragma unroll
            for (int k = 0; k < CF; k++) { acc[k] = 0.f; head_acc[k] = 0.f; }
            if (bt < n_bmt) {
                uint32_t b, e;
                idx_range<FX>(bmt_first_nz, f_nz, bt, b, e);
                const uint64_t mask = row_start_mask[bt];
                const bool next_continues = (bt + 1 < n_bmt) && !(row_start_mask[bt + 1] & 1ull);
                const uint32_t r0 = idx_at<FX>(bmt_first_row, f_row, bt);
                const uint32_t sbase = seg_ptr[bt];
                uint32_t seg = 0, cur_row = r0;
                bool cur_open_head = !(mask & 1ull);
                typedef typename raw_vec<CF * sizeof(VT)>::t RB;
                for (uint32_t p0 = b; p0 < e; p0 += SCF) {
                    CT cc[SCF];
                    VT vv[SCF];
                    load_raw<CT, SCF>(col + p0, cc);
                    load_raw<VT, SCF>(val + p0, vv);
                    RB braw[SCF];  // all gathers of the chunk in flight before any use
#pragma unroll
                    for (int j = 0; j < SCF; j++) braw[j] = *reinterpret_cast<const RB *>(B + (size_t)cc[j] * N + c0);
#pragma unroll
                    for (int j = 0; j < SCF; j++) {
                        const uint32_t i = p0 + j - b;
                        if (i > 0 && ((mask >> i) & 1ull)) {  // a new row starts: flush the current segment
                            if (cur_open_head) {
                                head_row = cur_row;
#pragma unroll
                                for (int k = 0; k < CF; k++) head_acc[k] = acc[k];
                            } else if (cok) {
                                store_f32<VT, CF>(C + (size_t)(cur_row + row_base) * N + c0, acc);
                            }
#pragma unroll
                            for (int k = 0; k < CF; k++) acc[k] = 0.f;
                            seg++;
                            cur_row = r0 + seg_row_off[sbase + seg];
                            cur_open_head = false;
                        }
                        VT bt[CF];
                        __builtin_memcpy(bt, &braw[j], sizeof(RB));
                        const float v = (float)vv[j];
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] = __builtin_fmaf(v, (float)bt[k], acc[k]);
                    }
                }
                // last segment
                if (cur_open_head || next_continues) {
                    if (cur_open_head && !next_continues) {
                        head_row = cur_row;
#pragma unroll
                        for (int k = 0; k < CF; k++) head_acc[k] = acc[k];
                    } else {
                        tail_row = cur_row;  // open at the tail (and maybe at the head too)
                        if (cur_open_head) head_row = 0xffffffffu;
                    }
                } else if (cok) {
                    store_f32<VT, CF>(C + (size_t)(cur_row + row_base) * N + c0, acc);
                }
            }
            // publish open partials: [slot][0] = head, [slot][1] = tail
            if (xl == 0) {
                open_row[wib][slot][0] = head_row;
                open_row[wib][slot][1] = tail_row;
            }
            float *hp = my_dyn + ((size_t)(slot * 2 + 0) * X + xl) * CF;
            float *tp = my_dyn + ((size_t)(slot * 2 + 1) * X + xl) * CF;
#pragma unroll
            for (int k = 0; k < CF; k++) { hp[k] = head_acc[k]; tp[k] = acc[k]; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // slot 0's lanes merge the 2S open partials in order, one atomic per row run
            if (slot == 0 && cok) {
                uint32_t run_row = 0xffffffffu;
                float run[CF];
#pragma unroll
                for (int k = 0; k < CF; k++) run[k] = 0.f;
                for (uint32_t q = 0; q < 2 * S; q++) {
                    const uint32_t r = open_row[wib][q >> 1][q & 1];
                    if (r == 0xffffffffu) continue;
                    const float *src = my_dyn + ((size_t)q * X + xl) * CF;
                    if (r != run_row) {
                        if (run_row != 0xffffffffu) {
                            if (ws) atomic_add_vals<float, CF>(ws + (size_t)(run_row + row_base) * N + c0, run);
                            else if constexpr (!std::is_same<VT, bf16>::value) atomic_add_vals<VT, CF>(C + (size_t)(run_row + row_base) * N + c0, run);
                        }
                        run_row = r;
#pragma unroll
                        for (int k = 0; k < CF; k++) run[k] = src[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < CF; k++) run[k] += src[k];
                    }
                }
                if (run_row != 0xffffffffu) {
                    if (ws) atomic_add_vals<float, CF>(ws + (size_t)(run_row + row_base) * N + c0, run);
                    else if constexpr (!std::is_same<VT, bf16>::value) atomic_add_vals<VT, CF>(C + (size_t)(run_row + row_base) * N + c0, run);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

template <class VT, class CT, int CF, int SCF>
__global__ __launch_bounds__(256) void k_bitmap_segment(const uint32_t *__restrict__ bmt_first_nz, const idx_formula f_nz,
                                                        const uint32_t *__restrict__ bmt_first_row, const idx_formula f_row,
                                                        const uint64_t *__restrict__ row_start_mask,
                                                        const uint32_t *__restrict__ seg_ptr,
                                                        const uint32_t *__restrict__ seg_row_off, const CT *__restrict__ col,
                                                        const VT *__restrict__ val, const VT *__restrict__ B,
                                                        VT *__restrict__ C, uint32_t n_bmt, uint32_t N, uint32_t X,
                                                        uint32_t row_base, float *__restrict__ ws) {
    __shared__ uint32_t open_row[4][64][2];
    if (f_nz.kind == IDX_ARRAY && f_row.kind == IDX_ARRAY)
        bitmap_segment_body<VT, CT, CF, SCF, false>(bmt_first_nz, f_nz, bmt_first_row, f_row, row_start_mask, seg_ptr,
                                                    seg_row_off, col, val, B, C, n_bmt, N, X, row_base, ws, open_row);
    else
        bitmap_segment_body<VT, CT, CF, SCF, true>(bmt_first_nz, f_nz, bmt_first_row, f_row, row_start_mask, seg_ptr,
                                                   seg_row_off, col, val, B, C, n_bmt, N, X, row_base, ws, open_row);
}

// ---------------------------------------------------------------------------
// K5 / K7 on col-direction plans (fixed_interval_col_direction_thread_blocking_
// operator + thread_total_reduce + warp_bit_map_operator / tblock_thread_bit_map_
// operator; token_test.cc:1250-1315, 1515-1582).  Every BMT is a chunk of ONE
// row, so a row is a run of consecutive BMTs.  A wave owns U consecutive BMTs
// and walks them S = 64/X at a time, one BMT per X-lane slot.  Equal-row slots
// are summed by a segmented shuffle tree (the row-equality-guarded __shfl_down
// of warp_bit_map_reduce_token.cc), the run reaching the end of a group is
// carried in registers into the next group, and a row is written once it
// closes: a plain store when the row lies inside the wave's range, fp32 atomics
// into `ws` when a neighbouring wave shares it (k_finalize_rows then rounds
// those rows and writes the empty ones).
// ---------------------------------------------------------------------------
template <class VT, class CT, int CF, int SCF, bool FX>
__device__ __forceinline__ void row_chunks_body(const uint32_t *__restrict__ bmt_nz,   // n_bmt+1
                                                    const idx_formula f_nz,
                                                    const uint32_t *__restrict__ bmt_row,  // n_bmt
                                                    const idx_formula f_row,
                                                    const CT *__restrict__ col, const VT *__restrict__ val,
                                                    const VT *__restrict__ B, VT *__restrict__ C,
                                                    float *__restrict__ ws, uint32_t n_bmt, uint32_t U, uint32_t N,
                                                    uint32_t X, uint32_t row_base, uint32_t ilv = 0,
                                                    const uint32_t *__restrict__ ilv_base = nullptr,
                                                    const uint32_t *__restrict__ ilv_stride = nullptr) {
    // ilv > 0: interleaved storage (interlance_storage_operator, GLOBAL parent): every BMT
    // has ilv nonzeros and the i-th of BMT b sits at b + i * n_bmt, so the slots of a wave
    // read consecutive addresses (total_BMT_result_reduce_to_one_register_token.cc:581-624).
    // ilv_base: interleaved per TBLOCK / WARP parent (modify_col_indices_by_interlance_storage.cc
    // :73-118): the i-th nonzero of BMT b sits at ilv_base[b] + i * ilv_stride[b] = the parent's
    // first nonzero + (b - its first BMT) + i * its BMT count; BMT b keeps its own size
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t xl = lane & (X - 1u);
    const uint32_t slot = lane / X;
    const uint32_t S = 64u / X;
    const uint32_t waves_total = gridDim.x * (blockDim.x >> 6);
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t w = xcd_block(blockIdx.x, gridDim.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); (size_t)w * U < n_bmt;
             w += waves_total) {
            const uint32_t r0 = w * U, r1 = min(r0 + U, n_bmt);
            const uint32_t first_row = idx_at<FX>(bmt_row, f_row, r0), last_row = idx_at<FX>(bmt_row, f_row, r1 - 1);
            const bool head_shared = r0 > 0 && idx_at<FX>(bmt_row, f_row, r0 - 1) == first_row;
            const bool tail_shared = r1 < n_bmt && idx_at<FX>(bmt_row, f_row, r1) == last_row;
            float carry[CF];
#pragma unroll
            for (int k = 0; k < CF; k++) carry[k] = 0.f;
            uint32_t carry_row = 0xffffffffu;
            for (uint32_t g = r0; g < r1; g += S) {
                const uint32_t bt = g + slot;
                const bool valid = bt < r1;
                const uint32_t row = valid ? idx_at<FX>(bmt_row, f_row, bt) : 0xfffffffeu;
                float acc[CF];
#pragma unroll
                for (int k = 0; k < CF; k++) acc[k] = 0.f;
                if (valid) {
                    if (ilv_base) {
                        uint32_t b, e;
                        idx_range<FX>(bmt_nz, f_nz, bt, b, e);
                        const uint32_t q0 = ilv_base[bt], st = ilv_stride[bt];
#pragma unroll 4
                        for (uint32_t i = 0; i < e - b; i++) {
                            const size_t p = (size_t)q0 + (size_t)i * st;
                            fma_row<VT, CF>(acc, (float)val[p], B + (size_t)col[p] * N + c0);
                        }
                    } else if (ilv) {
#pragma unroll 8
                        for (uint32_t i = 0; i < ilv; i++) {
                            const size_t p = (size_t)bt + (size_t)i * n_bmt;
                            fma_row<VT, CF>(acc, (float)val[p], B + (size_t)col[p] * N + c0);
                        }
                    } else {
                        uint32_t b, e;
                        idx_range<FX>(bmt_nz, f_nz, bt, b, e);
                        wave_row<VT, CT, CF, SCF>(b, e, col, val, B, N, c0, 0u, 1u, acc);
                    }
                }
                // segmented suffix sums: the first slot of each run ends with the run total
                for (uint32_t off = 1; off < S; off <<= 1) {
                    const uint32_t rn = __shfl_down(row, off * X, 64);
                    float v[CF];
#pragma unroll
                    for (int k = 0; k < CF; k++) v[k] = __shfl_down(acc[k], off * X, 64);
                    if (slot + off < S && rn == row) {
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] += v[k];
                    }
                }
                const uint32_t rp = __shfl_up(row, X, 64);
                const bool is_head = valid && (slot == 0 || rp != row);
                if (slot == 0 && row == carry_row) {
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] += carry[k];
                }
                const uint32_t nv = min(S, r1 - g);
                const uint32_t lr = __shfl(row, (nv - 1) * X, 64);
                const bool cont = g + S < r1 && idx_at<FX>(bmt_row, f_row, g + S) == lr;
                const unsigned long long hm = __ballot(is_head && row == lr);
                const uint32_t hs = (uint32_t)__builtin_ctzll(hm) / X;
#pragma unroll
                for (int k = 0; k < CF; k++) carry[k] = __shfl(acc[k], hs * X + xl, 64);
                carry_row = cont ? lr : 0xffffffffu;
                if (is_head && !(cont && row == lr) && cok) {
                    const size_t o = (size_t)(row_base + row) * N + cw;
                    if ((row == first_row && head_shared) || (row == last_row && tail_shared))
                        atomic_add_vals<float, CF>(ws + o, acc);
                    else
                        store_f32<VT, CF>(C + o, acc);
                }
            }
        }
    }
}

template <class VT, class CT, int CF, int SCF>
__global__ __launch_bounds__(256) void k_row_chunks(const uint32_t *__restrict__ bmt_nz, const idx_formula f_nz,
                                                    const uint32_t *__restrict__ bmt_row, const idx_formula f_row,
                                                    const CT *__restrict__ col, const VT *__restrict__ val,
                                                    const VT *__restrict__ B, VT *__restrict__ C,
                                                    float *__restrict__ ws, uint32_t n_bmt, uint32_t U, uint32_t N,
                                                    uint32_t X, uint32_t row_base, uint32_t ilv = 0,
                                                    const uint32_t *__restrict__ ilv_base = nullptr,
                                                    const uint32_t *__restrict__ ilv_stride = nullptr) {
    if (f_nz.kind == IDX_ARRAY && f_row.kind == IDX_ARRAY)
        row_chunks_body<VT, CT, CF, SCF, false>(bmt_nz, f_nz, bmt_row, f_row, col, val, B, C, ws, n_bmt, U, N, X, row_base, ilv,
                                                ilv_base, ilv_stride);
    else
        row_chunks_body<VT, CT, CF, SCF, true>(bmt_nz, f_nz, bmt_row, f_row, col, val, B, C, ws, n_bmt, U, N, X, row_base, ilv,
                                               ilv_base, ilv_stride);
}

}  // namespace gsk
