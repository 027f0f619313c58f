// hip_code/sddmm.hpp -- k_sddmm_tm: the sampled dense-dense product on token-major operands,
// out[e] = sum over t < n of G[t][row_e] * X[t][col_e] for the entries e of a plan's pattern
// (gs_sddmm: the weight gradient of gs_linear).  Instantiated by kernels/sddmm_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// k_sddmm_tm -- G: n x M, X: n x K, row-major, one row per token (ET: f16 or bf16); the pattern as
// CSR in canonical order (host/sddmm_layout.hpp): rp (M + 1 u32), cols (CI: u16 or u32), ascending
// inside a row, duplicates adjacent; out: nnz fp32.
// At the densities the engine targets the dense tile is computed on the matrix cores and sampled: the
// mirror of k_mfma_ks's dense image.  Workgroup (bx, by) owns the row block of 16 * RT output features
// bx; wave w of it the strip of CS = 16 * CT input features by * W + w.
// Token loop: 32 tokens per chunk.  The chunk of G (32 x 16 RT) is loaded by the workgroup, the chunk
// of X (32 x CS) by its wave, as they lie in memory -- 16-byte loads along the feature index when the
// operand's row stride and base allow them (flags bit 0: G, bit 1: X), else 2-byte loads -- one
// chunk ahead, in registers, and stored into [token][feature] LDS images (sddmm_row_off: conflict-free
// transposed reads).  The reduction index is the token, the images' row, so both MFMA operands are
// read with ds_read_b64_tr_b16: lane l gets feature l & 15, tokens 8 (l >> 4) .. + 7, for A (G^T) and
// B (X) alike; the reads run in uniform control flow (EXEC all ones) on 8-byte aligned addresses of
// 16-byte aligned images.  RT x CT v_mfma_f32_16x16x32 per chunk into fp32 accumulators kept over the
// whole call: no split over tokens, no atomics -- out[e] depends on column row_e of G, column col_e of
// X and n only, and two launches give the same bits.
// Edges by predication: tokens past n, features past M, columns past K are never read from memory and
// are zero in both images.
// Sampling: lane r holds, for row r of the block, the first of its entries inside the wave's strip (a
// lower bound in the row's sorted columns) and the row's end.  Per 16-row tile the accumulators go to LDS
// (row 4 (l >> 4) + reg, column l & 15 per tile, in the wave's X image, dead by then); a half wave
// takes a row, its lanes consecutive entries from that first one while their columns stay inside the
// strip, and stores out[e] with plain 4-byte stores.  Every entry lies in one row block and one strip:
// written exactly once, nothing else is written.
// ---------------------------------------------------------------------------
template <class CI>
__device__ __forceinline__ uint32_t sddmm_lower_bound(const CI *__restrict__ cols, uint32_t b, uint32_t e, uint32_t c) {
    while (b < e) {
        const uint32_t m = b + ((e - b) >> 1);
        if ((uint32_t)cols[m] < c) b = m + 1u;
        else e = m;
    }
    return b;
}

// 8 features [f, f + 8) of token row `row` (null: a token past n) of an operand with F features: one
// 16-byte load (fast: F % 8 == 0 and a 16-byte aligned base, so the piece is whole or absent), else
// 2-byte loads; what is absent is zero
template <class ET>
__device__ __forceinline__ u32x4 sddmm_load8(const ET *__restrict__ row, uint32_t f, uint32_t F, bool fast) {
    u32x4 v = {0u, 0u, 0u, 0u};
    if (!row) return v;
    if (fast) {
        if (f < F) v = *reinterpret_cast<const u32x4 *>(row + f);
    } else {
        const uint16_t *r = reinterpret_cast<const uint16_t *>(row);
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (f + j < F) v[j >> 1] |= (uint32_t)r[f + j] << (16 * (j & 1));
    }
    return v;
}

template <class ET, class CI, int RT, int CT, int W>
__global__ __launch_bounds__(64 * W) void k_sddmm_tm(const ET *__restrict__ G, const ET *__restrict__ X,
                                                      const uint32_t *__restrict__ rp, const CI *__restrict__ cols,
                                                      float *__restrict__ out, uint32_t n, uint32_t M, uint32_t K,
                                                      uint32_t flags) {
    static_assert(RT >= 1 && RT <= 4 && CT >= 1, "a lane per row of the block: 16 * RT <= 64");
    static_assert((32 * 2 * RT) % (64 * W) == 0 || (64 * W) % (32 * 2 * RT) == 0, "G pieces over the workgroup");
    constexpr uint32_t GIMG = sddmm_image_bytes(RT), XIMG = sddmm_image_bytes(CT);
    constexpr uint32_t CS = 16u * CT, SW = CS + 1u;  // strip width; floats per row of the sampling stage
    static_assert(16u * SW * 4u <= XIMG, "the sampling stage reuses the wave's X image");
    constexpr uint32_t GP = (32u * 2u * RT + 64u * W - 1u) / (64u * W);  // G pieces per thread and chunk
    constexpr uint32_t XP = 32u * 2u * CT / 64u;                         // X pieces per lane and chunk
    typedef typename mfma_elem<ET>::frag frag;
    __shared__ __attribute__((aligned(16))) unsigned char lds[GIMG + W * XIMG];

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned char *gimg = lds, *ximg = lds + GIMG + wv * XIMG;
    const uint32_t r0 = blockIdx.x * 16u * RT;                        // first output feature of the block
    const uint64_t c0w = ((uint64_t)blockIdx.y * W + wv) * CS;        // first input feature of the strip
    const uint32_t c0 = c0w < K ? (uint32_t)c0w : K;                  // (a strip past K: empty)
    const uint32_t c1 = K - c0 < CS ? K : c0 + CS;
    const bool gfast = (flags & 1u) != 0u, xfast = (flags & 2u) != 0u;

    f4v acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};

    // a chunk's pieces: piece p of an image 16 T features wide is token p / (2 T), features 8 (p % (2 T)) ..
    u32x4 gr[GP], xr[XP];
    auto load_chunk = [&](uint32_t t0) {
#pragma unroll
        for (uint32_t i = 0; i < GP; i++) {
            const uint32_t p = tid + 64u * W * i, t = p / (2u * RT), s = p % (2u * RT);
            const bool on = p < 32u * 2u * RT && t0 + t < n;
            gr[i] = sddmm_load8<ET>(on ? G + (size_t)(t0 + t) * M : nullptr, r0 + 8u * s, M, gfast);
        }
#pragma unroll
        for (uint32_t i = 0; i < XP; i++) {
            const uint32_t p = lane + 64u * i, t = p / (2u * CT), s = p % (2u * CT);
            xr[i] = sddmm_load8<ET>(t0 + t < n ? X + (size_t)(t0 + t) * K : nullptr, c0 + 8u * s, c1, xfast);
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (uint32_t i = 0; i < GP; i++) {
            const uint32_t p = tid + 64u * W * i, t = p / (2u * RT), s = p % (2u * RT);
            if (p < 32u * 2u * RT) *reinterpret_cast<u32x4 *>(gimg + sddmm_row_off(RT, t) + 16u * s) = gr[i];
        }
#pragma unroll
        for (uint32_t i = 0; i < XP; i++) {
            const uint32_t p = lane + 64u * i, t = p / (2u * CT), s = p % (2u * CT);
            *reinterpret_cast<u32x4 *>(ximg + sddmm_row_off(CT, t) + 16u * s) = xr[i];
        }
    };

    // fragment reads: lane 4 q + p of a 16-lane group supplies row q, features 4 p .. 4 p + 3 of the block
    const uint32_t kb = 8u * (lane >> 4) + ((lane & 15u) >> 2);
    const uint32_t ga[2] = {sddmm_row_off(RT, kb) + (lane & 3u) * 8u, sddmm_row_off(RT, kb + 4u) + (lane & 3u) * 8u};
    const uint32_t xa[2] = {sddmm_row_off(CT, kb) + (lane & 3u) * 8u, sddmm_row_off(CT, kb + 4u) + (lane & 3u) * 8u};

    load_chunk(0);

    // this lane's row of the block: the first of its entries inside the strip (a lower bound in the row's
    // sorted columns; the first chunk's loads are in flight meanwhile) and the row's end
    uint32_t lo = 0, end = 0;
    if (lane < 16u * RT && r0 + lane < M && c0 < c1) {
        end = rp[r0 + lane + 1u];
        lo = sddmm_lower_bound(cols, rp[r0 + lane], end, c0);
    }

    for (uint32_t t0 = 0; t0 < n; t0 += kSddmmChunk) {  // (uniform: every wave runs every chunk)
        store_chunk();
        __syncthreads();  // G's image is whole (X's is the wave's own: LDS runs a wave's operations in order)
        load_chunk(t0 + kSddmmChunk);  // (past n: nothing is read)
        frag av[RT], bv[CT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            s4v t[2];
#pragma unroll
            for (int hh = 0; hh < 2; hh++) t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v *)(gimg + ga[hh] + 32u * rt));
            __builtin_memcpy(&av[rt], t, 16);
        }
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            s4v t[2];
#pragma unroll
            for (int hh = 0; hh < 2; hh++) t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v *)(ximg + xa[hh] + 32u * ct));
            __builtin_memcpy(&bv[ct], t, 16);
        }
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[rt][ct] = mfma_elem<ET>::mfma_16x16x32(av[rt], bv[ct], acc[rt][ct]);
        __syncthreads();  // every wave has read G's image: the next chunk may replace it
    }

    // sampling, one 16-row tile at a time through the wave's stage
    float *stage = reinterpret_cast<float *>(ximg);
    const uint32_t sl = lane & 31u, half = lane >> 5;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
#pragma unroll
        for (int ct = 0; ct < CT; ct++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) stage[(4u * (lane >> 4) + reg) * SW + 16u * ct + (lane & 15u)] = acc[rt][ct][reg];
        // rows 2 i, 2 i + 1 of the tile: a half wave each, its lanes consecutive entries from the row's first
        // inside the strip, for as long as their columns stay below the strip's end
        uint32_t e[8], ee[8], more = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int src = 16 * rt + 2 * i + (int)half;
            e[i] = (uint32_t)__shfl((int)lo, src, 64) + sl;
            ee[i] = (uint32_t)__shfl((int)end, src, 64);
        }
        // the first 32 entries of every run (the loads of the 8 row pairs in flight together) ...
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t c = e[i] < ee[i] ? (uint32_t)cols[e[i]] : c1;
            const bool in = c < c1;
            if (in) out[e[i]] = stage[(2u * i + half) * SW + (c - c0)];
            // (sorted columns: a run goes on past 32 entries only if the half wave's last lane is inside)
            if ((__builtin_amdgcn_ballot_w64(in) >> (32u * half + 31u)) & 1ull) more |= 1u << i;
        }
        // ... and what a run holds beyond them (a wide strip of a dense row, repeated coordinates)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            if (!((more >> i) & 1u)) continue;
            for (uint32_t x = e[i] + 32u; x < ee[i]; x += 32u) {
                const uint32_t c = cols[x];
                if (c >= c1) break;
                out[x] = stage[(2u * i + half) * SW + (c - c0)];
            }
        }
    }
}

}  // namespace gsk
