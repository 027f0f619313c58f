// hip_code/nm_mfma.hpp -- k_nm_mfma: 2:4 panels on the sparse matrix cores.  Instantiated by
// kernels/mfma_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// k_nm_mfma -- fixed_interval_col_direction BMTs that are 2:4 panels
//  on the sparse matrix cores:
// v_smfmac_f32_16x16x64_f16 multiplies a 16x64 A tile stored as 16x32 values
// plus 2-bit positions by a dense 64x16 B tile.
//
// Operand layout of the instruction (measured, scripts/probes/probe_smfmac.hip):
// lane l holds A row l%16, dense k [16*(l/16), +16) of the 64-wide k-step as 8
// values (two per aligned group of 4; idx bits [4g+1:4g] / [4g+3:4g+2] = the
// positions of group g's two values, ascending); B lane l holds column l%16,
// k [8*(l/16), +8) in elements 0-7 and k [32 + 8*(l/16), +8) in elements 8-15;
// the accumulator is the 16x16 MFMA layout (column l%16, rows 4*(l/16)+i).
//
// HBM layout (device_plan.hip build_nm_panels): per row group of 64 rows (four
// 16-row tiles) and k-step s a 4608-byte block: [lane] 8 B of positions (u16
// per tile: tiles 0/1 in the low dword, selected by abid 0/1, tiles 2/3 in the
// high dword), then [tile rt][lane] 16 B of values.  Every wave load is one
// coalesced 512 B / 1 KB request; A is read exactly once.
//
// Workgroup = 8 waves = two row groups (128 rows) x four k-phases: wave (rh, q)
// takes k-step 4c+q of every 256-row chunk c of B.  B chunks are staged in LDS
// (two buffers, 32-B pieces XOR-permuted by b_piece so the transposed reads
// are conflict-free) by all 512 threads through registers, one chunk ahead;
// each wave's A blocks are loaded two chunks ahead.  One barrier per chunk;
// sched_barriers keep the phases in issue order so each wait leaves the younger
// prefetches in flight.  The four k-phase partial tiles are summed in a fixed
// order through LDS ((q0 + q2) + (q1 + q3): deterministic) and stored as fp16.
// ---------------------------------------------------------------------------
// kNmWaves, kNmBlockBytes, kNmKC: kernel_consts.hpp

// DBG (diagnostic builds only, GS_NM_DEBUG): 1 = no B loads in the loop, 2 = no A loads,
// 4 = s_memtime phase stamps of waves 0/4 of workgroups 0 and 100, printed, 8 = the transposed B
// fragment reads of odd n-tiles skipped (half the LDS reads; wrong results)
// NG: the dense width in HBM (B and C row length); NG = 8 runs one 16-column tile whose
// columns 8..15 are zeros in LDS and never stored (N = 8, the half-used tile of C3's N sweep)
// TT: 16-row tiles per workgroup (nm_tiles; kernel_consts.hpp nm_wg_block_bytes): the wave set rh
// = 0 takes the first G0 = ceil(TT/2) tiles, rh = 1 the other G1 = TT/2 (TT = 8: two 64-row groups,
// the original layout).  TT = 7 spreads C3's 1,792 tiles over exactly 256 workgroups (one per
// CU) where TT = 8 leaves 32 CUs idle; the guards `rt < G` fold away for the tiles both sets hold.
template <int CT, int DBG = 0, int NG = 16 * CT, bool NT = false, int TT = 8>
__global__ __launch_bounds__(64 * kNmWaves) void k_nm_mfma(const unsigned char *__restrict__ A,
                                                           const f16 *__restrict__ B, f16 *__restrict__ C,
                                                           uint32_t K, uint32_t S, uint32_t rows,
                                                           uint32_t row_base, uint32_t krot = 0) {
    static_assert(NG == 16 * CT || (CT == 1 && NG == 8), "NG: 16*CT, or 8 in one half-used tile");
    static_assert(TT >= 2 && TT <= 8, "2..8 tiles per workgroup");
    constexpr uint32_t G0 = (TT + 1) / 2, G1 = TT / 2;
    constexpr uint32_t N = NG, RB = 32 * CT, UB = 2 * CT;
    constexpr uint32_t RBG = 2 * NG, UBG = RBG / 16;  // B row bytes / 16-B units in HBM
    constexpr uint32_t szB = kNmKC * RB;
    constexpr uint32_t NTH = 64 * kNmWaves;
    constexpr uint32_t NBU = szB / 16 / NTH;  // 16-B units of B per thread per chunk
    constexpr uint32_t RPU = NTH / UB;        // B rows between a thread's units
    static_assert(szB % (16 * NTH) == 0 && NTH % UB == 0, "whole B units per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t rh = wv >> 2, q = wv & 3u;
    const uint32_t G = rh ? G1 : G0;                             // this wave set's tiles
    const uint32_t r0 = blockIdx.x * 16u * TT + rh * 16u * G0;   // its first row
    const uint32_t BB = 512u + 1024u * G;                        // its block bytes per k-step
    const uint32_t nch = S / 4u;
    // chunk order (krot, as in k_mfma_rows): iteration c works on chunk jr(c), every
    // workgroup starting at its own chunk so they do not all pull the same B rows at once
    const uint32_t rot = krot ? blockIdx.x % nch : 0u;
    auto jr = [&](uint32_t c) -> uint32_t { const uint32_t x = c + rot; return x >= nch ? x - nch : x; };
    const unsigned char *arow = A + (size_t)blockIdx.x * S * nm_wg_block_bytes(TT) + (size_t)rh * S * (512u + 1024u * G0);
    const unsigned char *bbase = reinterpret_cast<const unsigned char *>(B);
    const uint32_t bk = tid / UB, boff = bk * RBG + (tid % UB) * 16u;  // this thread's first unit
    const bool bun = tid % UB < UBG;  // the unit exists in HBM (NG = 8: the tile's upper half is zeros)
    // LDS byte offset of unit i (row bk + i*RPU, 16-B unit tid%UB) in either buffer
    auto bdst = [&](uint32_t i) {
        const uint32_t k = bk + i * RPU, s = tid % UB;
        return k * RB + b_piece<CT>(k, s >> 1) * 32u + (s & 1u) * 16u;
    };

    u32x4 a0v[4], a1v[4];
    uint2 a0i, a1i;
#define GS_NM_ALOAD(c, V, I)                                                                        \
    if (DBG != 2 || (uint32_t)(c) < 2u) {                                                         \
        const uint32_t cc_ = jr(min((uint32_t)(c), nch - 1u));                                    \
        const unsigned char *blk_ = arow + (size_t)(4u * cc_ + q) * BB;                           \
        const u32x2 i_ = ld_once_if<NT>(reinterpret_cast<const u32x2 *>(blk_ + lane * 8u));      \
        I = make_uint2(i_[0], i_[1]);                                                             \
        _Pragma("unroll") for (int rt = 0; rt < 4; rt++) if ((uint32_t)rt < G) V[rt] =            \
            ld_once_if<NT>(reinterpret_cast<const u32x4 *>(blk_ + 512u + rt * 1024u + lane * 16u)); \
    }
    u32x4 bs[NBU];
    // whole chunks: one lane offset, uniform bases; the last partial chunk clamps rows
#define GS_NM_BLOAD(c)                                                                              \
    if (DBG != 1 || (uint32_t)(c) < 2u) {                                                         \
        const uint32_t k0_ = jr(min((uint32_t)(c), nch - 1u)) * kNmKC;                            \
        if (k0_ + kNmKC <= K) {                                                                   \
            const unsigned char *src_ = bbase + (size_t)k0_ * RBG;                                \
            _Pragma("unroll") for (uint32_t i = 0; i < NBU; i++) bs[i] =                          \
                bun ? *reinterpret_cast<const u32x4 *>(src_ + i * RPU * RBG + boff) : u32x4{0u, 0u, 0u, 0u}; \
        } else {                                                                                  \
            _Pragma("unroll") for (uint32_t i = 0; i < NBU; i++) {                                \
                const uint32_t kk_ = min(k0_ + bk + i * RPU, K - 1u);                             \
                bs[i] = bun ? *reinterpret_cast<const u32x4 *>(bbase + (size_t)kk_ * RBG + (tid % UB) * 16u) \
                            : u32x4{0u, 0u, 0u, 0u};                                              \
            }                                                                                     \
        }                                                                                         \
    }
#define GS_NM_BSTORE(c)                                                                             \
    {                                                                                             \
        const uint32_t k0_ = jr(min((uint32_t)(c), nch - 1u)) * kNmKC;                            \
        unsigned char *lb_ = lds + ((uint32_t)(c) & 1u) * szB;                                    \
        if (k0_ + kNmKC <= K) {                                                                   \
            _Pragma("unroll") for (uint32_t i = 0; i < NBU; i++)                                  \
                *reinterpret_cast<u32x4 *>(lb_ + bdst(i)) = bs[i];                                \
        } else { /* rows past K: zeros */                                                         \
            _Pragma("unroll") for (uint32_t i = 0; i < NBU; i++) {                                \
                const uint32_t z_ = k0_ + bk + i * RPU < K ? ~0u : 0u;                            \
                *reinterpret_cast<u32x4 *>(lb_ + bdst(i)) = bs[i] & z_;                           \
            }                                                                                     \
        }                                                                                         \
    }
    f4v acc[4][CT];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    // transposed-read offsets of this lane (h = 0..3: k +0/+4/+32/+36 of the step)
    const uint32_t kl = 64u * q + 8u * (lane >> 4) + ((lane & 15u) >> 2);
    // chunk c's k-step for this wave: B rows 64q + [0, 64) of LDS buffer c&1
#define GS_NM_BFRAG(lb_, ct, BF)                                                                    \
    {                                                                                             \
        s4v t_[4];                                                                                \
        _Pragma("unroll") for (int h = 0; h < 4; h++) {                                           \
            const uint32_t k = kl + 32u * (h >> 1) + 4u * (h & 1);                                \
            t_[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(                                      \
                (lds_s4v *)(lb_ + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));         \
        }                                                                                         \
        __builtin_memcpy(&BF, t_, 32);                                                            \
    }
    // B fragments double-buffered in registers: the reads of n-tile ct+1 are in
    // flight while the four smfmac of n-tile ct run.  A wave set with G < 4 tiles runs the
    // smfmac of its missing tiles on whatever their (never loaded) registers hold: no branch
    // splits the issue-ordered region, and those accumulators are never stored
#define GS_NM_COMPUTE(c, V, I)                                                                      \
    {                                                                                             \
        const unsigned char *lb_ = lds + ((uint32_t)(c) & 1u) * szB;                              \
        h8v av_[4];                                                                               \
        _Pragma("unroll") for (int rt = 0; rt < 4; rt++) __builtin_memcpy(&av_[rt], &V[rt], 16);  \
        const int ix0_ = (int)I.x, ix1_ = (int)I.y;                                               \
        h16v bf_[2];                                                                              \
        GS_NM_BFRAG(lb_, 0, bf_[0]);                                                              \
        _Pragma("unroll") for (int ct = 0; ct < CT; ct++) {                                       \
            if (ct + 1 < CT && !(DBG == 8 && ((ct + 1) & 1))) GS_NM_BFRAG(lb_, ct + 1, bf_[(ct + 1) & 1]); \
            const h16v b_ = bf_[ct & 1];                                                          \
            acc[0][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[0], b_, acc[0][ct], ix0_, 0, 0); \
            acc[1][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[1], b_, acc[1][ct], ix0_, 0, 1); \
            acc[2][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[2], b_, acc[2][ct], ix1_, 0, 0); \
            acc[3][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[3], b_, acc[3][ct], ix1_, 0, 1); \
        }                                                                                         \
        /* issue order: reads of n-tile 0, then (reads of ct+1, smfmac of ct) */                  \
        __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                        \
        _Pragma("unroll") for (int ct = 0; ct < CT; ct++) {                                       \
            if (ct + 1 < CT) __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                   \
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                    \
        }                                                                                         \
    }
    // prologue in the loop's steady-state issue order (B of c+1, then A of c+1)
    GS_NM_BLOAD(0u);
    GS_NM_ALOAD(0u, a0v, a0i);
    __builtin_amdgcn_sched_barrier(0);
    GS_NM_BSTORE(0u);
    __builtin_amdgcn_sched_barrier(0);
    GS_NM_BLOAD(nch > 1u ? 1u : 0u);
    __builtin_amdgcn_sched_barrier(0);
    GS_NM_ALOAD(1u, a1v, a1i);
    __syncthreads();
    // iteration c: stage chunk c+1 (its buffer was last read in iteration c-1,
    // before the barrier), fetch B of c+2, compute c, fetch A of c+2
    uint64_t *stl = reinterpret_cast<uint64_t *>(lds + 2 * szB);  // DBG 4 only
#define GS_NM_STAMP(hc, k)                                                                          \
    if constexpr (DBG == 4) {                                                                     \
        if (lane == 0 && (hc) >= 4u && (hc) < 10u) stl[wv * 32u + ((hc) - 4u) * 5u + (k)] = __builtin_amdgcn_s_memtime(); \
    }
    uint32_t c = 0;
    for (; c + 1 < nch; c += 2) {
        GS_NM_BSTORE(c + 1u);
        GS_NM_STAMP(c, 0u);
        __builtin_amdgcn_sched_barrier(0);
        GS_NM_BLOAD(c + 2u < nch ? c + 2u : c + 1u);
        GS_NM_STAMP(c, 1u);
        __builtin_amdgcn_sched_barrier(0);
        GS_NM_COMPUTE(c, a0v, a0i);
        GS_NM_STAMP(c, 2u);
        __builtin_amdgcn_sched_barrier(0);
        GS_NM_ALOAD(c + 2u, a0v, a0i);
        GS_NM_STAMP(c, 3u);
        __syncthreads();
        GS_NM_STAMP(c, 4u);
        GS_NM_BSTORE(c + 2u);  /* past the end: a buffer nobody reads again */
        GS_NM_STAMP(c + 1u, 0u);
        __builtin_amdgcn_sched_barrier(0);
        GS_NM_BLOAD(c + 3u < nch ? c + 3u : c + 1u);
        GS_NM_STAMP(c + 1u, 1u);
        __builtin_amdgcn_sched_barrier(0);
        GS_NM_COMPUTE(c + 1u, a1v, a1i);
        GS_NM_STAMP(c + 1u, 2u);
        __builtin_amdgcn_sched_barrier(0);
        GS_NM_ALOAD(c + 3u, a1v, a1i);
        GS_NM_STAMP(c + 1u, 3u);
        __syncthreads();
        GS_NM_STAMP(c + 1u, 4u);
    }
    if constexpr (DBG == 4) {
        __syncthreads();
        if ((blockIdx.x == 0 || blockIdx.x == 100) && lane == 0 && (wv == 0 || wv == 4)) {
            const uint64_t t0 = stl[wv * 32u];
            for (int hc = 0; hc < 6; hc++)
                printf("wg %u wave %u half %d: bstore %llu bload %llu compute %llu aload %llu barrier %llu\n",
                       blockIdx.x, wv, hc + 4, (unsigned long long)(stl[wv * 32u + hc * 5] - t0),
                       (unsigned long long)(stl[wv * 32u + hc * 5 + 1] - t0), (unsigned long long)(stl[wv * 32u + hc * 5 + 2] - t0),
                       (unsigned long long)(stl[wv * 32u + hc * 5 + 3] - t0), (unsigned long long)(stl[wv * 32u + hc * 5 + 4] - t0));
        }
    }
#undef GS_NM_STAMP
    if (c < nch) GS_NM_COMPUTE(c, a0v, a0i);
#undef GS_NM_COMPUTE
#undef GS_NM_BFRAG
#undef GS_NM_BSTORE
#undef GS_NM_BLOAD
#undef GS_NM_ALOAD
    // fixed-order k-phase reduction: pass 1 q2 -> q0, q3 -> q1; pass 2 q1 -> q0
    __syncthreads();
    f4v *red = reinterpret_cast<f4v *>(lds);
    constexpr uint32_t TW = 4 * CT * 64;  // f4v per wave
    if (q >= 2) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) red[(rh * 2 + (q - 2)) * TW + (rt * CT + ct) * 64 + lane] = acc[rt][ct];
    }
    __syncthreads();
    if (q < 2) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[rt][ct] += red[(rh * 2 + q) * TW + (rt * CT + ct) * 64 + lane];
    }
    __syncthreads();
    if (q == 1) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) red[rh * TW + (rt * CT + ct) * 64 + lane] = acc[rt][ct];
    }
    __syncthreads();
    if (q == 0) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++) {
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                const f4v v = acc[rt][ct] + red[rh * TW + (rt * CT + ct) * 64 + lane];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const uint32_t r = r0 + rt * 16u + 4u * (lane >> 4) + i;
                    if ((uint32_t)rt < G && r < rows && ct * 16u + (lane & 15u) < N)
                        C[(size_t)(row_base + r) * N + ct * 16u + (lane & 15u)] = (f16)v[i];
                }
            }
        }
    }
}

}  // namespace gsk
