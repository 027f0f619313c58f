// hip_code/nm_mfma_exp.hpp -- experiments build only (measured slower than k_nm_mfma, kept
// opt-in): the K-split 2:4 kernels k_nm_mfma_ks and k_nm_mfma4.  Included only under
// GS_EXPERIMENTS; instantiated by kernels/mfma_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// k_nm_mfma_ks -- the same 2:4 panels (same HBM blocks as k_nm_mfma) with one 64-row
// group per wave, four waves = 256 rows per workgroup and K split over `nsplit`
// workgroups (config C3, N = 128).
// Why: a k_nm_mfma workgroup (128 rows) streams all of B (1.8 MB at N = 128) for its
// 1.0 MB of A, and one CU takes in only ~45-70 GB/s, so B is 64% of every CU's intake
// (C3 runs at 69% of HBM at N = 32 and 40% at N = 128, profiles/r03_n_sweep.json).  Here a
// workgroup owns 256 rows over half of K: B 0.9 MB + A 1.0 MB per CU (-32%).
// One wave per SIMD: each wave holds its 64 x N fp32 tile (4 x CT accumulators, 128
// registers at N = 128, the rest of the 512-register budget for the look-ahead), the A
// blocks of the next 256-column chunk (four k-steps) in registers while it computes the
// current one, and the B chunk is staged through registers by all 256 threads into a
// double-buffered LDS image (b_piece permutation, one raw s_barrier per chunk: global
// loads stay in flight across it).  No cross-wave reduction: every wave owns its rows.
// K split: each wave publishes its fp32 tile (8-B agent-scope stores, its own vmcnt(0),
// then one agent-scope add on its row group's counter); the wave whose add completes the
// count sums the slabs in split order with agent-scope loads and stores C
// (deterministic), then re-arms the counter.
// ---------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(256) void k_nm_mfma_ks(const unsigned char *__restrict__ A,
                                                   const f16 *__restrict__ B, f16 *__restrict__ C, uint32_t K,
                                                   uint32_t S, uint32_t rows, uint32_t row_base, uint32_t nsplit,
                                                   uint32_t ncs, float *__restrict__ slabs,
                                                   uint32_t *__restrict__ arrivals) {
    constexpr uint32_t N = 16 * CT, RB = 32 * CT, UB = 2 * CT;
    constexpr uint32_t szB = kNmKC * RB;
    constexpr uint32_t NTH = 256;
    constexpr uint32_t NBU = szB / 16 / NTH;  // 16-B units of B per thread per chunk
    constexpr uint32_t RPU = NTH / UB;        // B rows between a thread's units
    static_assert(szB % (16 * NTH) == 0 && NTH % UB == 0, "whole B units per thread");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t g = blockIdx.x / nsplit, sp = blockIdx.x - g * nsplit;
    const uint32_t rg = g * 4u + wv;  // this wave's 64-row group
    const uint32_t nch = S / 4u;
    const uint32_t c0 = sp * ncs, ncl = min(nch, c0 + ncs) - c0;  // this workgroup's chunks
    const unsigned char *arow = A + (size_t)rg * S * kNmBlockBytes;
    const unsigned char *bbase = reinterpret_cast<const unsigned char *>(B);
    const uint32_t bk = tid / UB, boff = bk * RB + (tid % UB) * 16u;  // this thread's first unit
    auto bdst = [&](uint32_t i) {
        const uint32_t k = bk + i * RPU, s = tid % UB;
        return k * RB + b_piece<CT>(k, s >> 1) * 32u + (s & 1u) * 16u;
    };
    // the four k-step blocks of chunk c (clamped: past the range re-reads the last)
    auto aload = [&](uint32_t i, u32x4 (&V)[4][4], uint2 (&I)[4]) {
        const uint32_t c = c0 + min(i, ncl - 1u);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const unsigned char *blk = arow + (size_t)(4u * c + q) * kNmBlockBytes;
            I[q] = *reinterpret_cast<const uint2 *>(blk + lane * 8u);
#pragma unroll
            for (int rt = 0; rt < 4; rt++) V[q][rt] = *reinterpret_cast<const u32x4 *>(blk + 512u + rt * 1024u + lane * 16u);
        }
    };
    u32x4 bs[NBU];
    auto bload = [&](uint32_t i) {
        const uint32_t k0 = (c0 + min(i, ncl - 1u)) * kNmKC;
        if (k0 + kNmKC <= K) {
            const unsigned char *src = bbase + (size_t)k0 * RB;
#pragma unroll
            for (uint32_t u = 0; u < NBU; u++) bs[u] = *reinterpret_cast<const u32x4 *>(src + u * RPU * RB + boff);
        } else {
#pragma unroll
            for (uint32_t u = 0; u < NBU; u++) {
                const uint32_t kk = min(k0 + bk + u * RPU, K - 1u);
                bs[u] = *reinterpret_cast<const u32x4 *>(bbase + (size_t)kk * RB + (tid % UB) * 16u);
            }
        }
    };
    auto bstore = [&](uint32_t i) {
        const uint32_t k0 = (c0 + min(i, ncl - 1u)) * kNmKC;
        unsigned char *lb = lds + (i & 1u) * szB;
        if (k0 + kNmKC <= K) {
#pragma unroll
            for (uint32_t u = 0; u < NBU; u++) *reinterpret_cast<u32x4 *>(lb + bdst(u)) = bs[u];
        } else {  // rows past K: zeros
#pragma unroll
            for (uint32_t u = 0; u < NBU; u++) {
                const uint32_t z = k0 + bk + u * RPU < K ? ~0u : 0u;
                *reinterpret_cast<u32x4 *>(lb + bdst(u)) = bs[u] & z;
            }
        }
    };
    f4v acc[4][CT];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    const uint32_t kl0 = 8u * (lane >> 4) + ((lane & 15u) >> 2);
    auto compute = [&](uint32_t i, const u32x4 (&V)[4][4], const uint2 (&I)[4]) {
        const unsigned char *lb = lds + (i & 1u) * szB;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            h8v av[4];
#pragma unroll
            for (int rt = 0; rt < 4; rt++) __builtin_memcpy(&av[rt], &V[q][rt], 16);
            const int ix0 = (int)I[q].x, ix1 = (int)I[q].y;
            const uint32_t kl = 64u * q + kl0;
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                s4v t[4];
#pragma unroll
                for (int h = 0; h < 4; h++) {
                    const uint32_t k = kl + 32u * (h >> 1) + 4u * (h & 1);
                    t[h] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (lds_s4v *)(lb + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));
                }
                h16v b;
                __builtin_memcpy(&b, t, 32);
                acc[0][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av[0], b, acc[0][ct], ix0, 0, 0);
                acc[1][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av[1], b, acc[1][ct], ix0, 0, 1);
                acc[2][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av[2], b, acc[2][ct], ix1, 0, 0);
                acc[3][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av[3], b, acc[3][ct], ix1, 0, 1);
            }
        }
    };
    // LDS stores of this thread done, then a raw barrier (the look-ahead loads stay in flight)
    auto barrier = [&]() {
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
    };
    u32x4 va[4][4], vb[4][4];
    uint2 ia[4], ib[4];
    aload(0, va, ia);
    bload(0);
    bstore(0);
    barrier();
    // chunk i: B of i+1 and A of i+1 in flight while i computes; B of i+1 staged after it
    uint32_t i = 0;
    // (sched_barriers keep the look-ahead loads in front of the MFMAs: the scheduler would
    // otherwise sink them past the compute to shorten register lifetimes)
    for (; i + 1 < ncl; i += 2) {
        bload(i + 1);
        aload(i + 1, vb, ib);
        __builtin_amdgcn_sched_barrier(0);
        compute(i, va, ia);
        __builtin_amdgcn_sched_barrier(0);
        bstore(i + 1);
        barrier();
        bload(i + 2);
        aload(i + 2, va, ia);
        __builtin_amdgcn_sched_barrier(0);
        compute(i + 1, vb, ib);
        __builtin_amdgcn_sched_barrier(0);
        bstore(i + 2);
        barrier();
    }
    if (i < ncl) compute(i, va, ia);
    // the trailing look-ahead loads land in registers only
    const bool live = rg * 64u < rows;
    auto store_tile = [&](const f4v (&v)[4][CT]) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const uint32_t r = rg * 64u + rt * 16u + 4u * (lane >> 4) + e;
                    if (r < rows) C[(size_t)(row_base + r) * N + ct * 16u + (lane & 15u)] = (f16)v[rt][ct][e];
                }
    };
    if (nsplit == 1) {
        if (live) store_tile(acc);
        return;
    }
    if (!live) return;  // a row group past the matrix has no counter traffic
    // K split: this wave's tile -> its slab (8-B agent-scope stores: write-through, and
    // compiler-visible, so the MFMA-result -> store wait states are inserted -- an inline-asm
    // 16-B store of the accumulators read one register before the smfmac had written it),
    // then one add
    constexpr uint32_t TI = 4u * CT * 64u;  // f4v per wave tile
    f4v *slab = reinterpret_cast<f4v *>(slabs) + ((size_t)rg * nsplit + sp) * TI;
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            uint64_t *dst = reinterpret_cast<uint64_t *>(slab + (rt * CT + ct) * 64u + lane);
            uint64_t w[2];
            __builtin_memcpy(w, &acc[rt][ct], 16);
            __hip_atomic_store(dst, w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(dst + 1, w[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(&arrivals[rg], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != nsplit - 1u) return;
    if (lane == 0) __hip_atomic_store(&arrivals[rg], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const f4v *base = reinterpret_cast<const f4v *>(slabs) + (size_t)rg * nsplit * TI;
    f4v sum[4][CT];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) sum[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    for (uint32_t qq = 0; qq < nsplit; qq++) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                if (qq == sp) {
                    sum[rt][ct] += acc[rt][ct];
                } else {
                    const uint64_t *src = reinterpret_cast<const uint64_t *>(base + (size_t)qq * TI + (rt * CT + ct) * 64u + lane);
                    uint64_t w[2];
                    w[0] = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    w[1] = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    f4v x;
                    __builtin_memcpy(&x, w, 16);
                    sum[rt][ct] += x;
                }
            }
    }
    store_tile(sum);
}

// ---------------------------------------------------------------------------
// k_nm_mfma4 -- the same 2:4 panels (build_nm_panels blocks) for wide B (N = 128, CT = 8),
// with a quarter of k_nm_mfma's B bytes per row.
// Why: a k_nm_mfma workgroup (128 rows, all of K) takes in 1.8 MB of B for its 1.0 MB of A,
// and one CU's intake is the sum of its A (HBM, ~24 GB/s per CU) and B (L2, ~70 GB/s)
// streams (DESIGN §4 model: 43 + 26 us on C3).  Here a workgroup owns 256 rows (four 64-row
// groups) over one of S K ranges: B per CU halves (0.9 MB at S = 2), A per CU is unchanged,
// the grid stays 224 workgroups on C3.
// Waves: 8 = four row groups x two k-phases; wave (rh, q) takes k-steps 4c+q and 4c+q+2 of
// every 256-row chunk c of its range (its 64 x 128 fp32 tile: 128 accumulator registers).
// B chunks go to LDS by LDS-DMA (global_load_lds_dwordx4: no register staging, no LDS store
// cycles; b_piece's XOR rides on the source address), two 64 KB buffers, one chunk ahead;
// A blocks two chunks ahead in registers.  One barrier per chunk.  Epilogue: the two
// k-phase tiles summed through LDS (q0 + q1), then, with S > 1, the tagged-slab K-split
// combine of k_mfma_ks (ks_slab_wait; sums in K-range order: deterministic).  K must be a
// multiple of 256 (whole chunks; the upload checks).
// ---------------------------------------------------------------------------
template <int CT>
__global__ __launch_bounds__(64 * kNmWaves) void k_nm_mfma4(const unsigned char *__restrict__ A,
                                                            const f16 *__restrict__ B, f16 *__restrict__ C,
                                                            uint32_t K, uint32_t S64, uint32_t rows, uint32_t row_base,
                                                            uint32_t S, uint32_t ncs, uint32_t nwg,
                                                            float *__restrict__ slabs, uint32_t *__restrict__ arrivals,
                                                            uint32_t flags) {
    constexpr uint32_t N = 16 * CT, RB = 32 * CT, UB = 2 * CT;
    constexpr uint32_t HR = kNmKC / 2;                       // B rows of a half chunk (two k-steps)
    constexpr uint32_t szH = HR * RB;                         // one ring slot
    constexpr uint32_t NBW = szH / 16u / (64u * kNmWaves);    // LDS-DMA wave-instructions per wave per half
    static_assert(CT == 8 || CT == 4, "k_nm_mfma4: 64- or 128-column tiles");
    static_assert(4 * szH <= 160u * 1024u, "four ring slots");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t rh = wv >> 1, q = wv & 1u;
    const uint32_t u = xcd_block(blockIdx.x, nwg);
    const uint32_t g = u / S, qs = u - g * S;
    const uint32_t rg = g * 4u + rh;
    const uint32_t nch = S64 / 4u, c0 = qs * ncs, nc = min(ncs, nch - c0);  // this range's chunks
    const uint32_t nh = 2u * nc;                                             // ... and half chunks
    const unsigned char *arow = A + (size_t)rg * S64 * kNmBlockBytes;

    // ---- B half chunk h (k-steps 2h, 2h+1 of the range) -> ring slot h & 3 by LDS-DMA:
    // wave-instruction i of wave wv fills the 1 KB at unit (wv*NBW + i)*64 (lane-linear), rows
    // k = (wv*NBW + i)*RPI + lane/UB of the half; the piece permutation rides on the source
    // address.  b_piece's swizzle of row k depends on i only through bit 3 of k (bit 1 of i at
    // RPI = 4 rows per instruction, CT = 8; bit 0 at RPI = 8, CT = 4): two per-lane offsets
    static_assert(64 % UB == 0, "whole B rows per wave-instruction");
    constexpr uint32_t RPI = 64u / UB;
    auto par_of = [](uint32_t i) -> uint32_t { return RPI == 4 ? (i >> 1) & 1u : i & 1u; };
    auto i0_of = [](uint32_t par) -> uint32_t { return RPI == 4 ? 2u * par : par; };
    uint32_t boff[2];
#pragma unroll
    for (uint32_t par = 0; par < 2; par++) {
        const uint32_t k = (wv * NBW + i0_of(par)) * RPI + lane / UB, sp = lane % UB;
        boff[par] = (k * N + (b_piece<CT>(k, sp >> 1) * 2u + (sp & 1u)) * 8u) * 2u;
    }
    auto issue_b = [&](uint32_t h) {
        const unsigned char *src0 = reinterpret_cast<const unsigned char *>(B) + ((size_t)c0 * kNmKC + (size_t)h * HR) * N * 2u;
        unsigned char *buf = lds + (h & 3u) * szH;
#pragma unroll
        for (uint32_t i = 0; i < NBW; i++) {
            const uint32_t par = par_of(i);
            const uint32_t u0 = (wv * NBW + i) * 64u;
            __builtin_amdgcn_global_load_lds((const void *)(src0 + boff[par] + (i - i0_of(par)) * RPI * N * 2u),
                                             (__attribute__((address_space(3))) void *)(buf + u0 * 16u), 16, 0, 0);
        }
    };
    // ---- A block of half h for this wave: k-step 2h + q of the range (positions + four tiles)
    u32x4 av[3][4];
    uint2 ai[3];
#define GS_NM4_ALOAD(h, V, I)                                                                       \
    {                                                                                             \
        const unsigned char *blk_ = arow + (size_t)(4u * c0 + 2u * (h) + q) * kNmBlockBytes;     \
        const u32x2 i_ = ld_once(reinterpret_cast<const u32x2 *>(blk_ + lane * 8u));              \
        I = make_uint2(i_[0], i_[1]);                                                             \
        _Pragma("unroll") for (int rt = 0; rt < 4; rt++) V[rt] =                                  \
            ld_once(reinterpret_cast<const u32x4 *>(blk_ + 512u + rt * 1024u + lane * 16u));      \
    }
    constexpr int NAL = 5;  // vector loads of one A block
    f4v acc[4][CT];
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    // transposed B reads: row k = 64*q + klane + {0, 4, 32, 36} keeps klane's swizzle bits
    // (k & 3 and bit 3: klane & 7 <= 3, so +4 carries nowhere), so piece ct of row k sits at
    // fb[h] ^ (ct << 5) + 64*q*RB, fb[h] = the row's byte offset + its swizzled piece 0
    const uint32_t klane = 8u * (lane >> 4) + ((lane & 15u) >> 2);
    uint32_t fb[4];
#pragma unroll
    for (int hh = 0; hh < 4; hh++) {
        const uint32_t k = klane + 32u * (hh >> 1) + 4u * (hh & 1);
        fb[hh] = 64u * q * RB + k * RB + b_piece<CT>(k, 0) * 32u + (lane & 3u) * 8u;
    }
#define GS_NM4_BFRAG(lb_, ct, BF)                                                                   \
    {                                                                                             \
        s4v t_[4];                                                                                \
        _Pragma("unroll") for (int hh = 0; hh < 4; hh++)                                          \
            t_[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v *)(lb_ + (fb[hh] ^ ((uint32_t)(ct) << 5)))); \
        __builtin_memcpy(&BF, t_, 32);                                                            \
    }
#define GS_NM4_COMPUTE(h, V, I)                                                                     \
    {                                                                                             \
        const unsigned char *lb_ = lds + ((uint32_t)(h) & 3u) * szH;                              \
        h8v av_[4];                                                                               \
        _Pragma("unroll") for (int rt = 0; rt < 4; rt++) __builtin_memcpy(&av_[rt], &V[rt], 16);  \
        const int ix0_ = (int)I.x, ix1_ = (int)I.y;                                               \
        h16v bf_[2];                                                                              \
        GS_NM4_BFRAG(lb_, 0, bf_[0]);                                                             \
        _Pragma("unroll") for (int ct = 0; ct < CT; ct++) {                                       \
            if (ct + 1 < CT) GS_NM4_BFRAG(lb_, ct + 1, bf_[(ct + 1) & 1]);                        \
            const h16v b_ = bf_[ct & 1];                                                          \
            acc[0][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[0], b_, acc[0][ct], ix0_, 0, 0); \
            acc[1][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[1], b_, acc[1][ct], ix0_, 0, 1); \
            acc[2][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[2], b_, acc[2][ct], ix1_, 0, 0); \
            acc[3][ct] = __builtin_amdgcn_smfmac_f32_16x16x64_f16(av_[3], b_, acc[3][ct], ix1_, 0, 1); \
        }                                                                                         \
    }
    // prologue: B halves 0, 1 and A blocks 0, 1, 2 in flight; half 0 retired (B(1), A(1), A(2)
    // left in flight: NBW + 2 * NAL loads)
    issue_b(0u);
    GS_NM4_ALOAD(0u, av[0], ai[0]);
    issue_b(1u);  // nh >= 2 (a range holds whole chunks)
    GS_NM4_ALOAD(1u, av[1], ai[1]);
    if (nh > 2u) {
        GS_NM4_ALOAD(2u, av[2], ai[2]);
        __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NBW + 2 * NAL) : "memory");
    } else {
        __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NBW + NAL) : "memory");
    }
    __builtin_amdgcn_s_barrier();
    // half iteration h: B(h+2) -> slot (h+2)&3 (read last in h-2, two barriers ago), compute h,
    // A(h+3) into h's register set, retire B(h+1) and A(h+1) (B(h+2), A(h+2), A(h+3) left in
    // flight), barrier.  B is issued two half iterations ahead, A three.
#define GS_NM4_ITER(h, SET)                                                                         \
    {                                                                                             \
        const bool b2_ = (h) + 2u < nh, a3_ = (h) + 3u < nh;                                      \
        if (b2_) issue_b((h) + 2u);                                                               \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        GS_NM4_COMPUTE(h, av[SET], ai[SET]);                                                      \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        if (a3_) GS_NM4_ALOAD((h) + 3u, av[SET], ai[SET]);                                        \
        /* younger than B(h+1) and A(h+1): A(h+2) (if any), B(h+2), A(h+3) */                      \
        if (a3_) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NBW + 2 * NAL) : "memory");         \
        else if (b2_) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NBW + NAL) : "memory");        \
        else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");                                 \
        __builtin_amdgcn_s_barrier();                                                             \
        __builtin_amdgcn_sched_barrier(0);                                                        \
    }
    uint32_t h = 0;
    for (; h + 2u < nh; h += 3u) {
        GS_NM4_ITER(h, 0);
        GS_NM4_ITER(h + 1u, 1);
        GS_NM4_ITER(h + 2u, 2);
    }
    if (h < nh) GS_NM4_ITER(h, 0);
    if (h + 1u < nh) GS_NM4_ITER(h + 1u, 1);
#undef GS_NM4_ITER
#undef GS_NM4_COMPUTE
#undef GS_NM4_BFRAG
#undef GS_NM4_ALOAD
    // ---- K-split ticket (wave 0), then the two k-phase tiles summed in LDS: q1 -> q0
    uint32_t *arr = arrivals + g;
    uint32_t ticket = 0;
    if (S > 1 && wv == 0 && lane == 0) ticket = __hip_atomic_fetch_add(arr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f4v *red = reinterpret_cast<f4v *>(lds);
    constexpr uint32_t TW = 4 * CT * 64;  // f4v per wave tile
    uint32_t *flag = reinterpret_cast<uint32_t *>(lds + 4u * TW * 16u);  // (nm4_lds_bytes: after the tiles)
    if (q == 1u) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) red[rh * TW + (rt * CT + ct) * 64u + lane] = acc[rt][ct];
    }
    if (S > 1 && wv == 0 && lane == 0) *flag = ticket;
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __asm__ volatile("" ::: "memory");
    if (q == 1u) return;
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] += red[rh * TW + (rt * CT + ct) * 64u + lane];
    auto store_c = [&](int rt, int ct, const f4v &v) {
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const uint32_t r = rg * 64u + rt * 16u + 4u * (lane >> 4) + i;
            if (r < rows) C[(size_t)(row_base + r) * N + ct * 16u + (lane & 15u)] = (f16)v[i];
        }
    };
    if (S == 1) {
#pragma unroll
        for (int rt = 0; rt < 4; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) store_c(rt, ct, acc[rt][ct]);
        return;
    }
    // ---- tagged-slab combine (k_mfma_ks's protocol): slab of unit u = [rh][rt][ct][lane] f4v
    const uint32_t tk = *flag & 0xffffu, tag = ((*flag >> 16) & 1u) ^ 1u;
    auto tagged = [&](const f4v &v) {
        u32x4 w;
        __builtin_memcpy(&w, &v, 16);
        w[0] = (w[0] & ~1u) | tag; w[1] = (w[1] & ~1u) | tag; w[2] = (w[2] & ~1u) | tag; w[3] = (w[3] & ~1u) | tag;
        return w;
    };
    f4v *slab = reinterpret_cast<f4v *>(slabs) + (size_t)u * 4u * TW + rh * TW;
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const u32x4 w = tagged(acc[rt][ct]);
            __asm__ volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(slab + (rt * CT + ct) * 64u + lane), "v"(w) : "memory");
        }
    if (tk != S - 1u) return;
    if (wv == 0 && lane == 0) __hip_atomic_store(arr, tag << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t *err = arrivals + nwg / S;  // the replica's device error word
#pragma unroll
    for (int rt = 0; rt < 4; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            f4v sum = {0.f, 0.f, 0.f, 0.f};
            for (uint32_t qq = 0; qq < S; qq++) {
                u32x4 w;
                if (qq == qs) {
                    w = tagged(acc[rt][ct]);
                } else {
                    const f4v *src = reinterpret_cast<const f4v *>(slabs) + (size_t)(g * S + qq) * 4u * TW + rh * TW +
                                     (rt * CT + ct) * 64u + lane;
                    w = ks_slab_wait(reinterpret_cast<const uint32_t *>(src), tag, err, GS_KS_FORCE(flags));
                }
                w[0] &= ~1u; w[1] &= ~1u; w[2] &= ~1u; w[3] &= ~1u;
                f4v x;
                __builtin_memcpy(&x, &w, 16);
                sum += x;
            }
            store_c(rt, ct, sum);
        }
}

}  // namespace gsk
