// hip_code/mfma_rows.hpp -- k_mfma_rows: BMTB row blocks on the matrix cores, one workgroup per
// row block.  Instantiated by kernels/mfma_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// BMTB row blocks on the matrix cores (MI355X layout of a tblock/warp/block-
// total plan whose row blocks are dense enough).  Workgroup g owns BMTB g
// (R <= RMAX <= 16*RT rows) and walks K in chunks of KC = 2^LGKC columns.
// 16 waves in three roles, each role its own loop with one barrier per chunk
// (so hipcc's vmcnt analysis of a role sees only that role's loads):
//   compute waves 0-5: v_mfma_f32_16x16x32_f16 over chunk j (A rows by
//     ds_read_b128 from the dense image, B by ds_read_b64_tr_b16, fp32
//     accumulators), then clear the dense image of chunk j+2;
//   B waves 6-9: B rows of chunk j+3 -> registers (three sets), each load
//     next to the LDS store of chunk j+1's rows;
//   entry waves 10-15: compressed entries of chunk j+4 -> registers (four
//     sets: HBM latency is the longest), scatter of chunk j+1's entries
//     (upload layout: per group of 8, [8 x u16 h = row*RS/2 + col, the
//     entry's halfword index in the dense image] in one array and [8 x f16
//     value] in another, so both loads are coalesced and the LDS address is
//     one shift; padding entries write 0 to row R) into its dense image.
// Register set indices are compile-time constants (each role's loop is
// unrolled by its set count).  LDS: two B buffers (row k at k*N*2 bytes, 32-B
// pieces permuted by b_piece() so the transposed reads are conflict-free) and
// three dense images (RMAX+1 rows of RS = 2*KC+32 bytes, conflict-free
// ds_read_b128; row R stays zero and stands in for every MFMA row >= R).  At
// the end the compute waves' partial tiles are summed in a fixed order through
// LDS (deterministic) and rows < R are stored.  A zero of the dense image
// times a non-finite B value gives NaN: the kernel multiplies the row block's
// whole tile.
// ---------------------------------------------------------------------------

// STAMPS (diagnostic build only, gs_debug_mfma_timeline): lane 0 of the first
// compute / B / entry wave records s_memtime at phase boundaries
// NBG (GLDS only): B buffers, the B rows of chunk j + NBG - 1 issued in period j
// WCT: compute waves (the entry waves are the other 16 - WCT - B waves)
// DBG (diagnostic timing builds only, wrong results): 1 no B DMA, 2 no scatter, 4 no compute-wave
// LDS reads or clears, 8 no entry loads
// FLG (round 3, MFMA_FLAGS, LDS-DMA variant only): the roles hand buffers over through three
// LDS counters instead of one workgroup barrier per chunk -- B full (B waves, after the
// chunk's DMA retired), image full (entry waves, after the scatter), chunk consumed (compute
// waves, after their reads and clears); each wave waits (s_sleep polling) only for what
// it consumes, so a role runs ahead of the others by the ring depth
template <int CT, int RT, int LGKC, int MAXA, bool STAMPS = false, int GLDS = 0, int NBG = 3, int WCT = kMfmaCompute,
          int DBG = 0, bool FLG = false>
__global__ __launch_bounds__(64 * kMfmaWaves) void k_mfma_rows(
    const uint32_t *__restrict__ bmtb_first_row,  // n_bmtb+1
    const uint32_t *__restrict__ seg_start,       // n_bmtb*nc+1 (groups)
    const u32x4 *__restrict__ tP,                 // per group: 8 x u16 pos (+1 spare group)
    const u32x4 *__restrict__ tV,                 // per group: 8 x f16 value (+1 spare group)
    const f16 *__restrict__ B, f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t nc, uint32_t RMAX,
    uint32_t row_base, uint32_t nsplit, uint32_t ncs, float *__restrict__ slabs, uint32_t *__restrict__ arrivals,
    uint64_t *__restrict__ stamps = nullptr, uint32_t krot = 0) {
    constexpr uint32_t KC = 1u << LGKC;
    constexpr uint32_t RB = 32 * CT;                  // bytes per LDS B row (N <= 16*CT)
    constexpr uint32_t UB = 2 * CT;                   // 16-B units per B row
    constexpr uint32_t RS = 2 * KC + 32;              // dense image row stride
    constexpr uint32_t NT = 64 * kMfmaWaves;
    constexpr uint32_t WC = WCT;
    constexpr uint32_t BWV = GLDS ? GLDS : kMfmaBWaves;
    constexpr uint32_t NBT = 64 * BWV, NAT = 64 * (kMfmaWaves - WC - BWV);  // B / entry threads
    constexpr uint32_t szB = KC * RB;
    constexpr uint32_t NB = szB / 16 / NBT;           // B units per B thread per chunk
    static_assert(szB % (16 * NBT) == 0, "whole B units per B thread");
    constexpr int MAXS = (int)((KC / 32 + WC - 1) / WC);  // k-steps per compute wave per chunk
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t szD = (RMAX + 1) * RS;
    // register-staged B: two B buffers + three dense images; GLDS (B by LDS-DMA, two
    // chunks ahead): three B buffers + two dense images, each compute wave clearing the
    // k-step columns it read
    constexpr uint32_t NBUF = GLDS ? (uint32_t)NBG : 2u, NDI = GLDS ? 2u : 3u;
    static_assert(!GLDS || NBG >= 3, "LDS-DMA B ring of at least three buffers");
    static_assert(!FLG || (GLDS && !STAMPS), "counter hand-offs: LDS-DMA variant, no stamps");
    const uint32_t oD = NBUF * szB;                   // dense images follow the B buffers
    constexpr uint32_t NAW = kMfmaWaves - WCT - (GLDS ? GLDS : kMfmaBWaves);  // entry waves
    // FLG counters (in the launch's 1 KB tail slack): [0] B chunks full x BWV, [1] images full
    // x NAW, [2] chunks consumed x WC
    uint32_t *flg = reinterpret_cast<uint32_t *>(lds + oD + NDI * ((RMAX + 1) * (2u * KC + 32u)) + 768u);
    auto flg_wait = [&](uint32_t idx, uint32_t target) {
        if constexpr (FLG) {
            while (__builtin_amdgcn_readfirstlane(__hip_atomic_load(flg + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) <
                   target)
                __builtin_amdgcn_s_sleep(1);
            __asm__ volatile("" ::: "memory");
        }
    };
    auto flg_arrive = [&](uint32_t idx) {
        if constexpr (FLG) {
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if ((threadIdx.x & 63u) == 0u) __hip_atomic_fetch_add(flg + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __asm__ volatile("" ::: "memory");
        }
    };
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    const uint32_t role = wv < WC ? 0u : (wv < WC + BWV ? 1u : 2u);  // wave-uniform
    const uint32_t bt = tid - 64 * WC;                // B thread index (role 1)
    const uint32_t at = tid - 64 * (WC + BWV);         // entry thread index (role 2)
    // K-split: workgroup (g, sp) takes chunks [j0, j0 + ncl) of BMTB g
    const uint32_t g = blockIdx.x / nsplit, sp = blockIdx.x % nsplit;
    const uint32_t j0 = sp * ncs, ncl = min(nc, j0 + ncs) - j0;
    const uint32_t r0 = bmtb_first_row[g], R = bmtb_first_row[g + 1] - r0;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    // this BMTB's segment starts, lane t holding chunk t's (nc <= 63, host-checked);
    // GS_SEG takes a local chunk index
    const uint32_t segv = seg_start[g * nc + min(lane, nc)];
#define GS_SEG(j) __builtin_amdgcn_readlane(segv, j0 + (j))
    // chunk order: period j works on chunk jr(j); with krot every workgroup starts at its
    // own chunk (g mod ncl) and wraps, so the 256 workgroups are not all pulling the same
    // B rows from the same L2 channels at once (wave-uniform; the k order of a row block's
    // partial sums changes, the result stays deterministic per plan)
    const uint32_t rot = krot ? g % ncl : 0u;
    auto jr = [&](uint32_t j) -> uint32_t { const uint32_t x = j + rot; return x >= ncl ? x - ncl : x; };
    uint64_t *lst = reinterpret_cast<uint64_t *>(lds + oD + NDI * szD);  // STAMPS only
    // first lane of each role -> slots [21*role, 21*role + 21): 0 start, 1 chunk 0 staged,
    // 2+2j chunk j's work done, 3+2j after its barrier (j < 9); slot 63 end
#define GS_STAMP(i)                                                                               \
    if constexpr (STAMPS) {                                                                       \
        if ((tid == 0 || tid == 64 * WC || tid == 64 * (WC + BWV)) && (i) < 21u)                  \
            lst[(i) + 21u * role] = __builtin_amdgcn_s_memtime();                                 \
    }
    GS_STAMP(0u);

    for (uint32_t u = tid; u < NDI * szD / 16u; u += NT) *reinterpret_cast<u32x4 *>(lds + oD + u * 16u) = zero4;
    if constexpr (FLG) {
        if (tid < 4u) flg[tid] = 0u;
    }

    if (role == 0) {
        // ---------------------------------------------------------------- compute
        f4v acc[RT][CT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
        uint32_t arow[RT];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
            const uint32_t row = 16u * rt + (lane & 15u);
            arow[rt] = (row < R ? row : R) * RS;
        }
        __syncthreads();  // dense images cleared
        GS_STAMP(1u);
        __syncthreads();  // chunk 0 staged
        for (uint32_t j = 0; j < ncl; j++) {
            flg_wait(0, BWV * j);  // chunk j's B rows landed (FLG)
            flg_wait(1, NAW * j);  // ... and its dense image scattered
            const uint32_t kr = min(KC, K - (j0 + jr(j)) * KC);
            const uint32_t nsteps = (kr + 31u) / 32u;
            const unsigned char *la = lds + oD + (j % NDI) * szD;
            const unsigned char *lb = lds + (j % NBUF) * szB;
            // all of this wave's k-steps of the chunk: every fragment read issued
            // before the first MFMA (steps past the chunk's end read step 0 and
            // multiply a zeroed A fragment: no branch around the reads)
            h8v av[MAXS][RT], bv[MAXS][CT];
#pragma unroll
            for (int q = 0; q < MAXS; q++) {
                const uint32_t st = wv + q * WC;
                const uint32_t kb = (st < nsteps ? st : 0u) * 32u + 8u * (lane >> 4);
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
                    av[q][rt] = (DBG & 4) ? h8v{} : *reinterpret_cast<const h8v *>(la + arow[rt] + kb * 2u);
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    s4v t[2];
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const uint32_t k = kb + 4u * h + ((lane & 15u) >> 2);
                        t[h] = (DBG & 4) ? s4v{} : __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s4v *)(lb + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));
                    }
                    __builtin_memcpy(&bv[q][ct], t, 16);
                }
            }
#pragma unroll
            for (int q = 0; q < MAXS; q++) {
                const bool live = wv + q * WC < nsteps;
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    const h8v a = live ? av[q][rt] : h8v{};
#pragma unroll
                    for (int ct = 0; ct < CT; ct++)
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bv[q][ct], acc[rt][ct], 0, 0, 0);
                }
            }
            if constexpr (GLDS) {
                // image j%2 holds chunk j+2 next: clear the k-step columns this wave read
                // (its MFMAs consumed the reads; no other wave reads these columns)
                if (j + 2 < ncl && !(DBG & 4)) {
                    unsigned char *dj = lds + oD + (j & 1u) * szD;
#pragma unroll
                    for (int q = 0; q < MAXS; q++) {
                        const uint32_t st = wv + q * WC;
                        if (st < nsteps)
                            for (uint32_t u = lane; u < R * 4u; u += 64u)
                                *reinterpret_cast<u32x4 *>(dj + (u >> 2) * RS + st * 64u + (u & 3u) * 16u) = zero4;
                    }
                }
            } else if (j + 2 < ncl) {
                for (uint32_t u = tid; u < R * RS / 16u; u += 64u * WC)
                    *reinterpret_cast<u32x4 *>(lds + oD + ((j + 2) % 3u) * szD + u * 16u) = zero4;
            }
            GS_STAMP(2u + 2u * j);
            if constexpr (FLG) flg_arrive(2);  // reads and clears of chunk j done
            else __syncthreads();
            GS_STAMP(3u + 2u * j);
        }
        // partial tiles -> LDS for the fixed-order reduction below
        __syncthreads();
        float *red = reinterpret_cast<float *>(lds);
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++)
                *reinterpret_cast<f4v *>(red + (((wv * RT + rt) * CT + ct) * 64u + lane) * 4u) = acc[rt][ct];
    } else if (role == 1 && GLDS) {
        // ---------------------------------------------------------------- B rows, LDS-DMA
        // global_load_lds_dwordx4: no VGPR round trip, no ds_write transfer cycles.
        // Wave-instruction i of B wave bw fills the 1 KB at unit (bw*NB + i)*64 (the
        // destination is lane-linear); b_piece's permutation rides on the source address
        // (an XOR with a per-row constant: its own inverse).  Period j issues chunk j+2
        // into the buffer period j-1 finished reading and retires chunk j+1 with a
        // counted vmcnt before a raw s_barrier (__syncthreads would drain to vmcnt(0)).
        const uint32_t bw = wv - WC;
        auto issue = [&](uint32_t jl) {
            const uint32_t kc0 = (j0 + jr(jl)) * KC;
#pragma unroll
            for (uint32_t i = 0; i < NB; i++) {
                const uint32_t u0 = (bw * NB + i) * 64u, u = u0 + lane;
                const uint32_t k = u / UB, s = u % UB;
                const uint32_t kk = kc0 + k < K ? kc0 + k : kc0;
                // N < 16*CT (N = 8): the tile's columns past N copy column 0; their outputs are not stored
                const uint32_t cu = (b_piece<CT>(k, s >> 1) * 2u + (s & 1u)) * 8u;
                const f16 *src = B + (size_t)kk * N + (cu < N ? cu : 0u);
                __builtin_amdgcn_global_load_lds(
                    (const void *)src, (__attribute__((address_space(3))) void *)(lds + (jl % NBUF) * szB + u0 * 16u),
                    16, 0, 0);
            }
        };
        for (uint32_t jl = 0; jl + 1 < NBUF && jl < ncl; jl++)
            if (!(DBG & 1)) issue(jl);
        __syncthreads();  // dense images cleared (its vmcnt(0) retires the first chunks)
        GS_STAMP(1u);
        __syncthreads();  // chunk 0 staged
        for (uint32_t j = 0; j < ncl; j++) {
            flg_wait(2, WC * j);  // chunk j-1 consumed: its buffer takes chunk j+NBUF-1 (FLG)
            if (j + NBUF - 1 < ncl) {
                if (!(DBG & 1)) issue(j + NBUF - 1);
                // chunk j+1 retired, chunks j+2 .. j+NBUF-1 left in flight
                // (vmcnt holds at most 63: a larger count waits for more than chunk j+1)
                __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"((NBUF - 2) * NB < 63u ? (NBUF - 2) * NB : 63u) : "memory");
            } else {
                // tail: chunks j+2 .. ncl-1 are in flight
                const uint32_t left = ncl > j + 2 ? ncl - j - 2 : 0u;
                if constexpr (NBUF >= 5) {
                    if (left >= 3) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * NB < 63u ? 3 * NB : 63u) : "memory");
                    else if (left == 2) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB < 63u ? 2 * NB : 63u) : "memory");
                    else if (left == 1) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NB < 63u ? NB : 63u) : "memory");
                    else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else if constexpr (NBUF == 4) {
                    if (left >= 2) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB < 63u ? 2 * NB : 63u) : "memory");
                    else if (left == 1) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NB < 63u ? NB : 63u) : "memory");
                    else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
                } else {
                    if (left >= 1) __asm__ volatile("s_waitcnt vmcnt(%0)" ::"n"(NB < 63u ? NB : 63u) : "memory");
                    else __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
            }
            GS_STAMP(2u + 2u * j);
            if constexpr (FLG) flg_arrive(0);  // chunk j+1 landed
            else __builtin_amdgcn_s_barrier();
            GS_STAMP(3u + 2u * j);
        }
        __syncthreads();
    } else if (role == 1) {
        // ---------------------------------------------------------------- B rows
        u32x4 s0[NB], s1[NB], s2[NB];
#define GS_BLOAD(j, S)                                                                              \
    {                                                                                             \
        const uint32_t kc0_ = (j0 + jr(min((uint32_t)(j), ncl - 1u))) * KC;                      \
        _Pragma("unroll") for (uint32_t i = 0; i < NB; i++) {                                     \
            const uint32_t u = bt + i * NBT;                                                      \
            const uint32_t k = u / UB;                                                            \
            const uint32_t kk = kc0_ + k < K ? kc0_ + k : kc0_;                                   \
            S[i] = *reinterpret_cast<const u32x4 *>(B + (size_t)kk * N + ((u % UB) * 8u < N ? (u % UB) * 8u : 0u)); \
        }                                                                                         \
    }
#define GS_BSTORE_UNIT(jb, S, i)                                                                    \
    {                                                                                             \
        const uint32_t u = bt + (i) * NBT;                                                        \
        const uint32_t k = u / UB, s = u % UB;                                                    \
        *reinterpret_cast<u32x4 *>(lds + ((jb) & 1u) * szB + k * RB + b_piece<CT>(k, s >> 1) * 32u + (s & 1u) * 16u) = S[i]; \
    }
        // chunk j: fetch j+3 into set j%3 next to staging j+1 from set (j+1)%3 (the
        // store is unconditional: B[(nc)&1] is free at the last chunk)
#define GS_BITER(j, Sn, Ss)                                                                         \
    {                                                                                             \
        const uint32_t kc0_ = (j0 + jr(min((uint32_t)(j) + 3u, ncl - 1u))) * KC;                 \
        _Pragma("unroll") for (uint32_t i = 0; i < NB; i++) {                                     \
            const uint32_t u = bt + i * NBT;                                                      \
            const uint32_t k = u / UB;                                                            \
            const uint32_t kk = kc0_ + k < K ? kc0_ + k : kc0_;                                   \
            Sn[i] = *reinterpret_cast<const u32x4 *>(B + (size_t)kk * N + ((u % UB) * 8u < N ? (u % UB) * 8u : 0u)); \
            GS_BSTORE_UNIT((j) + 1u, Ss, i);                                                      \
        }                                                                                         \
        GS_STAMP(2u + 2u * (j));                                                                  \
        __syncthreads();                                                                          \
        GS_STAMP(3u + 2u * (j));                                                                  \
    }
        GS_BLOAD(0u, s0);
        GS_BLOAD(1u, s1);
        GS_BLOAD(2u, s2);
        __syncthreads();  // dense images cleared
#pragma unroll
        for (uint32_t i = 0; i < NB; i++) GS_BSTORE_UNIT(0u, s0, i);
        GS_STAMP(1u);
        __syncthreads();  // chunk 0 staged
        uint32_t j = 0;
        for (; j + 2 < ncl; j += 3) {
            GS_BITER(j, s0, s1);
            GS_BITER(j + 1, s1, s2);
            GS_BITER(j + 2, s2, s0);
        }
        if (j < ncl) GS_BITER(j, s0, s1);
        if (j + 1 < ncl) GS_BITER(j + 1, s1, s2);
#undef GS_BITER
#undef GS_BSTORE_UNIT
#undef GS_BLOAD
        __syncthreads();
    } else {
        // ---------------------------------------------------------------- entries
        u32x4 p0[MAXA], v0[MAXA], p1[MAXA], v1[MAXA], p2[MAXA], v2[MAXA], p3[MAXA], v3[MAXA];
#define GS_ALOAD(j, P, V)                                                                           \
    {                                                                                             \
        const uint32_t jj_ = jr(min((uint32_t)(j), ncl - 1u));                                    \
        const uint32_t s0_ = GS_SEG(jj_);                                                         \
        const uint32_t G_ = (uint32_t)(j) < ncl ? GS_SEG(jj_ + 1) - s0_ : 0u;                     \
        _Pragma("unroll") for (int I = 0; I < MAXA; I++) {                                        \
            const uint32_t q = at + I * NAT;                                                      \
            const size_t qq = (size_t)s0_ + (q < G_ ? q : 0u);                                    \
            P[I] = tP[qq];                                                                        \
            V[I] = tV[qq];                                                                        \
        }                                                                                         \
    }
#define GS_SCATTER(j, P, V)                                                                         \
    {                                                                                             \
        const uint32_t G_ = GS_SEG(jr(j) + 1) - GS_SEG(jr(j));                                    \
        unsigned char *ld_ = lds + oD + ((j) % NDI) * szD;                                        \
        _Pragma("unroll") for (int I = 0; I < MAXA; I++) {                                        \
            const uint32_t q = at + I * NAT;                                                      \
            if (q < G_) {                                                                         \
                _Pragma("unroll") for (int e = 0; e < 8; e++) {                                   \
                    const uint32_t h = (P[I][e >> 1] >> (16 * (e & 1))) & 0xffffu;                \
                    const uint16_t v = (uint16_t)((V[I][e >> 1] >> (16 * (e & 1))) & 0xffffu);    \
                    *reinterpret_cast<uint16_t *>(ld_ + h * 2u) = v;                              \
                }                                                                                 \
            }                                                                                     \
        }                                                                                         \
    }
        // chunk j: fetch j+4 into set j%4, scatter j+1 from set (j+1)%4
#define GS_AITER(j, Pn, Vn, Ps, Vs)                                                                 \
    {                                                                                             \
        if (!(DBG & 8)) GS_ALOAD((j) + 4, Pn, Vn);                                                \
        GS_STAMP(2u + 2u * (j)); /* entry role: loads issued, then scatter done */                \
        flg_wait(2, WC * (uint32_t)(j)); /* FLG: chunk j-1 consumed, its image cleared */         \
        if ((j) + 1 < ncl && !(DBG & 2)) GS_SCATTER((j) + 1, Ps, Vs);                             \
        GS_STAMP(3u + 2u * (j));                                                                  \
        if constexpr (FLG) flg_arrive(1);                                                         \
        else __syncthreads();                                                                     \
    }
        GS_ALOAD(0u, p0, v0);
        GS_ALOAD(1u, p1, v1);
        GS_ALOAD(2u, p2, v2);
        GS_ALOAD(3u, p3, v3);
        __syncthreads();  // dense images cleared
        GS_SCATTER(0u, p0, v0);
        GS_STAMP(1u);
        __syncthreads();  // chunk 0 staged
        uint32_t j = 0;
        for (; j + 3 < ncl; j += 4) {
            GS_AITER(j, p0, v0, p1, v1);
            GS_AITER(j + 1, p1, v1, p2, v2);
            GS_AITER(j + 2, p2, v2, p3, v3);
            GS_AITER(j + 3, p3, v3, p0, v0);
        }
        if (j < ncl) GS_AITER(j, p0, v0, p1, v1);
        if (j + 1 < ncl) GS_AITER(j + 1, p1, v1, p2, v2);
        if (j + 2 < ncl) GS_AITER(j + 2, p2, v2, p3, v3);
#undef GS_AITER
#undef GS_SCATTER
#undef GS_ALOAD
        __syncthreads();
    }
#undef GS_SEG
    __syncthreads();
    // fixed-order reduction of the compute waves' partial tiles (all threads)
    const float *red = reinterpret_cast<const float *>(lds);
    auto tile_sum = [&](uint32_t e, uint32_t &row, uint32_t &colx) {
        const uint32_t cc = e & 15u, rr = (e >> 4) & 15u, tt = e >> 8;
        const uint32_t rt = tt / CT, ct = tt % CT;
        const uint32_t ln = 16u * (rr >> 2) + cc, i = rr & 3u;
        float sum = 0.f;
#pragma unroll
        for (uint32_t w = 0; w < WC; w++) sum += red[(((w * RT + rt) * CT + ct) * 64u + ln) * 4u + i];
        row = 16u * rt + rr;
        colx = 16u * ct + cc;
        return sum;
    };
    if (nsplit == 1) {
        for (uint32_t e = tid; e < RT * CT * 256u; e += NT) {
            uint32_t row, colx;
            const float sum = tile_sum(e, row, colx);
            if (row < R && colx < N) C[(size_t)(row_base + r0 + row) * N + colx] = (f16)sum;
        }
    } else {
        // K-split: this workgroup's fp32 slab, then the last of the row block's
        // nsplit workgroups sums the slabs in split order (deterministic) and stores C.
        // Slabs and the arrival counter use agent-scope relaxed atomics: the stores and
        // loads themselves are device-coherent (no L2 write-back / invalidate fences
        // across the XCDs); the stores are complete (vmcnt 0) before the counter moves,
        // and the combining workgroup loads only after it has seen the count.
        float *slab = slabs + ((size_t)g * nsplit + sp) * RMAX * N;
        for (uint32_t e = tid; e < RT * CT * 256u; e += NT) {
            uint32_t row, colx;
            const float sum = tile_sum(e, row, colx);
            if (row < R && colx < N)
                __hip_atomic_store(slab + (size_t)row * N + colx, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        uint32_t *flag = reinterpret_cast<uint32_t *>(lds + oD + NDI * szD + 512);
        if (tid == 0)
            *flag = __hip_atomic_fetch_add(&arrivals[g], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        if (*flag == nsplit - 1u) {
            if (tid == 0) __hip_atomic_store(&arrivals[g], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float *base = slabs + (size_t)g * nsplit * RMAX * N;
            for (uint32_t e = tid; e < R * N; e += NT) {
                float sum = 0.f;
                for (uint32_t q = 0; q < nsplit; q++)
                    sum += __hip_atomic_load(base + (size_t)q * RMAX * N + e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                C[(size_t)(row_base + r0) * N + e] = (f16)sum;
            }
        }
    }
    if constexpr (STAMPS) {
        __syncthreads();
        if (tid == 0) {
            lst[63] = __builtin_amdgcn_s_memtime();
            for (uint32_t i = 0; i < 64; i++) stamps[(size_t)blockIdx.x * 64 + i] = lst[i];
        }
    }
#undef GS_STAMP
}

}  // namespace gsk
