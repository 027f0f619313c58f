// hip_code/mfma_bm_exp.hpp -- experiments build only (measured slower than k_mfma_rows /
// k_mfma_ks, kept opt-in): the bitmap-layout matrix-core kernels k_mfma_kb, k_mfma_bm, k_mfma_bm2.
// Included only under GS_EXPERIMENTS; instantiated by kernels/ks_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// k_mfma_kb -- k_mfma_ks's K split and per-wave pipeline on k_mfma_bm's bitmap layout: no
// dense image, no entry scatter.  Per (unit u = row block g x K range q, 32-column k-step s)
// one 8-byte record per lane l (byte t < RT: the occupancy of row 16t + l%16, columns
// 32s + 8(l/16) + [0, 8) -- exactly the 8 halves lane l holds of tile t's A operand of
// v_mfma_f32_16x16x32_f16 -- bytes 6..7: the lane's first value from the step's base
// sbase[u*NS + s]) and the step's values, lane after lane, tile after tile (host layout:
// device_layout.cc build_bm_tiles).  A is ~2.4 B per nonzero at 30% density (k_mfma_ks:
// 4 B).  Wave w runs steps w, w+W, ...: a slot's record and value bounds are loaded one
// round (D steps) ahead of its values; the values are fetched as whole 16-B units (the
// step's run from its 16-B-aligned start, NVB KB at most: one full wave load per KB, lanes
// past the run re-read the first unit) and staged through the wave's LDS slot with B's rows
// (b_piece-permuted, ds_read_b64_tr_b16 fragments); each lane reads its two 8-byte windows
// per tile there and expands them into the tile's fragment by four v_perm_b32 with
// selectors from a 16-entry LDS table.  (The first version loaded the windows straight from
// HBM: 2 x RT 8-byte loads per lane and step at 2-byte alignment, ~40% of each request
// used -- C2 21.1 us; the windows alone cost 11.5 us of it.)  Epilogue as k_mfma_ks (wave
// partial tiles summed in wave order, tagged-slab K-range combine).
// ---------------------------------------------------------------------------
// DBG (experiments diagnostics, wrong results): 2 = no value loads, 3 = no B loads
template <int CT, int RT, int W, int D, int NVB, bool STAMPS, int DBG = 0>
__device__ __forceinline__ void kb_body(const uint32_t *__restrict__ bmtb_first_row, const uint2 *__restrict__ rec,
                                        const uint32_t *__restrict__ sbase, const f16 *__restrict__ vals,
                                        const f16 *__restrict__ B, f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t S,
                                        uint32_t NS, uint32_t nwg, uint32_t row_base, float *__restrict__ slabs,
                                        uint32_t *__restrict__ arrivals, uint64_t *__restrict__ stamps, uint32_t bx,
                                        uint32_t prio) {
    static_assert(RT >= 1 && RT <= 6, "six mask bytes per record");
    static_assert(NVB >= 1 && NVB <= 4, "1..4 KB of values per step");
    constexpr uint32_t RB = 32 * CT;  // bytes per LDS B row (a 16*CT-column tile)
    constexpr uint32_t UB = 2 * CT;   // 16-B units per B row
    constexpr uint32_t STG = 32u * RB;  // one k-step of B rows
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t u = xcd_block(bx, nwg);
    const uint32_t g = u / S, q = u - g * S;
#define GS_KB_STAMP(slot)                                                                          \
    if constexpr (STAMPS) {                                                                        \
        if (lane == 0) stamps[((size_t)blockIdx.x * W + wv) * 32u + (slot)] = __builtin_amdgcn_s_memtime(); \
    }
    GS_KB_STAMP(0u);
    const uint32_t k0 = q * NS * 32u;
    const uint32_t col0 = blockIdx.y * 16u * CT, nv = min(16u * CT, N - col0);
    uint2 *lut = reinterpret_cast<uint2 *>(lds);
    unsigned char *bst = lds + 128u + wv * (STG + NVB * 1024u);
    unsigned char *vst = bst + STG;  // the step's values (16-B-aligned run start at byte 0)
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    if (tid < 16u) lut[tid] = make_uint2(bm_sel(tid, 0), bm_sel(tid, 1));

    const uint32_t nsw = NS > wv ? (NS - wv + W - 1u) / W : 0u;
    const size_t ubase = (size_t)u * NS;
    u32x4 BR[D][CT];
    u32x4 VR[D][NVB];  // per slot: the values of the step it holds (16-B units)
    uint2 RC[D];       // ... its record
    uint32_t RL[D];    // ... and its first value's offset (halves) from the run's aligned start
    uint2 NX[D];       // per slot: record of the step the slot loads next
    uint32_t NB[D], NE[D];  // ... and its value bounds [sbase[s], sbase[s+1])
    uint32_t vz;
    __asm__ volatile("v_mov_b32 %0, 0" : "=v"(vz));
    auto st_of = [&](uint32_t i) -> uint32_t { return __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u); };
    auto mbyte = [](const uint2 &r, int t) -> uint32_t {
        return t < 4 ? (r.x >> (8 * t)) & 0xffu : (r.y >> (8 * (t - 4))) & 0xffu;
    };
    // record + value bounds of step i (vector loads, in order with the values: see k_mfma_ks)
    auto load_rec = [&](uint32_t i, uint2 &NX_, uint32_t &NB_, uint32_t &NE_) {
        const uint32_t st = st_of(i);
        NX_ = rec[(ubase + st) * 64u + lane + vz];
        NB_ = sbase[ubase + st + vz];
        NE_ = sbase[ubase + st + 1u + vz];
    };
    auto load_b = [&](uint32_t i, u32x4 (&B_)[CT]) {
        const uint32_t kr = k0 + st_of(i) * 32u;
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint32_t un = lane + 64u * c;
            const uint32_t k = kr + un / UB, cu = (un % UB) * 8u;
            if constexpr (DBG == 3) B_[c] = u32x4{k, cu, k, cu};
            else B_[c] = *reinterpret_cast<const u32x4 *>(B + (size_t)(k < K ? k : K - 1u) * N + col0 + (cu < nv ? cu : 0u));
        }
    };
    // the slot takes over the record it loaded a round ago, issues its step's values, and
    // loads the record of its step a round ahead
    auto load_v = [&](uint32_t i, uint2 &NX_, uint32_t &NB_, uint32_t &NE_, uint2 &RC_, uint32_t &RL_,
                      u32x4 (&VR_)[NVB]) {
        RC_ = NX_;
        const uint32_t b0 = NB_ & ~7u, len = NE_ - b0;  // halves from the aligned start
        RL_ = NB_ - b0;
#pragma unroll
        for (int j = 0; j < NVB; j++) {
            const uint32_t h = 8u * (lane + 64u * j);
            if constexpr (DBG == 2) VR_[j] = u32x4{RC_.x, RC_.y, RC_.x, RC_.y};
            else VR_[j] = *reinterpret_cast<const u32x4 *>(vals + b0 + (h < len ? h : 0u));
        }
        load_rec(i + D, NX_, NB_, NE_);
    };
#pragma unroll
    for (int d = 0; d < D; d++) load_rec((uint32_t)d, NX[d], NB[d], NE[d]);
#pragma unroll
    for (int d = 0; d < D; d++) load_b((uint32_t)d, BR[d]);
#pragma unroll
    for (int d = 0; d < D; d++) load_v((uint32_t)d, NX[d], NB[d], NE[d], RC[d], RL[d], VR[d]);
    // the selector table (written by wave 0) before any wave expands a fragment
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __asm__ volatile("" ::: "memory");
    GS_KB_STAMP(1u);

    f4v acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};

    auto step = [&](uint32_t i, uint2 &NX_, uint32_t &NB_, uint32_t &NE_, uint2 &RC_, uint32_t &RL_,
                    u32x4 (&VR_)[NVB], u32x4 (&B_)[CT]) {
        const bool live = i < nsw;  // wave-uniform
        h8v av[RT], bv[CT];
        if (live) {
            const uint32_t kr = k0 + (wv + i * W) * 32u;
#pragma unroll
            for (int c = 0; c < CT; c++) {
                const uint32_t un = lane + 64u * c, k = un / UB, s = un % UB;
                *reinterpret_cast<u32x4 *>(bst + k * RB + b_piece<CT>(k, s >> 1) * 32u + (s & 1u) * 16u) =
                    kr + k < K && s * 8u < nv ? B_[c] : zero4;
            }
#pragma unroll
            for (int j = 0; j < NVB; j++) *reinterpret_cast<u32x4 *>(vst + (lane + 64u * j) * 16u) = VR_[j];
            const uint32_t kb = 8u * (lane >> 4);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                s4v t2[2];
#pragma unroll
                for (int hh = 0; hh < 2; hh++) {
                    const uint32_t k = kb + 4u * hh + ((lane & 15u) >> 2);
                    t2[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (lds_s4v *)(bst + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));
                }
                __builtin_memcpy(&bv[ct], t2, 16);
            }
            uint32_t p = RL_ + (RC_.y >> 16);
#pragma unroll
            for (int t = 0; t < RT; t++) {
                const uint32_t m = mbyte(RC_, t);
                const uint2 sl = lut[m & 15u], sh = lut[m >> 4];
                const u32x2_a2 lo = *reinterpret_cast<const u32x2_a2 *>(vst + 2u * p);
                const u32x2_a2 hi = *reinterpret_cast<const u32x2_a2 *>(vst + 2u * (p + __builtin_popcount(m & 15u)));
                p += __builtin_popcount(m);
                uint32_t w4[4];
                w4[0] = __builtin_amdgcn_perm(lo.y, lo.x, sl.x);
                w4[1] = __builtin_amdgcn_perm(lo.y, lo.x, sl.y);
                w4[2] = __builtin_amdgcn_perm(hi.y, hi.x, sh.x);
                w4[3] = __builtin_amdgcn_perm(hi.y, hi.x, sh.y);
                __builtin_memcpy(&av[t], w4, 16);
            }
        }
        load_b(i + D, B_);
        load_v(i + D, NX_, NB_, NE_, RC_, RL_, VR_);
        if (live) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av[rt], bv[ct], acc[rt][ct], 0, 0, 0);
            if (i < 16u) GS_KB_STAMP(3u + i);
        }
    };
    const bool young = wv >= W / 2u;
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(1);
    for (uint32_t i0 = 0; i0 < nsw; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(i0 + d, NX[d], NB[d], NE[d], RC[d], RL[d], VR[d], BR[d]);
    }
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(0);
    GS_KB_STAMP(20u);
    // ---- K-split ticket: wave 0 takes its row block's arrival ticket as soon as its own
    // loop ends, so the add's round trip overlaps the partial-tile reduction below
    uint32_t *arr = arrivals + (size_t)g * gridDim.y + blockIdx.y;
    uint32_t ticket = 0;
    if (S > 1 && wv == 0 && lane == 0) ticket = __hip_atomic_fetch_add(arr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- wave partial tiles -> LDS (the trailing loads write registers only), summed in
    // wave order.  Item t = (tile, lane) of a 16x16 tile: the 4 rows 4*(lane/16)+i of
    // column lane%16.  When the W partial tiles fit LDS beside the wave images (APART), each
    // wave stores its tile as soon as its loop ends, without waiting for the others
    constexpr bool APART = kb_red_apart(CT, RT, W, NVB);
    f4v *red = reinterpret_cast<f4v *>(lds + (APART ? kb_stage_bytes(CT, W, NVB) : 0u));
    constexpr bool HALVES = !APART && ks_red_halves(CT, RT, W);
    constexpr uint32_t WR = HALVES ? W / 2 : W;  // partial tiles summed from LDS
    uint32_t *flag = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(red) + (size_t)WR * RT * CT * 1024u);
    if constexpr (!APART) {
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
    }
    if constexpr (HALVES) {
        if (wv >= WR) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++) red[(((wv - WR) * RT + rt) * CT + ct) * 64u + lane] = acc[rt][ct];
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
        if (wv < WR) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++) acc[rt][ct] += red[((wv * RT + rt) * CT + ct) * 64u + lane];
        }
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
    }
    if (wv < WR) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) red[((wv * RT + rt) * CT + ct) * 64u + lane] = acc[rt][ct];
    }
    if (S > 1 && wv == 0 && lane == 0) *flag = ticket;  // (waits for the add's return)
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __asm__ volatile("" ::: "memory");
    constexpr uint32_t NI = RT * CT * 64u, NT = 64u * W;
    const uint32_t r0 = bmtb_first_row[g], R = bmtb_first_row[g + 1] - r0;
    auto item_sum = [&](uint32_t t) {
        f4v sum = red[t];
#pragma unroll
        for (uint32_t w = 1; w < WR; w++) sum += red[w * NI + t];
        return sum;
    };
    auto store_item = [&](uint32_t t, const f4v &v) {
        const uint32_t ln = t & 63u, tt = t >> 6, rt = tt / CT, ct = tt % CT;
        const uint32_t col = 16u * ct + (ln & 15u), rb = 16u * rt + 4u * (ln >> 4);
        if (col >= nv) return;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (rb + i < R) C[(size_t)(row_base + r0 + rb + i) * N + col0 + col] = (f16)v[i];
    };
    GS_KB_STAMP(21u);
    if (S == 1) {
        for (uint32_t t = tid; t < NI; t += NT) store_item(t, item_sum(t));
        GS_KB_STAMP(22u);
        return;
    }
    // ---- K-split combine by tagged slabs.  Every fp32 word of a published slab carries
    // its own validity tag in the low mantissa bit (the reader drops the bit, a 2^-24
    // relative truncation), so no store needs to be drained before a signal: every workgroup
    // stores its slab with 16-B write-through (sc1) stores, and the one that drew the last
    // ticket loads each other slab word with agent-scope (sc1) loads until its tag reads
    // this launch's value -- its writer holds an earlier ticket, so it is running and its
    // stores are issued or about to be -- sums the S partials in q order (deterministic) and
    // writes C.  The tag alternates from launch to launch: the arrival counter holds
    // (epoch << 16) | arrivals, the tag is epoch ^ 1, and the last workgroup re-arms the
    // counter with the epoch flipped and no arrivals.  Every slab word then holds the
    // previous launch's tag when a launch starts (the last workgroup stores its own slab
    // too), and the zero-filled first state reads as "tag 0, epoch 0" -- so no slab is
    // cleared after use ((S - 1) fewer slab stores than clearing, the last workgroup's own
    // store issued before it waits).  Every access to the slabs is sc1 (MI355X_MICROARCH.md
    // Workgroup dispatch, Valid forms: the R2 granule, here one naturally aligned word).
    // The next launch on the stream starts after these stores complete.
    const uint32_t tk = *flag & 0xffffu, tag = ((*flag >> 16) & 1u) ^ 1u;
    f4v *slab = reinterpret_cast<f4v *>(slabs) + ((size_t)u * gridDim.y + blockIdx.y) * NI;
    auto tagged = [&](const f4v &v) {
        u32x4 w;
        __builtin_memcpy(&w, &v, 16);
        w[0] = (w[0] & ~1u) | tag; w[1] = (w[1] & ~1u) | tag; w[2] = (w[2] & ~1u) | tag; w[3] = (w[3] & ~1u) | tag;
        return w;
    };
    for (uint32_t t = tid; t < NI; t += NT) {
        const u32x4 w = tagged(item_sum(t));
        __asm__ volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(slab + t), "v"(w) : "memory");
    }
    if (tk != S - 1u) {
        GS_KB_STAMP(22u);
        return;
    }
    if (tid == 0) __hip_atomic_store(arr, tag << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const f4v *base = reinterpret_cast<const f4v *>(slabs) + blockIdx.y * NI;
    const size_t qstride = (size_t)gridDim.y * NI;  // slab of (g, qq) = base + (g*S + qq) * qstride
    uint32_t *err = arrivals + (size_t)(nwg / S) * gridDim.y;  // the replica's device error word
    for (uint32_t t = tid; t < NI; t += NT) {
        f4v sum = {0.f, 0.f, 0.f, 0.f};
        for (uint32_t qq = 0; qq < S; qq++) {
            u32x4 w;
            if (qq == q) {  // truncated as a published word is (whichever workgroup is last: deterministic)
                w = tagged(item_sum(t));
            } else {
                w = ks_slab_wait(reinterpret_cast<const uint32_t *>(base + ((size_t)g * S + qq) * qstride + t), tag, err,
                                 GS_KS_FORCE(prio));
            }
            w[0] &= ~1u; w[1] &= ~1u; w[2] &= ~1u; w[3] &= ~1u;
            f4v x;
            __builtin_memcpy(&x, &w, 16);
            sum += x;
        }
        store_item(t, sum);
    }
    GS_KB_STAMP(22u);
#undef GS_KB_STAMP
}

template <int CT, int RT, int W, int D, int NVB, bool STAMPS = false, int DBG = 0>
__global__ __launch_bounds__(64 * W) void k_mfma_kb(const uint32_t *__restrict__ bmtb_first_row,  // nb+1
                                                    const uint2 *__restrict__ rec,       // (u*NS + step)*64 + lane
                                                    const uint32_t *__restrict__ sbase,  // u*NS + step (+1)
                                                    const f16 *__restrict__ vals, const f16 *__restrict__ B,
                                                    f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t S,
                                                    uint32_t NS, uint32_t nwg, uint32_t row_base,
                                                    float *__restrict__ slabs, uint32_t *__restrict__ arrivals,
                                                    uint64_t *__restrict__ stamps = nullptr, uint32_t prio = 0) {
    kb_body<CT, RT, W, D, NVB, STAMPS, DBG>(bmtb_first_row, rec, sbase, vals, B, C, K, N, S, NS, nwg, row_base, slabs, arrivals,
                                  stamps, blockIdx.x, prio);
}

// ---------------------------------------------------------------------------
// k_mfma_bm -- BMTB row blocks on the matrix cores from a bitmap layout, with the
// dense A fragments built in registers (no dense image, no LDS scatter).
// Why: k_mfma_rows / k_mfma_ks move 4 B per nonzero ([u16 position][f16 value]) and
// scatter every entry into a dense LDS image (two LDS stores per entry, one to clear
// it); at 30% density a bitmap costs 0.42 B per nonzero, so A is ~2.4 B per nonzero
// and no entry ever passes through LDS.
// Layout (host/device_layout.cc build_bm_tiles): unit u = (row block g, K range q) of
// NS 32-column k-steps; per (u, step) one 8-byte record per lane l: byte t (t < RT) is
// the occupancy of row 16t + l%16, columns 32*step + 8*(l/16) + [0, 8) -- exactly the 8
// halves lane l holds of the A operand of v_mfma_f32_16x16x32_f16 for row tile t --
// and bytes 6..7 the lane's first value (halves, from the step's base sbase[u*NS+step]);
// a step's values are stored lane after lane, tile after tile, ascending columns.
// Wave w of the workgroup owns the range's k-steps w, w+W, ...: per k-step it loads the
// 32 B rows into registers and stores them into its own LDS ring slot (32-B pieces
// permuted by b_piece, so the ds_read_b64_tr_b16 fragment reads are conflict-free; not
// LDS-DMA: the compiler then waits for every DMA in flight before each LDS read of the
// same wave), loads the record, then per row tile two 8-byte
// value windows (at the tile's first value and past the low nibble's values; 2-byte
// aligned loads) that two v_perm_b32 each expand into the tile's dense fragment with
// selectors from a 16-entry table in LDS, and runs RT x CT MFMAs.  Pipeline per wave:
// B + record two steps ahead, B store + values one step ahead (counted waits); no
// workgroup barrier until the end.  Epilogue as k_mfma_ks: the W partial tiles summed in
// wave order through LDS, then C (S = 1) or a write-through fp32 slab + one arrival add,
// the last of the row block's S workgroups summing the slabs in q order (deterministic).
// Rows of B past K are read as row K-1 against zero A columns (a non-finite B value
// there gives NaN: the documented matrix-core deviation).
// ---------------------------------------------------------------------------

// STAMPS (diagnostic build only, gs_debug_mfma_timeline): lane 0 of every wave records
// s_memtime into stamps[(workgroup * W + wave) * 16 + slot]: 0 start, 1 B + records issued,
// 2 values issued, 3 B stored (all landed), 4 MFMAs done (first batch), 5 loop done,
// 6 reduced, 7 slab published, 8 end
template <int CT, int RT, int W, int NBT, bool STAMPS = false>
__global__ __launch_bounds__(64 * W) void k_mfma_bm(const uint32_t *__restrict__ bmtb_first_row,  // nb+1
                                                    const uint2 *__restrict__ rec,       // (u*NS + step)*64 + lane
                                                    const uint32_t *__restrict__ sbase,  // u*NS + step (+1)
                                                    const f16 *__restrict__ vals, const f16 *__restrict__ B,
                                                    f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t S,
                                                    uint32_t NS, uint32_t nwg, uint32_t row_base,
                                                    float *__restrict__ slabs, uint32_t *__restrict__ arrivals,
                                                    uint64_t *__restrict__ stamps = nullptr) {
    static_assert(RT >= 1 && RT <= 6, "six mask bytes per record");
#define GS_BM_STAMP(slot)                                                                          \
    if constexpr (STAMPS) {                                                                        \
        if ((threadIdx.x & 63u) == 0) stamps[((size_t)blockIdx.x * W + (threadIdx.x >> 6)) * 16u + (slot)] = __builtin_amdgcn_s_memtime(); \
    }
    GS_BM_STAMP(0u);
    constexpr uint32_t RB = 32 * CT;     // bytes per LDS B row (a 16*CT-column tile)
    constexpr uint32_t UB = 2 * CT;      // 16-B units per B row
    constexpr uint32_t STG = 32u * RB;   // one k-step of B rows = CT LDS-DMA wave-instructions
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t u = xcd_block(blockIdx.x, nwg);  // nwg == gridDim.x
    const uint32_t g = u / S, q = u - g * S;
    const uint32_t col0 = blockIdx.y * 16u * CT, nv = min(16u * CT, N - col0);
    uint2 *lut = reinterpret_cast<uint2 *>(lds);
    unsigned char *ring = lds + 128u + wv * NBT * STG;  // this wave's NBT k-step slots
    if (tid < 16u) lut[tid] = make_uint2(bm_sel(tid, 0), bm_sel(tid, 1));
    const uint32_t k0 = q * NS * 32u;
    const uint32_t nsw = NS > wv ? (NS - wv + W - 1u) / W : 0u;  // this wave's k-steps
    const size_t ub = (size_t)u * NS;
    // steps past the wave's last re-read its first (cached)
    auto step_of = [&](uint32_t i) -> uint32_t { return i < nsw ? wv + i * W : wv; };
    // B rows of step i -> registers (16-B units, lane-linear over the step's 32 rows), then into
    // slot j with the 32-B pieces permuted by b_piece (conflict-free transposed reads).  Not
    // LDS-DMA: the compiler then waits for all DMA in flight before the wave's next
    // dependent load, which serialises the records and the value windows behind the B rows
    auto load_b = [&](uint32_t i, u32x4 (&BR)[CT]) {
        const uint32_t kr = k0 + step_of(i) * 32u;
#pragma unroll
        for (uint32_t c = 0; c < CT; c++) {
            const uint32_t un = c * 64u + lane, k = un / UB, cu = (un % UB) * 8u;
            const uint32_t kk = kr + k < K ? kr + k : K - 1u;
            BR[c] = *reinterpret_cast<const u32x4 *>(B + (size_t)kk * N + col0 + (cu < nv ? cu : 0u));
        }
    };
    auto store_b = [&](uint32_t j, const u32x4 (&BR)[CT]) {
        unsigned char *dst = ring + j * STG;
#pragma unroll
        for (uint32_t c = 0; c < CT; c++) {
            const uint32_t un = c * 64u + lane, k = un / UB, s = un % UB;
            *reinterpret_cast<u32x4 *>(dst + k * RB + b_piece<CT>(k, s >> 1) * 32u + (s & 1u) * 16u) = BR[c];
        }
    };
    auto mbyte = [](const uint2 &r, int t) -> uint32_t {
        return t < 4 ? (r.x >> (8 * t)) & 0xffu : (r.y >> (8 * (t - 4))) & 0xffu;
    };
    f4v acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    const uint32_t kb = 8u * (lane >> 4);
    bool first = true;
    // batches of NBT k-steps: every load of the batch in flight at once (records, then the B
    // rows by DMA, then -- once each record is in -- the value windows), then the MFMAs
    for (uint32_t i0 = 0; i0 < nsw; i0 += NBT) {
        // B rows first (L2-served: they return before the records from HBM, and loads retire
        // in order, so waiting for the records costs nothing extra)
        u32x4 br[NBT][CT];
#pragma unroll
        for (int j = 0; j < NBT; j++) load_b(i0 + j, br[j]);
        uint2 rc[NBT];
        uint32_t sb[NBT];
#pragma unroll
        for (int j = 0; j < NBT; j++) {
            sb[j] = sbase[ub + step_of(i0 + j)];  // wave-uniform: a scalar load
            rc[j] = rec[(ub + step_of(i0 + j)) * 64u + lane];
        }
        if (first) GS_BM_STAMP(1u);
        u32x2_a2 vv[NBT][RT][2];
#pragma unroll
        for (int j = 0; j < NBT; j++) {
            uint32_t p = sb[j] + (rc[j].y >> 16);
#pragma unroll
            for (int t = 0; t < RT; t++) {
                const uint32_t m = mbyte(rc[j], t);
                vv[j][t][0] = *reinterpret_cast<const u32x2_a2 *>(vals + p);
                vv[j][t][1] = *reinterpret_cast<const u32x2_a2 *>(vals + p + __builtin_popcount(m & 15u));
                p += __builtin_popcount(m);
            }
        }
        if (first) GS_BM_STAMP(2u);
#pragma unroll
        for (int j = 0; j < NBT; j++) store_b(j, br[j]);
        if (first) {  // the selector table (its stores, once)
            __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            __asm__ volatile("" ::: "memory");
            GS_BM_STAMP(3u);
        }
#pragma unroll
        for (int j = 0; j < NBT; j++) {
            if (i0 + j < nsw) {
                const unsigned char *bst = ring + j * STG;
                h8v bv[CT];
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    s4v t2[2];
#pragma unroll
                    for (int hh = 0; hh < 2; hh++) {
                        const uint32_t k = kb + 4u * hh + ((lane & 15u) >> 2);
                        t2[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s4v *)(bst + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));
                    }
                    __builtin_memcpy(&bv[ct], t2, 16);
                }
#pragma unroll
                for (int t = 0; t < RT; t++) {
                    const uint32_t m = mbyte(rc[j], t);
                    const uint2 sl = lut[m & 15u], sh = lut[m >> 4];
                    const u32x2_a2 lo = vv[j][t][0], hi = vv[j][t][1];
                    uint32_t w[4];
                    w[0] = __builtin_amdgcn_perm(lo.y, lo.x, sl.x);
                    w[1] = __builtin_amdgcn_perm(lo.y, lo.x, sl.y);
                    w[2] = __builtin_amdgcn_perm(hi.y, hi.x, sh.x);
                    w[3] = __builtin_amdgcn_perm(hi.y, hi.x, sh.y);
                    h8v a;
                    __builtin_memcpy(&a, w, 16);
#pragma unroll
                    for (int ct = 0; ct < CT; ct++)
                        acc[t][ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bv[ct], acc[t][ct], 0, 0, 0);
                }
            }
        }
        if (first) {
            GS_BM_STAMP(4u);
            first = false;
        }
    }
    GS_BM_STAMP(5u);
    if (first) {  // a wave with no k-steps still meets the table barrier
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
    }
    // every wave is done with its ring before it is reused for the partial tiles
    __syncthreads();
    f4v *red = reinterpret_cast<f4v *>(lds);
    constexpr bool HALVES = bm_red_halves(CT, RT, W);
    constexpr uint32_t WR = HALVES ? W / 2 : W;
    if constexpr (HALVES) {
        if (wv >= WR) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++) red[(((wv - WR) * RT + rt) * CT + ct) * 64u + lane] = acc[rt][ct];
        }
        __syncthreads();
        if (wv < WR) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++) acc[rt][ct] += red[((wv * RT + rt) * CT + ct) * 64u + lane];
        }
        __syncthreads();
    }
    if (wv < WR) {
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int ct = 0; ct < CT; ct++) red[((wv * RT + rt) * CT + ct) * 64u + lane] = acc[rt][ct];
    }
    __syncthreads();
    constexpr uint32_t NI = RT * CT * 64u, NT = 64u * W;
    const uint32_t r0 = bmtb_first_row[g], R = bmtb_first_row[g + 1] - r0;
    auto item_sum = [&](uint32_t t) {
        f4v sum = red[t];
#pragma unroll
        for (uint32_t w = 1; w < WR; w++) sum += red[w * NI + t];
        return sum;
    };
    auto store_item = [&](uint32_t t, const f4v &v) {
        const uint32_t ln = t & 63u, tt = t >> 6, rt = tt / CT, ct = tt % CT;
        const uint32_t col = 16u * ct + (ln & 15u), rb = 16u * rt + 4u * (ln >> 4);
        if (col >= nv) return;
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (rb + i < R) C[(size_t)(row_base + r0 + rb + i) * N + col0 + col] = (f16)v[i];
    };
    GS_BM_STAMP(6u);
    if (S == 1) {
        for (uint32_t t = tid; t < NI; t += NT) store_item(t, item_sum(t));
        GS_BM_STAMP(8u);
        return;
    }
    // K-split hand-off (k_mfma_ks's form): 16-B write-through slab stores, every storing
    // wave's vmcnt(0), a barrier, one agent-scope arrival add; the last adder (told by the
    // returned count) loads the other slabs with agent-scope (sc1) loads
    f4v *slab = reinterpret_cast<f4v *>(slabs) + ((size_t)u * gridDim.y + blockIdx.y) * NI;
    for (uint32_t t = tid; t < NI; t += NT) {
        const f4v v = item_sum(t);
        __asm__ volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(slab + t), "v"(v) : "memory");
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    uint32_t *flag = reinterpret_cast<uint32_t *>(lds + (size_t)WR * NI * 16u);
    uint32_t *arr = arrivals + (size_t)g * gridDim.y + blockIdx.y;
    if (tid == 0) *flag = __hip_atomic_fetch_add(arr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    GS_BM_STAMP(7u);
    if (*flag != S - 1u) {
        GS_BM_STAMP(8u);
        return;
    }
    if (tid == 0) __hip_atomic_store(arr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const f4v *base = reinterpret_cast<const f4v *>(slabs) + blockIdx.y * NI;
    const size_t qstride = (size_t)gridDim.y * NI;
    for (uint32_t t = tid; t < NI; t += NT) {
        const f4v own = item_sum(t);
        f4v sum = {0.f, 0.f, 0.f, 0.f};
        for (uint32_t qq = 0; qq < S; qq++) {
            if (qq == q) {
                sum += own;
                continue;
            }
            const float *src = reinterpret_cast<const float *>(base + ((size_t)g * S + qq) * qstride + t);
            f4v x;
#pragma unroll
            for (int i = 0; i < 4; i++) x[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sum += x;
        }
        store_item(t, sum);
    }
    GS_BM_STAMP(8u);
#undef GS_BM_STAMP
}

// ---------------------------------------------------------------------------
// k_mfma_bm2 -- k_mfma_bm's layout with one wave per 16-row tile (RT waves per
// workgroup): no cross-wave reduction, and every wave streams its tile's records and
// value windows through register rings (records 16 k-steps ahead, values 8 ahead) while
// the workgroup's B slice (NS k-steps, staged once by all waves, one barrier) stays in
// LDS.  K split: each wave publishes its 16 x N fp32 tile (8-B agent-scope stores), one
// agent-scope add per (row block, tile), the last adder sums the slabs in K-range order
// (deterministic) and stores C.
// ---------------------------------------------------------------------------
template <int CT, int RT>
__global__ __launch_bounds__(64 * RT) void k_mfma_bm2(const uint32_t *__restrict__ bmtb_first_row,  // nb+1
                                                     const uint2 *__restrict__ rec, const uint32_t *__restrict__ sbase,
                                                     const f16 *__restrict__ vals, const f16 *__restrict__ B,
                                                     f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t S,
                                                     uint32_t NS, uint32_t nwg, uint32_t row_base,
                                                     float *__restrict__ slabs, uint32_t *__restrict__ arrivals) {
    constexpr uint32_t RB = 32 * CT, UB = 2 * CT, STG = 32u * RB;
    constexpr uint32_t DR = 16, DV = 8;  // look-ahead of the records / value windows (k-steps)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);  // = this wave's row tile
    const uint32_t u = xcd_block(blockIdx.x, nwg);
    const uint32_t g = u / S, q = u - g * S;
    const uint32_t col0 = blockIdx.y * 16u * CT, nv = min(16u * CT, N - col0);
    uint2 *lut = reinterpret_cast<uint2 *>(lds);
    unsigned char *bsl = lds + 128u;  // NS k-steps of B rows
    if (tid < 16u) lut[tid] = make_uint2(bm_sel(tid, 0), bm_sel(tid, 1));
    const uint32_t k0 = q * NS * 32u;
    const size_t ub = (size_t)u * NS;
    const uint32_t tsh = 8u * (wv & 3u);  // this tile's mask byte in the record word
    auto mask_of = [&](const uint2 &r) -> uint32_t { return ((wv < 4u ? r.x : r.y) >> tsh) & 0xffu; };
    // the value offset of this lane's run for this tile: the record's lane offset + the
    // values of the lower tiles (bytes below this tile's)
    auto vstart = [&](const uint2 &r, uint32_t sb) -> uint32_t {
        uint32_t lower = wv < 4u ? (wv ? r.x & ((1u << (8u * wv)) - 1u) : 0u)
                                 : r.x;
        uint32_t p = sb + (r.y >> 16) + (uint32_t)__builtin_popcount(lower);
        if (wv >= 4u) p += (uint32_t)__builtin_popcount(r.y & ((1u << (8u * (wv - 4u))) - 1u) & 0xffffu);
        return p;
    };
    auto ld_rec = [&](uint32_t s, uint32_t &sb) -> uint2 {
        const uint32_t ss = s < NS ? s : NS - 1u;
        sb = sbase[ub + ss];
        return rec[(ub + ss) * 64u + lane];
    };
    auto ld_vals = [&](const uint2 &r, uint32_t sb, u32x2_a2 (&V)[2]) {
        const uint32_t p = vstart(r, sb), m = mask_of(r);
        V[0] = *reinterpret_cast<const u32x2_a2 *>(vals + p);
        V[1] = *reinterpret_cast<const u32x2_a2 *>(vals + p + __builtin_popcount(m & 15u));
    };
    // records of the first DR steps (the critical HBM chain) before the B slice
    uint2 rr[DR];
    uint32_t rs[DR];
#pragma unroll
    for (uint32_t j = 0; j < DR; j++) rr[j] = ld_rec(j, rs[j]);
    // B slice: step s staged by wave s % RT (registers -> ds_write_b128, b_piece permutation)
    for (uint32_t s = wv; s < NS; s += RT) {
        const uint32_t kr = k0 + s * 32u;
        u32x4 br[CT];
#pragma unroll
        for (uint32_t c = 0; c < CT; c++) {
            const uint32_t un = c * 64u + lane, k = un / UB, cu = (un % UB) * 8u;
            const uint32_t kk = kr + k < K ? kr + k : K - 1u;
            br[c] = *reinterpret_cast<const u32x4 *>(B + (size_t)kk * N + col0 + (cu < nv ? cu : 0u));
        }
#pragma unroll
        for (uint32_t c = 0; c < CT; c++) {
            const uint32_t un = c * 64u + lane, k = un / UB, sx = un % UB;
            *reinterpret_cast<u32x4 *>(bsl + s * STG + k * RB + b_piece<CT>(k, sx >> 1) * 32u + (sx & 1u) * 16u) = br[c];
        }
    }
    // the value windows of the first DV steps
    u32x2_a2 vv[DV][2];
#pragma unroll
    for (uint32_t j = 0; j < DV; j++) ld_vals(rr[j], rs[j], vv[j]);
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // the B slice and the selector table
    __asm__ volatile("" ::: "memory");
    f4v acc[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) acc[ct] = f4v{0.f, 0.f, 0.f, 0.f};
    const uint32_t kb = 8u * (lane >> 4);
    // step i (ring slots i % DR, i % DV): compute i, then refill: values of i + DV (their
    // record is in slot (i + DV) % DR), record of i + DR
    for (uint32_t i0 = 0; i0 < NS; i0 += DR) {
#pragma unroll
        for (uint32_t d = 0; d < DR; d++) {
            const uint32_t i = i0 + d;
            if (i < NS) {
                const unsigned char *bst = bsl + i * STG;
                const uint32_t m = mask_of(rr[d]);
                const uint2 sl = lut[m & 15u], sh = lut[m >> 4];
                const u32x2_a2 lo = vv[d % DV][0], hi = vv[d % DV][1];
                uint32_t w[4];
                w[0] = __builtin_amdgcn_perm(lo.y, lo.x, sl.x);
                w[1] = __builtin_amdgcn_perm(lo.y, lo.x, sl.y);
                w[2] = __builtin_amdgcn_perm(hi.y, hi.x, sh.x);
                w[3] = __builtin_amdgcn_perm(hi.y, hi.x, sh.y);
                h8v a;
                __builtin_memcpy(&a, w, 16);
#pragma unroll
                for (int ct = 0; ct < CT; ct++) {
                    s4v t2[2];
#pragma unroll
                    for (int hh = 0; hh < 2; hh++) {
                        const uint32_t k = kb + 4u * hh + ((lane & 15u) >> 2);
                        t2[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (lds_s4v *)(bst + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));
                    }
                    h8v bv;
                    __builtin_memcpy(&bv, t2, 16);
                    acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, bv, acc[ct], 0, 0, 0);
                }
            }
            // refill (past NS: re-reads of the last step, never used)
            ld_vals(rr[(d + DV) % DR], rs[(d + DV) % DR], vv[d % DV]);
            rr[d] = ld_rec(i + DR, rs[d]);
        }
    }
    const uint32_t r0 = bmtb_first_row[g], R = bmtb_first_row[g + 1] - r0;
    auto store_tile = [&](const f4v (&v)[CT]) {
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            const uint32_t col = 16u * ct + (lane & 15u);
            if (col >= nv) continue;
#pragma unroll
            for (uint32_t e = 0; e < 4; e++) {
                const uint32_t rw = 16u * wv + 4u * (lane >> 4) + e;
                if (rw < R) C[(size_t)(row_base + r0 + rw) * N + col0 + col] = (f16)v[ct][e];
            }
        }
    };
    if (S == 1) {
        store_tile(acc);
        return;
    }
    if (16u * wv >= R) return;  // a tile past the block's rows: no counter traffic
    // K split hand-off per (row block, tile, column tile)
    constexpr uint32_t TI = CT * 64u;
    const size_t tix = ((size_t)g * gridDim.y + blockIdx.y) * RT + wv;
    f4v *slab = reinterpret_cast<f4v *>(slabs) + (tix * S + q) * TI;
#pragma unroll
    for (int ct = 0; ct < CT; ct++) {
        uint64_t *dst = reinterpret_cast<uint64_t *>(slab + ct * 64u + lane);
        uint64_t w[2];
        __builtin_memcpy(w, &acc[ct], 16);
        __hip_atomic_store(dst, w[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dst + 1, w[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __asm__ volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0;
    if (lane == 0) old = __hip_atomic_fetch_add(&arrivals[tix], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != S - 1u) return;
    if (lane == 0) __hip_atomic_store(&arrivals[tix], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    f4v sum[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ct++) sum[ct] = f4v{0.f, 0.f, 0.f, 0.f};
    const f4v *base = reinterpret_cast<const f4v *>(slabs) + tix * S * TI;
    for (uint32_t qq = 0; qq < S; qq++) {
#pragma unroll
        for (int ct = 0; ct < CT; ct++) {
            if (qq == q) {
                sum[ct] += acc[ct];
            } else {
                const uint64_t *src = reinterpret_cast<const uint64_t *>(base + (size_t)qq * TI + ct * 64u + lane);
                uint64_t w[2];
                w[0] = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                w[1] = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                f4v x;
                __builtin_memcpy(&x, w, 16);
                sum[ct] += x;
            }
        }
    }
    store_tile(sum);
}

}  // namespace gsk
