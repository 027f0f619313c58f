// hip_code/mfma_ks.hpp -- k_mfma_ks: BMTB row blocks on the matrix cores with K split over
// workgroups; k_mfma_ks_group (several launches as one grid) and, in the experiments build,
// k_mfma_ks_persist.  Instantiated by kernels/ks_launch.hip; k_mfma_ks_w8 (FP8 weights) by
// kernels/ks_w8_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// k_mfma_ks -- BMTB row blocks on the matrix cores with K split over S workgroups
// and every wave running on its own (the default matrix-core kernel for row blocks of
// >= 40 rows).
// Why: a workgroup that owns a row block over all of K streams all of B (327 KB on C2)
// for its ~120 KB of A; one CU takes in ~50-70 GB/s, so B, not A, set the time
// (scripts/probes/probe_floor.hip: loading A + B alone takes 10.9 us at S = 1, 7.2 us at
// S = 4).  Here workgroup (g, q) owns row block g over the K range [q*KR, q*KR + KR) and
// reads only that slice of B (KR rows).
// Wave w owns the range's 32-column k-steps w, w+W, ... and runs them with no
// workgroup barrier until the end: per k-step it loads (D steps ahead, into registers)
// the step's 32 B rows and its entries (upload layout: the step's groups back to back,
// each 8 x [u16 halfword position in the wave's dense image] + 8 x [f16 value], found by
// the step's {first group, group count} record, loaded D steps ahead of the groups;
// padding inside a group writes 0 into the image's zero row; NT: the groups by non-temporal
// loads when NTL & 1 (KS_NT; B's rows when NTL & 2, not instantiated: slower), stores the B rows into its private stage (32-B pieces
// permuted by b_piece so the ds_read_b64_tr_b16 fragment reads are conflict-free),
// scatters the entries into its private image of 16*RT+1 rows x 96 B (conflict-free
// ds_read_b128), reads the RT A fragments and the CT B fragments, writes zeros back at
// the entries' positions, and runs RT x CT v_mfma_f32_16x16x32_f16 into fp32
// accumulators.  Every step issues the same loads (steps past the wave's last read the
// first B rows and the spare group: one cached line each), and the prologue issues them
// slot by slot in the loop's own order, so the compiler's waits stay counted ones: inside
// the loop none goes below the L * (D - 1) loads of the other slots
// (tests/test_ks_wait_counts.py).  At the end the W partial tiles are summed through LDS in wave
// order; with S > 1 each workgroup publishes its fp32 slab (16-B sc1 write-through
// stores, drained by every storing wave, then one arrival add), and the last of the row
// block's S workgroups sums the S slabs in q order (deterministic, whichever arrives
// last) and writes C: the hand-off form of MI355X_MICROARCH.md §Workgroup dispatch,
// table row 1 (sc1 stores + vmcnt(0) + barrier + one agent add; the last adder, told by
// the returned value, loads with sc1 loads after a barrier).  Workgroup order: unit
// u = g*S + q, XCD-contiguous (xcd_block), so a row block's S workgroups are normally on
// one XCD (speed only).  Rows of B past K are stored as zeros; a zero of the dense tile
// times a non-finite in-range B value gives NaN for the row block (DESIGN.md deviation,
// as for k_mfma_rows).
// ---------------------------------------------------------------------------
// s_waitcnt immediate (gfx9 encoding) waiting for vmcnt <= N only (expcnt / lgkmcnt at their maxima)
template <int N>
__device__ constexpr int vmcnt_imm() {
    static_assert(N >= 0 && N < 64, "vmcnt is six bits");
    return (N & 0xF) | ((N >> 4) << 14) | 0x70 | 0xF00;
}

// kKsStride, ks_image_bytes, ks_lds_bytes: kernel_consts.hpp

// STAMPS (diagnostic build only, gs_debug_mfma_timeline): lane 0 of every wave records
// s_memtime into stamps[(workgroup * W + wave) * 32 + slot]: 0 start, 1 loads issued,
// 3 + i after step i (i < 16), 20 loop done, 21 reduced, 22 end
// the body of k_mfma_ks for workgroup bx of a launch of nwg workgroups (k_mfma_ks: the
// whole grid; k_mfma_ks_group: one entry's share of it)
// P8 (KS_POS8, device_layout.cc pos8_step): tP holds 8 bytes per group -- byte e = bit e of the
// group's 8 x 16 segment id in bit 7, the entry's (row % 8) << 4 | column % 16 below; the image
// halfword of a segment sg's entry is 384 * (sg >> 1) + 16 * (sg & 1) + 48 * (b >> 4) + (b & 15)
// PF, the position form of a group: kKsPosU16 (8 x u16 image halfword), kKsPos8 (P8 above) or
// kKsPosWin (KS_WPOS, device_layout.cc wpos_step): tP holds 8 bytes per group and tW one byte per
// group -- the group's window w of the image (rows [5w, 5w + 5): halfwords [240w, 240w + 240)); byte e
// of tP is entry e's halfword inside the window, so an entry's LDS address is (img + 480 w) + 2 * byte:
// one base per group and two VALU per entry, kept for the clearing pass
// ET (f16 or bf16, GS_BF16 plans): the element type of A's values, B and C.  The kernel moves
// 16-bit words whatever they hold; ET selects the MFMA (mfma_elem) and the store conversion only
// epi (gs_spmm_ex's epilogue, kernel_consts.hpp): store_item applies epilogue_apply to the fp32 sum --
// after the wave reduction at S == 1, after the last ticket holder's slab combine otherwise -- and
// rounds once; the identity (the default: emitted programs, k_mfma_ks_persist) stores as before
// GS_KS_FULL_TILE (1; 0 in a variant build for the A/B): the step loop's fast iterations, see ks_body
#ifndef GS_KS_FULL_TILE
#define GS_KS_FULL_TILE 1
#endif
// GS_KS_SLOT_ORDER (1; 0 in a variant build for the A/B): the prologue's load order, see ks_body
#ifndef GS_KS_SLOT_ORDER
#define GS_KS_SLOT_ORDER 1
#endif
enum : int { kKsPosU16 = 0, kKsPos8 = 1, kKsPosWin = 2 };
// VB, the storage of A's values: 16 (8 x 16-bit ET words per group: tV as u32x4) or 8 (FP8 weights, fp16
// activations: tV holds 8 bytes per group, one OCP e4m3fn code per entry, read as u32x2 through the same
// ld_once_if choice).  ks_decode8 turns a group's 8 codes into the 4 registers of packed fp16 the 16-bit
// form loads -- every finite e4m3 value is an fp16 value, so the scatter, the fragments and the MFMAs are
// the 16-bit form's on the same numbers -- and store_item multiplies the fp32 sum of a row by w_scale[row]
// (__fmul_rn, before epilogue_apply: at S == 1 and in the last ticket holder's combine; the slabs keep
// unscaled partial sums).  w_scale is indexed as the epilogue's bias is.  ks_decode8: kernel_common.hpp
template <int CT, int RT, int W, int D, int MAXG, bool STAMPS, bool AP = true, int PF = kKsPosU16, int NTL = 0, class ET = f16,
          int VB = 16>
__device__ __forceinline__ void ks_body(const uint32_t *__restrict__ bmtb_first_row, const u32x4 *__restrict__ tP,
                                        const u32x4 *__restrict__ tV, const u32x2 *__restrict__ steps,
                                        const ET *__restrict__ B, ET *__restrict__ C, uint32_t K, uint32_t N, uint32_t S,
                                        uint32_t NS, uint32_t nwg, uint32_t row_base, float *__restrict__ slabs,
                                        uint32_t *__restrict__ arrivals, uint64_t *__restrict__ stamps, uint32_t bx,
                                        uint32_t prio, const uint8_t *__restrict__ tW = nullptr,
                                        const epilogue &epi = epilogue_identity(),
                                        const float *__restrict__ w_scale = nullptr) {
    constexpr bool P8 = PF == kKsPos8, WP = PF == kKsPosWin;
    static_assert(VB == 16 || (VB == 8 && std::is_same<ET, f16>::value), "FP8 weights decode to fp16");
    constexpr uint32_t RB = 32 * CT;  // bytes per LDS B row (a 16*CT-column tile)
    constexpr uint32_t UB = 2 * CT;   // 16-B units per B row
    constexpr uint32_t IMG = ks_image_bytes<RT>();
    constexpr uint32_t STG = 32u * RB;  // one k-step of B rows
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t u = xcd_block(bx, nwg);
    const uint32_t g = u / S, q = u - g * S;
#define GS_KS_STAMP(slot)                                                                          \
    if constexpr (STAMPS) {                                                                        \
        if (lane == 0) stamps[((size_t)blockIdx.x * W + wv) * 32u + (slot)] = __builtin_amdgcn_s_memtime(); \
    }
    GS_KS_STAMP(0u);
    const uint32_t k0 = q * NS * 32u;
    // column tile blockIdx.y: columns [col0, col0 + nv) of B and C (N > 16*CT: several
    // tiles; N = 8: one partial tile)
    const uint32_t col0 = blockIdx.y * 16u * CT, nv = min(16u * CT, N - col0);
    unsigned char *img = lds + wv * (IMG + STG);
    unsigned char *bst = img + IMG;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- this wave's k-steps w, w+W, ...: step s of unit u is record steps[u*NS + s] =
    // {first group, group count}; a slot's next record is loaded one round (D steps) before
    // its groups, so the groups' addresses wait on a load issued a round earlier
    const uint32_t nsw = NS > wv ? (NS - wv + W - 1u) / W : 0u;
    const size_t ubase = (size_t)u * NS;
    using PV = typename std::conditional<P8 || WP, u32x2, u32x4>::type;
    const PV *tPp = reinterpret_cast<const PV *>(tP);
    using VV = typename std::conditional<VB == 8, u32x2, u32x4>::type;  // a group's values as loaded
    const VV *tVp = reinterpret_cast<const VV *>(tV);
    PV P[D][MAXG];
    VV V[D][MAXG];
    u32x4 BR[D][CT];
    uint32_t WN[D][MAXG];  // WP: the groups' window bytes
    u32x2 NX[D];      // per slot: record of the step the slot loads next
    uint32_t CN[D];   // per slot: group count of the step whose groups it holds
    // the record is read by a vector load (vmcnt, in order with the groups): a scalar load
    // would share lgkmcnt with the LDS traffic, and every step's lgkmcnt(0) before its
    // fragments would then wait for the newest record as well (80% sparsity: +3-9%)
    uint32_t vz;
    __asm__ volatile("v_mov_b32 %0, 0" : "=v"(vz));
    auto rec_of = [&](uint32_t i) -> u32x2 {
        const uint32_t st = __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u);
        return steps[ubase + st + vz];
    };
    // steps past the wave's last re-read the unit's first step (cached; the same lane-varying
    // load form as a live step, so no path of the loop issues a different count).  The B rows
    // of a step need no record: they are issued apart from (and, in the prologue, before) the
    // groups, whose addresses wait for the step's record
    // FAST (the loop's fast iterations, below): all 32 rows of the step lie below K and the column
    // tile is full, so the address is a scalar row term plus the lane's offset inside a step
    uint32_t boff[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) boff[c] = ((lane + 64u * c) / UB) * N + ((lane + 64u * c) % UB) * 8u;
    auto load_b = [&](auto fast, uint32_t i, u32x4 (&B_)[CT]) {
        const uint32_t st = __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u);
        const uint32_t kr = k0 + st * 32u;  // first B row of the step
        if constexpr (decltype(fast)::value) {
            const ET *Bk = B + (size_t)kr * N + col0;
#pragma unroll
            for (int c = 0; c < CT; c++) B_[c] = ld_once_if<(NTL & 2) != 0>(reinterpret_cast<const u32x4 *>(Bk + boff[c]));
            return;
        }
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint32_t un = lane + 64u * c;  // 16-B unit of the step's 32 rows
            const uint32_t k = kr + un / UB, cu = (un % UB) * 8u;
            // columns past N (a partial column tile: N = 8, 24, ...) read column 0 and are
            // stored as zeros below
            B_[c] = ld_once_if<(NTL & 2) != 0>(
                reinterpret_cast<const u32x4 *>(B + (size_t)(k < K ? k : K - 1u) * N + col0 + (cu < nv ? cu : 0u)));
        }
    };
    // the groups of step i (b0: first group, gc: count), then the record of step i + D
    auto load_g_at = [&](uint32_t i, uint32_t b0, uint32_t gc, u32x2 &NX_, uint32_t &CN_, PV (&P_)[MAXG],
                         VV (&V_)[MAXG], uint32_t (&W_)[MAXG]) {
        CN_ = gc;
        NX_ = rec_of(i + D);
#pragma unroll
        for (int j = 0; j < MAXG; j++) {
            const uint32_t qg = lane + 64u * j;
            const size_t at = (size_t)b0 + (qg < gc ? qg : 0u);
            P_[j] = ld_once_if<(NTL & 1) != 0>(tPp + at);
            V_[j] = ld_once_if<(NTL & 1) != 0>(tVp + at);
            if constexpr (WP) W_[j] = ld_once_if<(NTL & 1) != 0>(tW + at);
        }
    };
    auto load_g = [&](uint32_t i, u32x2 &NX_, uint32_t &CN_, PV (&P_)[MAXG], VV (&V_)[MAXG], uint32_t (&W_)[MAXG]) {
        load_g_at(i, __builtin_amdgcn_readfirstlane(NX_[0]), __builtin_amdgcn_readfirstlane(NX_[1]), NX_, CN_, P_, V_, W_);
    };
    // head steps (device_layout.cc ks_tiles::GH, prio bits 8..17): the first D steps of every wave
    // sit at (unit * min(W * D, NS) + step) * GH, padded with zero-row groups, so the prologue issues their
    // groups with the B rows at once instead of a record round trip later
    const uint32_t GH = (prio >> 8) & 0x3ffu;
    // GS_KS_SLOT_ORDER: both forms issue slot by slot in the step loop's own order -- a slot's B rows,
    // its next record, its groups -- with scheduling barriers between the slots, so the queue at the
    // loop's header is the steady state's and the loop's waits leave the other slots' loads in flight
    if (GS_KS_SLOT_ORDER && GH) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t st = (uint32_t)d < nsw ? wv + (uint32_t)d * W : 0u;
            load_b(std::false_type{}, (uint32_t)d, BR[d]);
            __builtin_amdgcn_sched_barrier(0);
            load_g_at((uint32_t)d, (u * min((uint32_t)(W * D), NS) + st) * GH, GH, NX[d], CN[d], P[d], V[d], WN[d]);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
        __builtin_amdgcn_sched_barrier(0);
    } else if (GS_KS_SLOT_ORDER) {
#pragma unroll
        for (int d = 0; d < D; d++) NX[d] = rec_of((uint32_t)d);
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
#pragma unroll
        for (int d = 0; d < D; d++) {
            __builtin_amdgcn_sched_barrier(0);
            load_b(std::false_type{}, (uint32_t)d, BR[d]);
            __builtin_amdgcn_sched_barrier(0);
            load_g((uint32_t)d, NX[d], CN[d], P[d], V[d], WN[d]);
        }
        __builtin_amdgcn_sched_barrier(0);
    } else if (GH) {
#pragma unroll
        for (int d = 0; d < D; d++) load_b(std::false_type{}, (uint32_t)d, BR[d]);
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t st = (uint32_t)d < nsw ? wv + (uint32_t)d * W : 0u;
            load_g_at((uint32_t)d, (u * min((uint32_t)(W * D), NS) + st) * GH, GH, NX[d], CN[d], P[d], V[d], WN[d]);
        }
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
    } else {
#pragma unroll
        for (int d = 0; d < D; d++) NX[d] = rec_of((uint32_t)d);
#pragma unroll
        for (int d = 0; d < D; d++) load_b(std::false_type{}, (uint32_t)d, BR[d]);
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
#pragma unroll
        for (int d = 0; d < D; d++) load_g((uint32_t)d, NX[d], CN[d], P[d], V[d], WN[d]);
    }
    GS_KS_STAMP(1u);

    f4v acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    uint32_t arow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) arow[rt] = (16u * rt + (lane & 15u)) * kKsStride + 16u * (lane >> 4);

    // step i on its set, then the set is reloaded with step i + D (issued whether or not
    // step i exists: every loop iteration issues the same loads)
    // image halfword of entry e of a group (u16 position, or P8's segment + 7-bit position)
    auto ent_h = [&](const PV &p, uint32_t hb, int e) -> uint32_t {
        if constexpr (P8) {
            const uint32_t b = (p[e >> 2] >> (8 * (e & 3))) & 0x7fu;
            return hb + 48u * (b >> 4) + (b & 15u);
        } else {
            return (p[e >> 1] >> (16 * (e & 1))) & 0xffffu;
        }
    };
    auto grp_hb = [&](const PV &p) -> uint32_t {
        if constexpr (P8) {
            const uint32_t x = p[0], y = p[1];
            const uint32_t sg = ((x >> 7) & 1u) | ((x >> 14) & 2u) | ((x >> 21) & 4u) | ((x >> 28) & 8u) | ((y >> 3) & 16u);
            return 384u * (sg >> 1) + 16u * (sg & 1u);
        } else {
            return 0u;
        }
    };
    auto step = [&](auto fast, uint32_t i, u32x2 &NX_, uint32_t &CN_, PV (&P_)[MAXG], VV (&V_)[MAXG], u32x4 (&B_)[CT],
                    uint32_t (&W_)[MAXG]) {
        const bool live = i < nsw;  // wave-uniform
        const uint32_t gc = CN_;
        typedef typename mfma_elem<ET>::frag frag;
        frag av[RT], bv[CT];
        if (live) {
            const uint32_t kr = k0 + (wv + i * W) * 32u;
            // the step's B rows into the stage (rows past K as zeros)
#pragma unroll
            for (int c = 0; c < CT; c++) {
                const uint32_t un = lane + 64u * c, k = un / UB, s = un % UB;
                u32x4 b = B_[c];
                if constexpr (!decltype(fast)::value) b = kr + k < K && s * 8u < nv ? b : zero4;
                *reinterpret_cast<u32x4 *>(bst + k * RB + b_piece<CT>(k, s >> 1) * 32u + (s & 1u) * 16u) = b;
            }
            // WP: the entries' LDS addresses, once for the scatter and the clearing pass (lanes past
            // the step's groups hold its first group: addresses inside the image all the same)
            unsigned char *wa[WP ? MAXG : 1][8];
            if constexpr (WP) {
#pragma unroll
                for (int j = 0; j < MAXG; j++) {
                    unsigned char *wb = img + W_[j] * 480u;
#pragma unroll
                    for (int e = 0; e < 8; e++) wa[j][e] = wb + 2u * ((P_[j][e >> 2] >> (8 * (e & 3))) & 0xffu);
                }
            }
            // scatter the step's entries into the image
#pragma unroll
            for (int j = 0; j < MAXG; j++) {
                if (lane + 64u * j < gc) {
                    const uint32_t hb = grp_hb(P_[j]);
                    const auto &gv = ks_group_values<VB>(V_[j]);  // the group's 8 values as 16-bit words
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const uint16_t v = (uint16_t)((gv[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                        if constexpr (WP) {
                            *reinterpret_cast<uint16_t *>(wa[j][e]) = v;
                        } else {
                            const uint32_t h = ent_h(P_[j], hb, e);
                            *reinterpret_cast<uint16_t *>(img + h * 2u) = v;
                        }
                    }
                }
            }
            // fragments (LDS runs a wave's operations in order: the reads see the stores)
#pragma unroll
            for (int rt = 0; rt < RT; rt++) av[rt] = *reinterpret_cast<const frag *>(img + arow[rt]);
            const uint32_t kb = 8u * (lane >> 4);
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                s4v t[2];
#pragma unroll
                for (int hh = 0; hh < 2; hh++) {
                    const uint32_t k = kb + 4u * hh + ((lane & 15u) >> 2);
                    t[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (lds_s4v *)(bst + k * RB + b_piece<CT>(k, ct) * 32u + (lane & 3u) * 8u));
                }
                __builtin_memcpy(&bv[ct], t, 16);
            }
            // the image back to zero at the entries' positions
#pragma unroll
            for (int j = 0; j < MAXG; j++) {
                if (lane + 64u * j < gc) {
                    const uint32_t hb = grp_hb(P_[j]);
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        if constexpr (WP) *reinterpret_cast<uint16_t *>(wa[j][e]) = (uint16_t)0;
                        else *reinterpret_cast<uint16_t *>(img + ent_h(P_[j], hb, e) * 2u) = (uint16_t)0;
                    }
                }
            }
        }
        load_b(fast, i + D, B_);
        load_g(i + D, NX_, CN_, P_, V_, W_);
        if (live) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[rt][ct] = mfma_elem<ET>::mfma_16x16x32(av[rt], bv[ct], acc[rt][ct]);
            if (i < 16u) GS_KS_STAMP(3u + i);
        }
    };
    // prio (KS_PRIO): the younger half of the waves (the second wave of each SIMD, the one
    // that loses issue arbitration) at s_setprio 1 -- prio & 3 = 1: for its whole loop, 2: for the
    // first half of its steps
    const bool young = wv >= W / 2u;
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(1);
    // Fast iterations: every k-step an iteration runs or loads for has its 32 B rows below K, on a full
    // column tile -- the B rows are stored without the zero selects and loaded at a scalar row term +
    // the lane's offset.  Only the last K range of a K that is no multiple of 32 has a short step, the
    // last one; its waves run their last iterations in the general form.  fsp: the range's full steps
    // (step st is full when st < fsp); a step past the wave's last reads step 0
    const uint32_t fsp = min(NS, K > k0 ? (K - k0) / 32u : 0u);
    const uint32_t nfull = fsp > wv ? (fsp - wv + W - 1u) / W : 0u;  // this wave's full steps
    uint32_t fast_end = 0;
    if (GS_KS_FULL_TILE && nv == 16u * CT)
        fast_end = fsp == NS ? nsw : (nfull >= 2u * D ? ((nfull - 2u * D) / D + 1u) * D : 0u);
    fast_end = __builtin_amdgcn_readfirstlane(fast_end);
    uint32_t i0 = 0;
    for (; i0 < fast_end; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(std::true_type{}, i0 + d, NX[d], CN[d], P[d], V[d], BR[d], WN[d]);
        if ((prio & 3u) == 2u && young && i0 + D >= nsw / 2u && i0 < nsw / 2u) __builtin_amdgcn_s_setprio(0);
    }
    for (; i0 < nsw; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(std::false_type{}, i0 + d, NX[d], CN[d], P[d], V[d], BR[d], WN[d]);
        if ((prio & 3u) == 2u && young && i0 + D >= nsw / 2u && i0 < nsw / 2u) __builtin_amdgcn_s_setprio(0);
    }
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(0);
    GS_KS_STAMP(20u);
    // ---- K-split ticket: wave 0 takes its row block's arrival ticket as soon as its own
    // loop ends, so the add's round trip overlaps the partial-tile reduction below
    uint32_t *arr = arrivals + (size_t)g * gridDim.y + blockIdx.y;
    uint32_t ticket = 0;
    if (S > 1 && wv == 0 && lane == 0) ticket = __hip_atomic_fetch_add(arr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- wave partial tiles -> LDS (the trailing loads write registers only), summed in
    // wave order.  Item t = (tile, lane) of a 16x16 tile: the 4 rows 4*(lane/16)+i of
    // column lane%16.  When the W partial tiles fit LDS beside the wave images (APART), each
    // wave stores its tile as soon as its loop ends, without waiting for the others
    constexpr bool APART = ks_red_apart(CT, RT, W, AP);
    f4v *red = reinterpret_cast<f4v *>(lds + (APART ? (size_t)W * (IMG + STG) : 0u));
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
    // a launch with an epilogue (kernel arguments: a wave-uniform branch, after the step loop and
    // the K-range combine; the identity takes the plain stores)
    const bool fused = !epilogue_is_identity(epi);
    auto store_item = [&](uint32_t t, const f4v &v) {
        const uint32_t ln = t & 63u, tt = t >> 6, rt = tt / CT, ct = tt % CT;
        const uint32_t col = 16u * ct + (ln & 15u), rb = 16u * rt + 4u * (ln >> 4);
        if (col >= nv) return;
        if constexpr (VB == 8) {  // FP8 weights: the row's scale on the fp32 sum first, then as below
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (rb + i < R) {
                    const size_t row = (size_t)(row_base + r0 + rb + i), at = row * N + col0 + col;
                    float o = __fmul_rn(w_scale[row], v[i]);
                    if (fused) {
                        const float res = epi.residual ? (float)static_cast<const ET *>(epi.residual)[at] : 0.f;
                        o = epilogue_apply(epi, o, row, res);
                    }
                    C[at] = (ET)o;
                }
            return;
        }
        if (fused) {  // the launch's epilogue on the fp32 sum, rounded once (epilogue_apply)
#pragma unroll
            for (uint32_t i = 0; i < 4; i++)
                if (rb + i < R) {
                    const size_t row = (size_t)(row_base + r0 + rb + i), at = row * N + col0 + col;
                    const float res = epi.residual ? (float)static_cast<const ET *>(epi.residual)[at] : 0.f;
                    C[at] = (ET)epilogue_apply(epi, v[i], row, res);
                }
            return;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (rb + i < R) C[(size_t)(row_base + r0 + rb + i) * N + col0 + col] = (ET)v[i];
    };
    GS_KS_STAMP(21u);
    if (S == 1) {
        for (uint32_t t = tid; t < NI; t += NT) store_item(t, item_sum(t));
        GS_KS_STAMP(22u);
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
        GS_KS_STAMP(22u);
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
    GS_KS_STAMP(22u);
#undef GS_KS_STAMP
}

template <int CT, int RT, int W, int D, int MAXG, bool STAMPS = false, bool AP = true, int PF = kKsPosU16, int NTL = 0, class ET = f16>
__global__ __launch_bounds__(64 * W) void k_mfma_ks(const uint32_t *__restrict__ bmtb_first_row,  // nb+1
                                                    const u32x4 *__restrict__ tP,  // 8 x u16 position per group (PF)
                                                    const u32x4 *__restrict__ tV,  // 8 x 16-bit value (ET) per group
                                                    const u32x2 *__restrict__ steps,  // per (unit, k-step): first group, count
                                                    const ET *__restrict__ B, ET *__restrict__ C, uint32_t K,
                                                    uint32_t N, uint32_t S, uint32_t NS, uint32_t nwg,
                                                    uint32_t row_base, float *__restrict__ slabs,
                                                    uint32_t *__restrict__ arrivals, uint64_t *__restrict__ stamps = nullptr,
                                                    uint32_t prio = 0,
                                                    const uint8_t *__restrict__ tW = nullptr,  // kKsPosWin: window byte per group
                                                    epilogue epi = epilogue_identity()) {  // applied in store_item
    // nwg == gridDim.x (an argument: kernarg preload)
    ks_body<CT, RT, W, D, MAXG, STAMPS, AP, PF, NTL, ET>(bmtb_first_row, tP, tV, steps, B, C, K, N, S, NS, nwg, row_base, slabs,
                                                    arrivals, stamps, blockIdx.x, prio, tW, epi);
}

// k_mfma_ks_w8 -- k_mfma_ks on a plan uploaded with FP8 weights (ks_body's VB = 8): the release layout
// (fp16 activations, the apart layout, 16-bit positions, no stamps) and one more argument, the rows'
// scales.  A kernel of its own name: the value storage and the scale pointer reach these instantiations
// only, and every k_mfma_ks instantiation keeps its template arguments, its parameters and its symbol
template <int CT, int RT, int W, int D, int MAXG, int NTL = 0>
__global__ __launch_bounds__(64 * W) void k_mfma_ks_w8(const uint32_t *__restrict__ bmtb_first_row,  // nb+1
                                                       const u32x4 *__restrict__ tP,  // 8 x u16 position per group
                                                       const u32x2 *__restrict__ tV,  // 8 x e4m3 code per group
                                                       const u32x2 *__restrict__ steps, const f16 *__restrict__ B,
                                                       f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t S, uint32_t NS,
                                                       uint32_t nwg, uint32_t row_base, float *__restrict__ slabs,
                                                       uint32_t *__restrict__ arrivals, uint32_t prio, epilogue epi,
                                                       const float *__restrict__ w_scale) {  // one per row of A
    ks_body<CT, RT, W, D, MAXG, false, true, kKsPosU16, NTL, f16, 8>(bmtb_first_row, tP, reinterpret_cast<const u32x4 *>(tV), steps,
                                                                    B, C, K, N, S, NS, nwg, row_base, slabs, arrivals, nullptr,
                                                                    blockIdx.x, prio, nullptr, epi, w_scale);
}

#ifdef GS_EXPERIMENTS
// ---------------------------------------------------------------------------
// k_mfma_ks_persist (KS_PERSIST = the grid): a persistent grid over
// the plan's units (row block, K range) -- workgroup b runs unit b, then units pulled from its
// XCD's head (queue[xcc]: unit grid + xcc + 8 n), until the units run out.  The pull for the next
// unit is issued as the current one starts (its round trip overlaps the unit's first loads);
// the units' K-range combine is k_mfma_ks's (tickets + tagged slabs in q order), so C is the
// same bits as the static launch's whichever workgroup runs a unit.  The last workgroup out
// re-arms the nine queue words (8 heads + the exit count).
// ---------------------------------------------------------------------------
template <int CT, int RT, int W, int D, int MAXG, int NTL = 0>
__global__ __launch_bounds__(64 * W) void k_mfma_ks_persist(const uint32_t *__restrict__ bmtb_first_row,
                                                            const u32x4 *__restrict__ tP, const u32x4 *__restrict__ tV,
                                                            const u32x2 *__restrict__ steps, const f16 *__restrict__ B,
                                                            f16 *__restrict__ C, uint32_t K, uint32_t N, uint32_t S,
                                                            uint32_t NS, uint32_t nunits, uint32_t row_base,
                                                            float *__restrict__ slabs, uint32_t *__restrict__ arrivals,
                                                            uint32_t prio, uint32_t *__restrict__ queue) {
    __shared__ uint32_t next_sh;
    uint32_t xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID, 0, 4)" : "=s"(xcc));
    xcc &= 7u;
    const uint32_t grid = gridDim.x;
    uint32_t u = blockIdx.x, qx = xcc, tried = 0;
    while (u < nunits) {
        uint32_t pulled = 0;
        if (threadIdx.x == 0) pulled = __hip_atomic_fetch_add(queue + qx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ks_body<CT, RT, W, D, MAXG, false, true, kKsPosU16, NTL>(bmtb_first_row, tP, tV, steps, B, C, K, N, S, NS, nunits,
                                                          row_base, slabs, arrivals, nullptr, u, prio);
        __syncthreads();
        if (threadIdx.x == 0) next_sh = pulled;
        __syncthreads();
        u = grid + qx + 8u * next_sh;
        __syncthreads();
        // this XCD's units are done: take the other heads' in turn (correct whatever the placement)
        while (u >= nunits && ++tried < 8u) {
            qx = (qx + 1u) & 7u;
            if (threadIdx.x == 0) next_sh = __hip_atomic_fetch_add(queue + qx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            u = grid + qx + 8u * next_sh;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0 && __hip_atomic_fetch_add(queue + 8, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == grid - 1u) {
        for (int i = 0; i < 9; i++) __hip_atomic_store(queue + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#endif  // GS_EXPERIMENTS (k_mfma_ks_persist)

// ---------------------------------------------------------------------------
// k_mfma_ks_group -- several k_mfma_ks launches of one instantiation as one grid (a layer's
// or a batch's SpMMs; gs_spmm_batch): entry i owns workgroups [begin[i], begin[i] + nwg_i) and
// runs them as its own launch would (begin[i] a multiple of 8: the entry's block numbers keep
// the XCD residues xcd_block assumes; the blocks up to begin[i+1] exit at once).  One launch instead of one per matrix: no kernel boundary
// between the matrices, and one matrix's last workgroups overlap the next one's first.  The
// entries are kernel arguments (ks_group_args, read through the kernarg segment with scalar
// loads); every entry has its own plan replica (distinct K-range tickets and slabs).
// ---------------------------------------------------------------------------
struct ks_entry {  // 120 B
    const uint32_t *tbr;
    const u32x4 *tP, *tV;
    const u32x2 *steps;
    const void *B;  // the instantiation's element type (k_mfma_ks_group ET)
    void *C;
    float *slabs;
    uint32_t *arrivals;
    uint32_t K, S, NS, nwg, row_base, pad0;  // pad0: the entry's head-step group count
    const uint8_t *tW;  // kKsPosWin: window byte per group
    epilogue epi;       // the entry's epilogue (the identity: plain stores)
};
static_assert(sizeof(ks_entry) == 120, "ks_entry is 120 bytes");
// kKsGroupMax: kernel_consts.hpp
struct ks_group_args {
    uint32_t begin[kKsGroupMax + 1];  // first workgroup of each entry (+ the total)
    uint32_t n, N, pad[2];  // pad[0]: k_mfma_ks's prio
    ks_entry e[kKsGroupMax];
};
static_assert(sizeof(ks_group_args) <= 4096, "ks_group_args must fit the 4 KB kernarg segment");

template <int CT, int RT, int W, int D, int MAXG, int PF = kKsPosU16, bool AP = true, int NTL = 0, class ET = f16>
__global__ __launch_bounds__(64 * W) void k_mfma_ks_group(ks_group_args args) {
    const uint32_t bx = blockIdx.x, n = args.n;
    uint32_t sel = 0;
#pragma unroll
    for (int i = 1; i < kKsGroupMax; i++)
        if ((uint32_t)i < n && args.begin[i] <= bx) sel = (uint32_t)i;
    sel = __builtin_amdgcn_readfirstlane(sel);
    const ks_entry &e = args.e[sel];  // kernel arguments: scalar loads at a computed offset
    if (bx - args.begin[sel] >= e.nwg) return;  // padding up to the next entry's multiple of 8
    ks_body<CT, RT, W, D, MAXG, false, AP, PF, NTL, ET>(e.tbr, e.tP, e.tV, e.steps, (const ET *)e.B, (ET *)e.C, e.K, args.N, e.S, e.NS,
                                                   e.nwg, e.row_base, e.slabs, e.arrivals, nullptr, bx - args.begin[sel],
                                                   args.pad[0] | (e.pad0 << 8), e.tW, e.epi);
}

}  // namespace gsk
