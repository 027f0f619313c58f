// hip_code/mfma_ks_tm.hpp -- k_mfma_ks_tm: k_mfma_ks with token-major activations, Y = X * A^T
// (gs_linear).  Instantiated by kernels/ks_tm_launch.hip; with FP8 weights (VB = 8) by
// kernels/ks_tm_w8_launch.hip.  And k_mfma_ks_tm_group: several such launches as one grid (gs_linear_batch),
// instantiated by kernels/ks_tm_group_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// ---------------------------------------------------------------------------
// k_mfma_ks_tm -- an uploaded k_mfma_ks plan (mfma_ks.hpp: the same tP / tV / steps arrays, head
// steps, KS_NT, slabs, arrival counters, tags, device error word and xcd_block order; 32-token
// tiles, 16-bit positions, the release layout) run on X: N x K and Y: N x M, both row-major -- one
// row per token, as a linear layer under PyTorch holds its activations -- instead of B: K x N and
// C: M x N.
// The same as ks_body: workgroup (g, q) owns row block g over K range q; wave w owns the k-steps
// w, w+W, ... and loads D steps ahead; the entries are scattered into the wave's dense image, the RT
// A fragments read from it and the image cleared at the entries' positions; RT x 2 MFMAs per k-step;
// the W partial tiles are summed through LDS in wave order; with S > 1 the ticket, the tagged slabs
// and the last ticket holder's combine in q order (ks_slab_wait).  The MFMAs, their order and the
// order of every sum are k_mfma_ks's, so Y is bit for bit the transpose of its C.
// Any token count N >= 1: T = ceil(N / 32) token tiles in one launch, the last one partial; a tile's
// workgroups see nothing of the others', so row t of Y does not depend on N nor on where token t
// stands.  With S > 1 the slabs and the arrival counters are laid out by T (slab of (unit, tile) at
// u * T + tile, counter of (row block, tile) at g * T + tile, the error word behind the nb * T
// counters): the caller passes state of that layout (ks_tm_launch.hip, gs_linear).
// What differs:
// - B side.  The MFMA's B operand of lane l is column l % 16, k = 8 * (l / 16) .. + 7: with X[n][k] these
//   are 16 contiguous bytes of token col0 + 16 * ct + l % 16 at k0 + 32 * st + 8 * (l / 16), loaded from
//   global memory into the registers the MFMA reads (BR[D][CT], D steps ahead).  No B stage in LDS, no
//   transposing read.  The launch needs K % 8 == 0 and X 16-byte aligned, so a 16-byte unit is
//   aligned and lies wholly below K or wholly past it; a unit past K loads the row's first unit
//   instead and reaches the MFMA as zeros (the image's zero times a stray NaN would poison the row
//   block); a token past N in a partial tile loads the tile's first token, and its accumulators are
//   never stored.  Every step issues the same loads (a step past the wave's last re-reads the
//   range's first), so the waits stay counted ones, as in ks_body.
// - C side.  A lane's 4 accumulators are rows rb .. rb + 3 of one token: contiguous in Y[n][m].  One
//   8-byte store where all four rows exist and the address is 8-byte aligned (a lane's own decision),
//   2-byte stores otherwise.  epilogue_apply on the fp32 sum as in ks_body's store_item: bias[row] is
//   per output feature, the residual is read token-major at Y's index; one rounding.
// LDS: the W images, then the W partial tiles (kernel_consts.hpp ks_tm_lds_bytes).
// VB is ks_body's (mfma_ks.hpp): 16, or 8 for a plan uploaded with FP8 weights (fp16 activations) -- tV
// holds 8 e4m3 codes per group, decoded by ks_decode8 into the registers the scatter reads, and
// store_item multiplies the fp32 sum of a row by its scale before the epilogue; everything else, the
// K-split state included, is the 16-bit form's.  WS: the instantiations with VB = 8 -- and only they --
// take one more argument, `const float *` scales, one per row of A (indexed as the bias is); the body
// stays in the kernel (moved into a function, the 16-bit instantiations allocate registers differently)
// ---------------------------------------------------------------------------
__device__ __forceinline__ const float *ks_scale_arg() { return nullptr; }
__device__ __forceinline__ const float *ks_scale_arg(const float *p) { return p; }
template <int RT, int W, int D, int MAXG, int NTL = 0, class ET = f16, int VB = 16, class... WS>
__global__ __launch_bounds__(64 * W) void k_mfma_ks_tm(const uint32_t *__restrict__ bmtb_first_row,  // nb+1
                                                       const u32x4 *__restrict__ tP,  // 8 x u16 position per group
                                                       const u32x4 *__restrict__ tV,  // 8 x 16-bit value (ET) per group; VB = 8: 8 bytes
                                                       const u32x2 *__restrict__ steps,  // per (unit, k-step): first group, count
                                                       const ET *__restrict__ X, ET *__restrict__ Y, uint32_t K,
                                                       uint32_t N, uint32_t M, uint32_t S, uint32_t NS, uint32_t nwg,
                                                       uint32_t row_base, float *__restrict__ slabs,
                                                       uint32_t *__restrict__ arrivals, uint32_t prio, epilogue epi,
                                                       WS... w_scale_arg) {
    static_assert(VB == 16 ? sizeof...(WS) == 0 : (VB == 8 && sizeof...(WS) == 1 && std::is_same<ET, f16>::value),
                  "16-bit values, or FP8 weights (fp16 activations) with the rows' scales as the last argument");
    constexpr int CT = 2;
    constexpr uint32_t IMG = ks_image_bytes<RT>();
    static_assert(!ks_red_halves(CT, RT, W), "the W partial tiles fit LDS");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // T token tiles per unit on a 1-D grid of nwg * T workgroups (T in prio's bits 18..31; 0 reads as 1):
    // unit-major, v = u * T + tile, so the T tiles of one unit are neighbours in dispatch order on one
    // XCD and share the unit's A stream through that L2.  T = 1: v = u, the grid of before
    const uint32_t T = max(prio >> 18, 1u);
    uint32_t u = xcd_block(blockIdx.x, nwg * T), tile = 0;
    if (T > 1u) {
        const uint32_t v = u;
#if defined(GS_EXPERIMENTS) && defined(GS_KS_TM_TILE_MAJOR)  // A/B: all units of tile 0, then tile 1, ...
        tile = v / nwg;
        u = v - tile * nwg;
#else
        u = v / T;
        tile = v - u * T;
#endif
    }
    const uint32_t g = u / S, q = u - g * S;
    const uint32_t k0 = q * NS * 32u;
    // token tile `tile`: tokens [col0, col0 + nv) of X and Y (N = 24: one partial tile)
    const uint32_t col0 = tile * 16u * CT, nv = min(16u * CT, N - col0);
    unsigned char *img = lds + wv * IMG;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- this wave's k-steps w, w+W, ... (records, groups and head steps as in ks_body)
    const uint32_t nsw = NS > wv ? (NS - wv + W - 1u) / W : 0u;
    const size_t ubase = (size_t)u * NS;
    using VV = typename std::conditional<VB == 8, u32x2, u32x4>::type;  // a group's values as loaded
    const VV *tVp = reinterpret_cast<const VV *>(tV);
    u32x4 P[D][MAXG], BR[D][CT];
    VV V[D][MAXG];
    u32x2 NX[D];     // per slot: record of the step the slot loads next
    uint32_t CN[D];  // per slot: group count of the step whose groups it holds
    uint32_t vz;
    __asm__ volatile("v_mov_b32 %0, 0" : "=v"(vz));
    auto rec_of = [&](uint32_t i) -> u32x2 {
        const uint32_t st = __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u);
        return steps[ubase + st + vz];
    };
    // the lane's 16-byte unit of a k-step: token 16 * c + lane % 16 of the tile, k = 8 * (lane / 16) .. + 7
    const uint32_t ku = 8u * (lane >> 4);
    // FAST (the loop's fast iterations, below): the step's 32 columns of X lie below K, so the address
    // is a scalar k term plus the lane's offset; the offset of a token past N in a partial tile is the
    // tile's first token's (its accumulators are never stored)
    uint32_t xoff[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const uint32_t tk = 16u * c + (lane & 15u);
        xoff[c] = (tk < nv ? tk : 0u) * K + ku;
    }
    auto load_b = [&](auto fast, uint32_t i, u32x4 (&B_)[CT]) {
        const uint32_t st = __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u);
        const uint32_t kr = k0 + st * 32u;  // first column of X of the step
        if constexpr (decltype(fast)::value) {
            const ET *Xk = X + (size_t)col0 * K + kr;
#pragma unroll
            for (int c = 0; c < CT; c++) B_[c] = *reinterpret_cast<const u32x4 *>(Xk + xoff[c]);
            return;
        }
        // a unit past K reads the row's first unit (zeroed in step); a token past N the tile's first
        const uint32_t kc = kr + ku < K ? kr + ku : 0u;
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint32_t tk = 16u * c + (lane & 15u);
            B_[c] = *reinterpret_cast<const u32x4 *>(X + (size_t)(col0 + (tk < nv ? tk : 0u)) * K + kc);
        }
    };
    // the groups of step i (b0: first group, gc: count), then the record of step i + D
    auto load_g_at = [&](uint32_t i, uint32_t b0, uint32_t gc, u32x2 &NX_, uint32_t &CN_, u32x4 (&P_)[MAXG],
                         VV (&V_)[MAXG]) {
        CN_ = gc;
        NX_ = rec_of(i + D);
#pragma unroll
        for (int j = 0; j < MAXG; j++) {
            const uint32_t qg = lane + 64u * j;
            const size_t at = (size_t)b0 + (qg < gc ? qg : 0u);
            P_[j] = ld_once_if<(NTL & 1) != 0>(tP + at);
            V_[j] = ld_once_if<(NTL & 1) != 0>(tVp + at);
        }
    };
    auto load_g = [&](uint32_t i, u32x2 &NX_, uint32_t &CN_, u32x4 (&P_)[MAXG], VV (&V_)[MAXG]) {
        load_g_at(i, __builtin_amdgcn_readfirstlane(NX_[0]), __builtin_amdgcn_readfirstlane(NX_[1]), NX_, CN_, P_, V_);
    };
    // the prologue issues slot by slot in the step loop's own order (ks_body, GS_KS_SLOT_ORDER)
    const uint32_t GH = (prio >> 8) & 0x3ffu;  // groups per head step (0: every step by record)
    if (GH) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t st = (uint32_t)d < nsw ? wv + (uint32_t)d * W : 0u;
            load_b(std::false_type{}, (uint32_t)d, BR[d]);
            __builtin_amdgcn_sched_barrier(0);
            load_g_at((uint32_t)d, (u * min((uint32_t)(W * D), NS) + st) * GH, GH, NX[d], CN[d], P[d], V[d]);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
        __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
        for (int d = 0; d < D; d++) NX[d] = rec_of((uint32_t)d);
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
#pragma unroll
        for (int d = 0; d < D; d++) {
            __builtin_amdgcn_sched_barrier(0);
            load_b(std::false_type{}, (uint32_t)d, BR[d]);
            __builtin_amdgcn_sched_barrier(0);
            load_g((uint32_t)d, NX[d], CN[d], P[d], V[d]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    f4v acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    uint32_t arow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) arow[rt] = (16u * rt + (lane & 15u)) * kKsStride + 16u * (lane >> 4);

    // step i on its set, then the set is reloaded with step i + D (issued whether or not step i
    // exists: every loop iteration issues the same loads)
    auto ent_h = [&](const u32x4 &p, int e) -> uint32_t { return (p[e >> 1] >> (16 * (e & 1))) & 0xffffu; };
    auto step = [&](auto fast, uint32_t i, u32x2 &NX_, uint32_t &CN_, u32x4 (&P_)[MAXG], VV (&V_)[MAXG], u32x4 (&B_)[CT]) {
        const bool live = i < nsw;  // wave-uniform
        const uint32_t gc = CN_;
        typedef typename mfma_elem<ET>::frag frag;
        frag av[RT], bv[CT];
        if (live) {
            // scatter the step's entries into the image
#pragma unroll
            for (int j = 0; j < MAXG; j++) {
                if (lane + 64u * j < gc) {
                    const auto &gv = ks_group_values<VB>(V_[j]);  // the group's 8 values as 16-bit words
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const uint16_t v = (uint16_t)((gv[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                        *reinterpret_cast<uint16_t *>(img + ent_h(P_[j], e) * 2u) = v;
                    }
                }
            }
            // A fragments (LDS runs a wave's operations in order: the reads see the stores)
#pragma unroll
            for (int rt = 0; rt < RT; rt++) av[rt] = *reinterpret_cast<const frag *>(img + arow[rt]);
            // the image back to zero at the entries' positions
#pragma unroll
            for (int j = 0; j < MAXG; j++) {
                if (lane + 64u * j < gc) {
#pragma unroll
                    for (int e = 0; e < 8; e++) *reinterpret_cast<uint16_t *>(img + ent_h(P_[j], e) * 2u) = (uint16_t)0;
                }
            }
            // B fragments: the loaded units as they are (a unit past K as zeros)
            const uint32_t kr = k0 + (wv + i * W) * 32u;
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                u32x4 b = B_[ct];
                if constexpr (!decltype(fast)::value) b = kr + ku < K ? b : zero4;
                __builtin_memcpy(&bv[ct], &b, 16);
            }
        }
        load_b(fast, i + D, B_);
        load_g(i + D, NX_, CN_, P_, V_);
        if (live) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[rt][ct] = mfma_elem<ET>::mfma_16x16x32(av[rt], bv[ct], acc[rt][ct]);
        }
    };
    // prio (KS_PRIO), the fast iterations (fsp, nfull, fast_end): ks_body's
    const bool young = wv >= W / 2u;
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(1);
    const uint32_t fsp = min(NS, K > k0 ? (K - k0) / 32u : 0u);
    const uint32_t nfull = fsp > wv ? (fsp - wv + W - 1u) / W : 0u;  // this wave's full steps
    uint32_t fast_end = fsp == NS ? nsw : (nfull >= 2u * D ? ((nfull - 2u * D) / D + 1u) * D : 0u);
    fast_end = __builtin_amdgcn_readfirstlane(fast_end);
    uint32_t i0 = 0;
    for (; i0 < fast_end; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(std::true_type{}, i0 + d, NX[d], CN[d], P[d], V[d], BR[d]);
        if ((prio & 3u) == 2u && young && i0 + D >= nsw / 2u && i0 < nsw / 2u) __builtin_amdgcn_s_setprio(0);
    }
    for (; i0 < nsw; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(std::false_type{}, i0 + d, NX[d], CN[d], P[d], V[d], BR[d]);
        if ((prio & 3u) == 2u && young && i0 + D >= nsw / 2u && i0 < nsw / 2u) __builtin_amdgcn_s_setprio(0);
    }
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(0);
    // ---- K-split ticket, taken as soon as wave 0's loop ends (ks_body)
    uint32_t *arr = arrivals + (size_t)g * T + tile;
    uint32_t ticket = 0;
    if (S > 1 && wv == 0 && lane == 0) ticket = __hip_atomic_fetch_add(arr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- wave partial tiles -> LDS, summed in wave order.  Item t = (tile, lane) of a 16x16 tile: the
    // 4 rows 4*(lane/16)+i of token lane%16.  Beside the images (APART) each wave stores its tile as
    // soon as its loop ends; in their place only after every wave's loop has ended
    constexpr bool APART = ks_tm_red_apart(RT, W);
    f4v *red = reinterpret_cast<f4v *>(lds + (APART ? (size_t)W * IMG : 0u));
    uint32_t *flag = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(red) + (size_t)W * RT * CT * 1024u);
    if constexpr (!APART) {
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) red[((wv * RT + rt) * CT + ct) * 64u + lane] = acc[rt][ct];
    if (S > 1 && wv == 0 && lane == 0) *flag = ticket;  // (waits for the add's return)
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __asm__ volatile("" ::: "memory");
    constexpr uint32_t NI = RT * CT * 64u, NT = 64u * W;
    const uint32_t r0 = bmtb_first_row[g], R = bmtb_first_row[g + 1] - r0;
    auto item_sum = [&](uint32_t t) {
        f4v sum = red[t];
#pragma unroll
        for (uint32_t w = 1; w < W; w++) sum += red[w * NI + t];
        return sum;
    };
    const bool fused = !epilogue_is_identity(epi);
    // rows rb .. rb + 3 of token col: 4 consecutive elements of Y (and of the residual)
    auto store_item = [&](uint32_t t, const f4v &v) {
        const uint32_t ln = t & 63u, tt = t >> 6, rt = tt / CT, ct = tt % CT;
        const uint32_t col = 16u * ct + (ln & 15u), rb = 16u * rt + 4u * (ln >> 4);
        if (col >= nv || rb >= R) return;
        const size_t row = (size_t)row_base + r0 + rb, at = (size_t)(col0 + col) * M + row;
        ET h[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            float o = v[i];
            if constexpr (VB == 8) {  // FP8 weights: the row's scale on the fp32 sum, before the epilogue
                if (rb + i < R) o = __fmul_rn(ks_scale_arg(w_scale_arg...)[row + i], o);
            }
            if (fused && rb + i < R) {  // the launch's epilogue on the fp32 sum, rounded once (epilogue_apply)
                const float res = epi.residual ? (float)static_cast<const ET *>(epi.residual)[at + i] : 0.f;
                o = epilogue_apply(epi, o, row + i, res);
            }
            h[i] = (ET)o;
        }
        if (rb + 3u < R && (reinterpret_cast<uintptr_t>(Y + at) & 7u) == 0u) {
            u32x2 w2;
            __builtin_memcpy(&w2, h, 8);
            *reinterpret_cast<u32x2 *>(Y + at) = w2;
            return;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (rb + i < R) Y[at + i] = h[i];
    };
    if (S == 1) {
        for (uint32_t t = tid; t < NI; t += NT) store_item(t, item_sum(t));
        return;
    }
    // ---- K-split combine by tagged slabs: ks_body's, word for word (the slabs, the tags, the
    // arrival counter's epoch and the device error word are the plan replica's, shared with k_mfma_ks)
    const uint32_t tk = *flag & 0xffffu, tag = ((*flag >> 16) & 1u) ^ 1u;
    f4v *slab = reinterpret_cast<f4v *>(slabs) + ((size_t)u * T + tile) * NI;
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
    if (tk != S - 1u) return;
    if (tid == 0) __hip_atomic_store(arr, tag << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const f4v *base = reinterpret_cast<const f4v *>(slabs) + tile * NI;
    const size_t qstride = (size_t)T * NI;  // slab of (g, qq) = base + (g*S + qq) * qstride
    uint32_t *err = arrivals + (size_t)(nwg / S) * T;  // the replica's device error word
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
}

// ---------------------------------------------------------------------------
// k_mfma_ks_tm_group -- several k_mfma_ks_tm launches of one instantiation as one grid (gs_linear_batch: the
// Q/K/V projections of one x, an MLP's gate / up pair, experts with their own token counts), the token-major
// counterpart of k_mfma_ks_group (mfma_ks.hpp).  One 1-D grid: entry i owns workgroups [begin[i], begin[i] +
// nwg_i * T_i), T_i = ceil(N_i / 32) of the entry's OWN token count N_i, and runs them as its own k_mfma_ks_tm
// launch would (unit-major, v = u * T_i + tile, xcd_block over nwg_i * T_i); begin[i] is a multiple of 8, so
// the entry's block numbers keep the XCD residues xcd_block assumes, and the workgroups up to begin[i + 1]
// exit at once.  The entries are kernel arguments (ks_tm_group_args, read through the kernarg segment with
// scalar loads).  Every entry has its own (plan, replica), so its own tickets, slabs and error word: with
// S > 1 and T_i > 1 the replica's state laid out for T_i tiles, else the upload's own, as a single launch.
// ks_tm_group_body is k_mfma_ks_tm's body at VB = 16 -- the same text but for the block number, which is the
// entry's and not the grid's, so the MFMAs, their order and the order of every sum are the same and an
// entry's Y has the bits of its own launch.  The text is duplicated on purpose: k_mfma_ks_tm keeps its body
// in the kernel (see above: as a function its 16-bit instantiations allocate registers differently), and the
// single launch's device code stays what it was.  A change to one body belongs in the other.
// ---------------------------------------------------------------------------
struct ks_tm_entry {  // 120 B
    const uint32_t *tbr;
    const u32x4 *tP, *tV;
    const u32x2 *steps;
    const void *X;  // the instantiation's element type (k_mfma_ks_tm_group ET)
    void *Y;
    float *slabs;
    uint32_t *arrivals;
    uint32_t K, N, M, S, NS, nwg, row_base, gh;  // N: the entry's token count; gh: its head-step group count
    epilogue epi;  // the entry's epilogue (the identity: plain stores)
};
static_assert(sizeof(ks_tm_entry) == 120, "ks_tm_entry is 120 bytes");
// kKsTmGroupMax: kernel_consts.hpp
struct ks_tm_group_args {
    uint32_t begin[kKsTmGroupMax + 1];  // first workgroup of each entry (+ the total)
    uint32_t n, prio, pad;              // prio: k_mfma_ks_tm's, bits 0..7 (KS_PRIO, the forced timeout)
    ks_tm_entry e[kKsTmGroupMax];
};
static_assert(sizeof(ks_tm_group_args) <= 4096, "ks_tm_group_args must fit the 4 KB kernarg segment");

template <int RT, int W, int D, int MAXG, int NTL, class ET>
__device__ __forceinline__ void ks_tm_group_body(const uint32_t *__restrict__ bmtb_first_row, const u32x4 *__restrict__ tP,
                                                 const u32x4 *__restrict__ tV, const u32x2 *__restrict__ steps,
                                                 const ET *__restrict__ X, ET *__restrict__ Y, uint32_t K, uint32_t N,
                                                 uint32_t M, uint32_t S, uint32_t NS, uint32_t nwg, uint32_t row_base,
                                                 float *__restrict__ slabs, uint32_t *__restrict__ arrivals, uint32_t bx,
                                                 uint32_t prio, const epilogue &epi) {
    constexpr int CT = 2;
    constexpr uint32_t IMG = ks_image_bytes<RT>();
    static_assert(!ks_red_halves(CT, RT, W), "the W partial tiles fit LDS");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    // bx: the workgroup's number inside the entry's nwg * T (T in prio's bits 18..31, as k_mfma_ks_tm)
    const uint32_t T = max(prio >> 18, 1u);
    uint32_t u = xcd_block(bx, nwg * T), tile = 0;
    if (T > 1u) {
        const uint32_t v = u;
        u = v / T;
        tile = v - u * T;
    }
    const uint32_t g = u / S, q = u - g * S;
    const uint32_t k0 = q * NS * 32u;
    const uint32_t col0 = tile * 16u * CT, nv = min(16u * CT, N - col0);
    unsigned char *img = lds + wv * IMG;
    const u32x4 zero4 = {0u, 0u, 0u, 0u};

    // ---- this wave's k-steps w, w+W, ...
    const uint32_t nsw = NS > wv ? (NS - wv + W - 1u) / W : 0u;
    const size_t ubase = (size_t)u * NS;
    u32x4 P[D][MAXG], BR[D][CT];
    u32x4 V[D][MAXG];
    u32x2 NX[D];     // per slot: record of the step the slot loads next
    uint32_t CN[D];  // per slot: group count of the step whose groups it holds
    uint32_t vz;
    __asm__ volatile("v_mov_b32 %0, 0" : "=v"(vz));
    auto rec_of = [&](uint32_t i) -> u32x2 {
        const uint32_t st = __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u);
        return steps[ubase + st + vz];
    };
    const uint32_t ku = 8u * (lane >> 4);
    uint32_t xoff[CT];
#pragma unroll
    for (int c = 0; c < CT; c++) {
        const uint32_t tk = 16u * c + (lane & 15u);
        xoff[c] = (tk < nv ? tk : 0u) * K + ku;
    }
    auto load_b = [&](auto fast, uint32_t i, u32x4 (&B_)[CT]) {
        const uint32_t st = __builtin_amdgcn_readfirstlane(i < nsw ? wv + i * W : 0u);
        const uint32_t kr = k0 + st * 32u;  // first column of X of the step
        if constexpr (decltype(fast)::value) {
            const ET *Xk = X + (size_t)col0 * K + kr;
#pragma unroll
            for (int c = 0; c < CT; c++) B_[c] = *reinterpret_cast<const u32x4 *>(Xk + xoff[c]);
            return;
        }
        // a unit past K reads the row's first unit (zeroed in step); a token past N the tile's first
        const uint32_t kc = kr + ku < K ? kr + ku : 0u;
#pragma unroll
        for (int c = 0; c < CT; c++) {
            const uint32_t tk = 16u * c + (lane & 15u);
            B_[c] = *reinterpret_cast<const u32x4 *>(X + (size_t)(col0 + (tk < nv ? tk : 0u)) * K + kc);
        }
    };
    auto load_g_at = [&](uint32_t i, uint32_t b0, uint32_t gc, u32x2 &NX_, uint32_t &CN_, u32x4 (&P_)[MAXG],
                         u32x4 (&V_)[MAXG]) {
        CN_ = gc;
        NX_ = rec_of(i + D);
#pragma unroll
        for (int j = 0; j < MAXG; j++) {
            const uint32_t qg = lane + 64u * j;
            const size_t at = (size_t)b0 + (qg < gc ? qg : 0u);
            P_[j] = ld_once_if<(NTL & 1) != 0>(tP + at);
            V_[j] = ld_once_if<(NTL & 1) != 0>(tV + at);
        }
    };
    auto load_g = [&](uint32_t i, u32x2 &NX_, uint32_t &CN_, u32x4 (&P_)[MAXG], u32x4 (&V_)[MAXG]) {
        load_g_at(i, __builtin_amdgcn_readfirstlane(NX_[0]), __builtin_amdgcn_readfirstlane(NX_[1]), NX_, CN_, P_, V_);
    };
    const uint32_t GH = (prio >> 8) & 0x3ffu;  // groups per head step (0: every step by record)
    if (GH) {
#pragma unroll
        for (int d = 0; d < D; d++) {
            const uint32_t st = (uint32_t)d < nsw ? wv + (uint32_t)d * W : 0u;
            load_b(std::false_type{}, (uint32_t)d, BR[d]);
            __builtin_amdgcn_sched_barrier(0);
            load_g_at((uint32_t)d, (u * min((uint32_t)(W * D), NS) + st) * GH, GH, NX[d], CN[d], P[d], V[d]);
            __builtin_amdgcn_sched_barrier(0);
        }
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
        __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
        for (int d = 0; d < D; d++) NX[d] = rec_of((uint32_t)d);
        __builtin_amdgcn_sched_barrier(0);
        for (uint32_t x = lane; x < IMG / 16u; x += 64u) *reinterpret_cast<u32x4 *>(img + x * 16u) = zero4;
#pragma unroll
        for (int d = 0; d < D; d++) {
            __builtin_amdgcn_sched_barrier(0);
            load_b(std::false_type{}, (uint32_t)d, BR[d]);
            __builtin_amdgcn_sched_barrier(0);
            load_g((uint32_t)d, NX[d], CN[d], P[d], V[d]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }

    f4v acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) acc[rt][ct] = f4v{0.f, 0.f, 0.f, 0.f};
    uint32_t arow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) arow[rt] = (16u * rt + (lane & 15u)) * kKsStride + 16u * (lane >> 4);

    auto ent_h = [&](const u32x4 &p, int e) -> uint32_t { return (p[e >> 1] >> (16 * (e & 1))) & 0xffffu; };
    auto step = [&](auto fast, uint32_t i, u32x2 &NX_, uint32_t &CN_, u32x4 (&P_)[MAXG], u32x4 (&V_)[MAXG], u32x4 (&B_)[CT]) {
        const bool live = i < nsw;  // wave-uniform
        const uint32_t gc = CN_;
        typedef typename mfma_elem<ET>::frag frag;
        frag av[RT], bv[CT];
        if (live) {
            // scatter the step's entries into the image
#pragma unroll
            for (int j = 0; j < MAXG; j++) {
                if (lane + 64u * j < gc) {
                    const auto &gv = ks_group_values<16>(V_[j]);  // the group's 8 values as 16-bit words
#pragma unroll
                    for (int e = 0; e < 8; e++) {
                        const uint16_t v = (uint16_t)((gv[e >> 1] >> (16 * (e & 1))) & 0xffffu);
                        *reinterpret_cast<uint16_t *>(img + ent_h(P_[j], e) * 2u) = v;
                    }
                }
            }
            // A fragments (LDS runs a wave's operations in order: the reads see the stores)
#pragma unroll
            for (int rt = 0; rt < RT; rt++) av[rt] = *reinterpret_cast<const frag *>(img + arow[rt]);
            // the image back to zero at the entries' positions
#pragma unroll
            for (int j = 0; j < MAXG; j++) {
                if (lane + 64u * j < gc) {
#pragma unroll
                    for (int e = 0; e < 8; e++) *reinterpret_cast<uint16_t *>(img + ent_h(P_[j], e) * 2u) = (uint16_t)0;
                }
            }
            // B fragments: the loaded units as they are (a unit past K as zeros)
            const uint32_t kr = k0 + (wv + i * W) * 32u;
#pragma unroll
            for (int ct = 0; ct < CT; ct++) {
                u32x4 b = B_[ct];
                if constexpr (!decltype(fast)::value) b = kr + ku < K ? b : zero4;
                __builtin_memcpy(&bv[ct], &b, 16);
            }
        }
        load_b(fast, i + D, B_);
        load_g(i + D, NX_, CN_, P_, V_);
        if (live) {
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int ct = 0; ct < CT; ct++)
                    acc[rt][ct] = mfma_elem<ET>::mfma_16x16x32(av[rt], bv[ct], acc[rt][ct]);
        }
    };
    const bool young = wv >= W / 2u;
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(1);
    const uint32_t fsp = min(NS, K > k0 ? (K - k0) / 32u : 0u);
    const uint32_t nfull = fsp > wv ? (fsp - wv + W - 1u) / W : 0u;  // this wave's full steps
    uint32_t fast_end = fsp == NS ? nsw : (nfull >= 2u * D ? ((nfull - 2u * D) / D + 1u) * D : 0u);
    fast_end = __builtin_amdgcn_readfirstlane(fast_end);
    uint32_t i0 = 0;
    for (; i0 < fast_end; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(std::true_type{}, i0 + d, NX[d], CN[d], P[d], V[d], BR[d]);
        if ((prio & 3u) == 2u && young && i0 + D >= nsw / 2u && i0 < nsw / 2u) __builtin_amdgcn_s_setprio(0);
    }
    for (; i0 < nsw; i0 += D) {
#pragma unroll
        for (int d = 0; d < D; d++) step(std::false_type{}, i0 + d, NX[d], CN[d], P[d], V[d], BR[d]);
        if ((prio & 3u) == 2u && young && i0 + D >= nsw / 2u && i0 < nsw / 2u) __builtin_amdgcn_s_setprio(0);
    }
    if ((prio & 3u) && young) __builtin_amdgcn_s_setprio(0);
    // ---- K-split ticket, taken as soon as wave 0's loop ends
    uint32_t *arr = arrivals + (size_t)g * T + tile;
    uint32_t ticket = 0;
    if (S > 1 && wv == 0 && lane == 0) ticket = __hip_atomic_fetch_add(arr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // ---- wave partial tiles -> LDS, summed in wave order
    constexpr bool APART = ks_tm_red_apart(RT, W);
    f4v *red = reinterpret_cast<f4v *>(lds + (APART ? (size_t)W * IMG : 0u));
    uint32_t *flag = reinterpret_cast<uint32_t *>(reinterpret_cast<unsigned char *>(red) + (size_t)W * RT * CT * 1024u);
    if constexpr (!APART) {
        __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __asm__ volatile("" ::: "memory");
    }
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int ct = 0; ct < CT; ct++) red[((wv * RT + rt) * CT + ct) * 64u + lane] = acc[rt][ct];
    if (S > 1 && wv == 0 && lane == 0) *flag = ticket;  // (waits for the add's return)
    __asm__ volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __asm__ volatile("" ::: "memory");
    constexpr uint32_t NI = RT * CT * 64u, NT = 64u * W;
    const uint32_t r0 = bmtb_first_row[g], R = bmtb_first_row[g + 1] - r0;
    auto item_sum = [&](uint32_t t) {
        f4v sum = red[t];
#pragma unroll
        for (uint32_t w = 1; w < W; w++) sum += red[w * NI + t];
        return sum;
    };
    const bool fused = !epilogue_is_identity(epi);
    // rows rb .. rb + 3 of token col: 4 consecutive elements of Y (and of the residual)
    auto store_item = [&](uint32_t t, const f4v &v) {
        const uint32_t ln = t & 63u, tt = t >> 6, rt = tt / CT, ct = tt % CT;
        const uint32_t col = 16u * ct + (ln & 15u), rb = 16u * rt + 4u * (ln >> 4);
        if (col >= nv || rb >= R) return;
        const size_t row = (size_t)row_base + r0 + rb, at = (size_t)(col0 + col) * M + row;
        ET h[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            float o = v[i];
            if (fused && rb + i < R) {  // the entry's epilogue on the fp32 sum, rounded once (epilogue_apply)
                const float res = epi.residual ? (float)static_cast<const ET *>(epi.residual)[at + i] : 0.f;
                o = epilogue_apply(epi, o, row + i, res);
            }
            h[i] = (ET)o;
        }
        if (rb + 3u < R && (reinterpret_cast<uintptr_t>(Y + at) & 7u) == 0u) {
            u32x2 w2;
            __builtin_memcpy(&w2, h, 8);
            *reinterpret_cast<u32x2 *>(Y + at) = w2;
            return;
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
            if (rb + i < R) Y[at + i] = h[i];
    };
    if (S == 1) {
        for (uint32_t t = tid; t < NI; t += NT) store_item(t, item_sum(t));
        return;
    }
    // ---- K-split combine by tagged slabs: k_mfma_ks_tm's, word for word
    const uint32_t tk = *flag & 0xffffu, tag = ((*flag >> 16) & 1u) ^ 1u;
    f4v *slab = reinterpret_cast<f4v *>(slabs) + ((size_t)u * T + tile) * NI;
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
    if (tk != S - 1u) return;
    if (tid == 0) __hip_atomic_store(arr, tag << 16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const f4v *base = reinterpret_cast<const f4v *>(slabs) + tile * NI;
    const size_t qstride = (size_t)T * NI;  // slab of (g, qq) = base + (g*S + qq) * qstride
    uint32_t *err = arrivals + (size_t)(nwg / S) * T;  // the replica's device error word
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
}

template <int RT, int W, int D, int MAXG, int NTL = 0, class ET = f16>
__global__ __launch_bounds__(64 * W) void k_mfma_ks_tm_group(ks_tm_group_args args) {
    const uint32_t bx = blockIdx.x, n = args.n;
    uint32_t sel = 0;
#pragma unroll
    for (int i = 1; i < kKsTmGroupMax; i++)
        if ((uint32_t)i < n && args.begin[i] <= bx) sel = (uint32_t)i;
    sel = __builtin_amdgcn_readfirstlane(sel);
    const ks_tm_entry &e = args.e[sel];  // kernel arguments: scalar loads at a computed offset
    const uint32_t T = (e.N + 31u) / 32u, rel = bx - args.begin[sel];
    if (rel >= e.nwg * T) return;  // padding up to the next entry's multiple of 8
    ks_tm_group_body<RT, W, D, MAXG, NTL, ET>(e.tbr, e.tP, e.tV, e.steps, (const ET *)e.X, (ET *)e.Y, e.K, e.N, e.M, e.S, e.NS,
                                              e.nwg, e.row_base, e.slabs, e.arrivals, rel,
                                              (args.prio & 0xffu) | (e.gh << 8) | (T << 18), e.epi);
}

}  // namespace gsk
