// hip_code/merge_path.hpp -- the merge-path levels: k_permute_rows, k_merge_path (with the
// merge_chain_* hand-off) and k_merge_fixup; in the experiments build also k_merge_rows.
// Instantiated by kernels/gather_launch.hip.
#pragma once

#include "kernel_common.hpp"

namespace gsk {

// k_permute_rows -- B into a merge-path plan's column order (MP_COL_PERM): row i of Bp is row
// perm[i] of B (perm: the original column of renumbered column i, most nonzeros first), read
// by a gather; SCATTER: perm[i] is the new place of column i, B read in order and each row
// written to its place.  16 B per thread when a row is whole 16-B units, one element otherwise.
template <class VT, bool SCATTER>
__global__ __launch_bounds__(256) void k_permute_rows(const VT *__restrict__ B, VT *__restrict__ Bp,
                                                      const uint32_t *__restrict__ perm, uint32_t K, uint32_t N) {
    const uint64_t stride = (uint64_t)gridDim.x * 256u;
    if ((N * sizeof(VT)) % 16u == 0) {
        const uint32_t upr = N * (uint32_t)sizeof(VT) / 16u;
        const uint64_t total = (uint64_t)K * upr;
        for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += stride) {
            const uint32_t i = (uint32_t)(t / upr), u = (uint32_t)(t - (uint64_t)i * upr);
            if constexpr (SCATTER)
                reinterpret_cast<u32x4 *>(Bp)[(size_t)perm[i] * upr + u] = reinterpret_cast<const u32x4 *>(B)[t];
            else
                reinterpret_cast<u32x4 *>(Bp)[t] = reinterpret_cast<const u32x4 *>(B)[(size_t)perm[i] * upr + u];
        }
    } else {
        const uint64_t total = (uint64_t)K * N;
        for (uint64_t t = (uint64_t)blockIdx.x * 256u + threadIdx.x; t < total; t += stride) {
            const uint32_t i = (uint32_t)(t / N), j = (uint32_t)(t - (uint64_t)i * N);
            if constexpr (SCATTER)
                Bp[(size_t)perm[i] * N + j] = B[t];
            else
                Bp[t] = B[(size_t)perm[i] * N + j];
        }
    }
}

// ---------------------------------------------------------------------------
// k_merge_path -- merge-path levels (merge_path_{thread,warp,tblock}_operator +
// the level's total-reduce token).  The plan's
// level starts (first_row_indices_without_ending / first_nz_indices,
// get_begin_{rows,nzs}_of_level_after_merge_path.cc) are decoded on the host
// into nz-exact wave ranges [wz[w], wz[w+1]) (gsk_host::merge_path_layout);
// rows are the non-empty rows in compact order: ends[j] = their CSR row ends,
// rid[j] = their output rows.  A wave walks its range in rounds of 8*S
// nonzeros (S = 64/X slots of X column lanes, 8 consecutive nonzeros per slot,
// one 16/32-B load of cols and of vals, all 8 B-row gathers in flight):
//   1. the rows closing in the round are staged in the wave's LDS and mark a
//      row-start flag per position (flag at e - zb for every row end e);
//   2. each slot walks its 8 positions with the flags as a bit mask: a run
//      that starts and closes inside the slot is stored at once; the slot's
//      head run (continuing from the left) is held back; its tail run is the
//      slot's carry;
//   3. a segmented scan over slots (stop = any row start/close in the slot)
//      gives every slot its carry-in; held-back heads add it and are stored;
//      the last slot's scan value is carried into the next round.
// Empty rows are zeroed from a list by the kernel's first fill_blocks
// workgroups, concurrently with the path waves (no memset of C, no extra
// launch).  Rows crossing waves: the wave the row is open at the end of writes
// its partial to rec[w], the wave that closes it writes its own partial to
// head_rec instead of C.  With `chain` (one column tile) the partials are
// combined in the same launch: every contributing wave publishes its partial
// with agent-scope (L2 write-through) stores, waits for them, and bumps the
// closing wave's arrival counter; the last arriver reads the chain's partials
// back in wave order, stores the row (one rounding, deterministic) and re-arms
// the counter.  No wave waits on another, so any dispatch order is safe.
// Without `chain`, rec_row[w] names the open row and k_merge_fixup sums them.
// ---------------------------------------------------------------------------
// kMpItems (nonzeros per slot per round): kernel_consts.hpp

// Rows split across waves, combined in the launch.  A partial is published to part[src]
// with agent-scope stores (written through the XCD's L2); its arrival (the X lanes of
// one slot; lane0 = the slot's first lane) waits for the wave's stores, then the slot's
// first lane bumps the closing wave's counter.  The arrival that completes the chain
// (parts = close - first + 1) sums rec[first .. close-1] and head_rec[close] in wave
// order with agent-scope loads, writes the row and re-arms the counter.
// Ordering: every access of the hand-off is an agent-scope atomic (sc1: written through
// to / read from the memory-side coherence point, no stale XCD-L2 copy), and the
// publisher's vmcnt(0) retires its stores before its counter add is issued; the reader
// loads only after its add returned the completing count (a control dependency).  That
// is MI355X_MICROARCH.md §Workgroup dispatch's hand-off form.  The language-level form
// (acq_rel on the add) is not used: on gfx950 an agent-scope release is a
// buffer_wbl2 sc1 (write-back of the XCD's whole L2) and the acquire a buffer_inv sc1,
// per arrival -- measured C4 merge_path(1024) 49 -> 84 us, r03 session 1.
template <int CF>
__device__ __forceinline__ void merge_chain_publish(const float (&a)[CF], float *part, uint32_t src, uint32_t N,
                                                    uint32_t c0, bool cok) {
    if (cok) {
#pragma unroll
        for (int k = 0; k < CF; k++)
            __hip_atomic_store(part + (size_t)src * N + c0 + k, a[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <class VT, int CF>
__device__ __forceinline__ void merge_chain_arrive(uint32_t close, uint32_t first, const float *rec, const float *head_rec,
                                                   uint32_t *cnt, uint32_t row, VT *C, uint32_t N, uint32_t c0, bool cok,
                                                   uint32_t lane0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    uint32_t old = 0;
    if ((threadIdx.x & 63u) == lane0) old = __hip_atomic_fetch_add(cnt + close, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    old = __shfl(old, (int)lane0, 64);
    if (old + 1u != close - first + 1u) return;
    if (cok) {
        float s[CF];
#pragma unroll
        for (int k = 0; k < CF; k++) s[k] = 0.f;
        for (uint32_t v = first; v < close; v++) {
#pragma unroll
            for (int k = 0; k < CF; k++)
                s[k] += __hip_atomic_load(rec + (size_t)v * N + c0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int k = 0; k < CF; k++)
            s[k] += __hip_atomic_load(head_rec + (size_t)close * N + c0 + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        store_f32<VT, CF>(C + (size_t)row * N + c0, s);
    }
    if ((threadIdx.x & 63u) == lane0) __hip_atomic_store(cnt + close, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// per wave: row-start flags (bytes 0..8S) and the staged output rows rid_l (cap + 2)
__host__ __device__ constexpr uint32_t merge_path_wave_lds_words(uint32_t S) {
    return (kMpItems * S) / 4u + 2u + (kMpItems * S + 64u) + 2u;
}

// STAMPS (diagnostic build only, gs_debug_mfma_timeline on a merge-path plan): lane 0 of
// every path wave records s_memtime into stamps[w * 16 + slot]: 0 start, 1 first loads
// issued, per round r < 4: 2 + 3r gathers issued, 3 + 3r rows staged, 4 + 3r walked and
// scanned; 14 loop done, 15 end (chain arrival)
template <class VT, class CT, int CF, bool STAMPS = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void k_merge_path(const uint32_t *__restrict__ wz,   // n_waves+1
                                                    const uint32_t *__restrict__ wq,   // n_waves+1
                                                    const uint32_t *__restrict__ ends, // n_crow
                                                    const uint32_t *__restrict__ rid,  // n_crow
                                                    uint32_t n_crow, const CT *__restrict__ col,
                                                    const VT *__restrict__ val, const VT *__restrict__ B,
                                                    VT *__restrict__ C, float *__restrict__ rec,
                                                    uint32_t *__restrict__ rec_row, float *__restrict__ head_rec,
                                                    uint32_t n_waves, uint32_t N, uint32_t X, uint32_t row_lo,
                                                    uint32_t row_hi, const uint32_t *__restrict__ empty_rows,
                                                    uint32_t n_empty, uint32_t fill_blocks,
                                                    const uint32_t *__restrict__ chain,  // 2 n_waves or null
                                                    uint32_t *__restrict__ chain_cnt,    // n_waves, zero between launches
                                                    uint32_t dbg = 0, uint64_t *__restrict__ stamps = nullptr) {
    // dbg (diagnostic timing runs only, wrong results): bit 1 gathers B row 0 for every nonzero;
    // experiments build: bit 8 skips the slot scans (row-start prefix and the segmented carry
    // scan), bit 16 treats every position as inside a row (no row closes or emits in a round)
    const uint32_t lb = blockIdx.x;  // (XCD-contiguous numbering measured no faster cold on C4)
    if (lb < fill_blocks) {
        // the first fill_blocks workgroups zero the empty rows (listed; 16-B stores when a
        // C row is whole 16-B units) while the path waves run
        const uint32_t rbytes = N * (uint32_t)sizeof(VT);
        const uint32_t U = rbytes % 16u == 0 ? rbytes / 16u : N;
        const uint32_t tot = blockIdx.y == 0 ? n_empty * U : 0u;  // one column-tile row of blocks fills
        for (uint32_t i = lb * blockDim.x + threadIdx.x; i < tot; i += fill_blocks * blockDim.x) {
            const uint32_t er = empty_rows[i / U];
            if (rbytes % 16u == 0)
                *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(C) + (size_t)er * rbytes + (i % U) * 16u) =
                    make_uint4(0u, 0u, 0u, 0u);
            else
                C[(size_t)er * N + i % U] = (VT)0.f;
        }
        return;
    }
    extern __shared__ uint32_t mp_lds[];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    const uint32_t xl = lane & (X - 1u), slot = lane / X, S = 64u / X;
    const uint32_t R8 = kMpItems * S;     // nonzeros per round
    const uint32_t fw = R8 / 4u + 2u;     // flag words: bytes 0..R8
    const uint32_t cap = R8 + 64u;        // staged rows per round
    uint32_t *wl = mp_lds + wib * merge_path_wave_lds_words(S);
    unsigned char *flags = reinterpret_cast<unsigned char *>(wl);
    uint32_t *rid_l = wl + fw;            // rid[qs - 1 + k]
    const uint32_t waves_total = (gridDim.x - fill_blocks) * (blockDim.x >> 6);
    typedef typename raw_vec<CF * sizeof(VT)>::t RB;
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t w = (lb - fill_blocks) * (blockDim.x >> 6) + wib; w < n_waves; w += waves_total) {
#define GS_MP_STAMP(slot)                                                                          \
    if constexpr (STAMPS) {                                                                        \
        if (lane == 0 && blockIdx.y == 0) stamps[(size_t)w * 16u + (slot)] = __builtin_amdgcn_s_memtime(); \
    }
            GS_MP_STAMP(0u);
            const uint32_t zlo = wz[w], wend = wz[w + 1], q0 = wq[w];
            uint32_t rnd = 0;
            // the wave starts inside row q0 (its partial goes to head_rec)
            const bool head_open = zlo > (q0 ? ends[q0 - 1] : 0u);
            const uint32_t head_first = chain && head_open ? chain[n_waves + w] : 0u;
            uint32_t qs = q0;
            float rc[CF];
#pragma unroll
            for (int k = 0; k < CF; k++) rc[k] = 0.f;
            bool closed_end = false;
            bool head_done = false;  // chain mode: this slot published the head row's partial
            auto emit = [&](uint32_t qq, const float (&a)[CF]) {
                if (qq == q0 && head_open) {
                    if (chain) {  // published now (agent-scope stores), arrives after the walk
                        merge_chain_publish<CF>(a, head_rec, w, N, c0, cok);
                        head_done = true;
                        return;
                    }
                    if (!cok) return;
#pragma unroll
                    for (int k = 0; k < CF; k++) head_rec[(size_t)w * N + c0 + k] = a[k];
                } else {
                    if (!cok) return;
                    store_f32<VT, CF>(C + (size_t)rid_l[qq - qs + 1u] * N + c0, a);
                }
            };
            // software pipeline: round r+1's A entries and first staging batch are loaded
            // while round r walks; round r's gathers are issued before that prefetch, so
            // waiting for them leaves the prefetch in flight
            CT cn[kMpItems];
            VT vn[kMpItems];
            // the next round's first kMpPref x 64 rows (ends, output rows), prefetched a round
            // ahead; rows past the prefetched batches are loaded synchronously.  (Two batches,
            // for rounds of ~3-nonzero rows that close ~85 rows: C4 51.0 against 49.2 us.)
            constexpr uint32_t kMpPref = 1;
            uint32_t en[kMpPref], rn[kMpPref];
            auto load_a = [&](uint32_t zb_) {
                const uint32_t b_ = zb_ + kMpItems * slot;
                if (b_ < wend) {
                    load_raw<CT, kMpItems>(col + b_, cn);
                    load_raw<VT, kMpItems>(val + b_, vn);
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < kMpItems; k++) { cn[k] = 0; vn[k] = (VT)0.f; }
                }
            };
            auto load_s = [&](uint32_t q_) {  // the first kMpPref x 64 rows a round stages
#pragma unroll
                for (uint32_t b = 0; b < kMpPref; b++) {
                    const uint32_t j = q_ + 64u * b + lane;
                    en[b] = j < n_crow ? ends[j] : 0xffffffffu;
                    rn[b] = j < n_crow ? rid[j] : 0u;
                }
            };
            const uint32_t zb0 = zlo & ~(kMpItems - 1u);
            load_a(zb0);
            load_s(qs);
            GS_MP_STAMP(1u);
            for (uint32_t zb = zb0; zb < wend; zb += R8) {
                const uint32_t zl = max(zb, zlo), ze = min(zb + R8, wend);
                const uint32_t base = zb + kMpItems * slot;
                CT cc[kMpItems];
                VT vv[kMpItems];
#pragma unroll
                for (uint32_t k = 0; k < kMpItems; k++) { cc[k] = cn[k]; vv[k] = vn[k]; }
                RB braw[kMpItems];  // all gathers of the round in flight before the walk
#pragma unroll
                for (uint32_t k = 0; k < kMpItems; k++) {
                    const uint32_t z = base + k;
                    const bool valid = z >= zl && z < ze;
                    braw[k] = *reinterpret_cast<const RB *>(B + (size_t)(valid && !(dbg & 2u) ? (uint32_t)cc[k] : 0u) * N + c0);
                }
                if (rnd < 4u) GS_MP_STAMP(2u + 3u * rnd);
                for (uint32_t i = lane; i < fw; i += 64u) wl[i] = 0u;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // stage the rows closing in this round and the one open at its end
                uint32_t nclose = 0;
                closed_end = false;
                uint32_t e = en[0], r = rn[0];
                for (uint32_t k0 = 0;; k0 += 64u) {
                    if (k0 && k0 < 64u * kMpPref) {
#pragma unroll
                        for (uint32_t b = 1; b < kMpPref; b++)
                            if (k0 == 64u * b) { e = en[b]; r = rn[b]; }
                    } else if (k0) {  // rows beyond the prefetched batches (short rows): synchronous
                        const uint32_t j = qs + k0 + lane;
                        e = j < n_crow ? ends[j] : 0xffffffffu;
                        r = j < n_crow ? rid[j] : 0u;
                    }
                    if (k0 + lane < cap) rid_l[k0 + lane + 1u] = r;
                    if (e > zl && e <= ze) flags[e - zb] = 1;
                    nclose += (uint32_t)__builtin_popcountll(__ballot(e <= ze));
                    closed_end = closed_end || __ballot(e == ze) != 0ull;
                    if (__ballot(e >= ze) != 0ull || k0 + 64u >= cap) break;
                }
                if (zb + R8 < wend) {
                    load_a(zb + R8);
                    load_s(qs + nclose);
                }
                if (rnd < 4u) GS_MP_STAMP(3u + 3u * rnd);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // this slot's row starts: bit k = position 8*slot + k (bit 8: the next slot's first)
                const uint32_t fo = kMpItems * slot;
                const uint2 f8 = *reinterpret_cast<const uint2 *>(flags + fo);
                uint32_t bits = (uint32_t)flags[fo + kMpItems] << 8;
#pragma unroll
                for (uint32_t k = 0; k < 4; k++) bits |= ((f8.x >> (8 * k)) & 1u) << k | ((f8.y >> (8 * k)) & 1u) << (k + 4);
#ifdef GS_EXPERIMENTS
                if (dbg & 16u) bits = 0u;
                const bool scans = !(dbg & 8u);
#else
                constexpr bool scans = true;
#endif
                const uint32_t pc = (uint32_t)__builtin_popcount(bits & 0xffu);
                uint32_t incl = pc;
                if (scans) {
#pragma unroll
                    for (uint32_t st = 0; st < 6; st++) {
                        const uint32_t off = X << st;
                        if (off >= 64u) break;
                        const uint32_t t = __shfl_up(incl, off, 64);
                        if (lane >= off) incl += t;
                    }
                }
                uint32_t qcur = qs + incl - pc;  // row open before this slot's first position
                float acc[CF], h[CF];
#pragma unroll
                for (int k = 0; k < CF; k++) { acc[k] = 0.f; h[k] = 0.f; }
                bool has_h = false, in_head = true;
                uint32_t hq = 0;
                const bool head_cont = !(bits & 1u);
                auto close = [&](uint32_t qq) {
                    if (in_head && head_cont) {
                        has_h = true;
                        hq = qq;
#pragma unroll
                        for (int k = 0; k < CF; k++) h[k] = acc[k];
                    } else {
                        emit(qq, acc);
                    }
                };
#pragma unroll
                for (uint32_t k = 0; k < kMpItems; k++) {
                    if ((bits >> k) & 1u) {
                        if (k > 0) close(qcur);
                        qcur++;
                        in_head = false;
#pragma unroll
                        for (int i = 0; i < CF; i++) acc[i] = 0.f;
                    }
                    const uint32_t z = base + k;
                    if (z >= zl && z < ze) {
                        VT bt[CF];
                        __builtin_memcpy(bt, &braw[k], sizeof(RB));
                        const float v = (float)vv[k];
#pragma unroll
                        for (int i = 0; i < CF; i++) acc[i] = __builtin_fmaf(v, (float)bt[i], acc[i]);
                    }
                }
                if ((bits >> kMpItems) & 1u) {
                    close(qcur);
#pragma unroll
                    for (int i = 0; i < CF; i++) acc[i] = 0.f;
                }
                // segmented inclusive scan of the slots' carries (stop: the slot starts or closes a row)
                uint32_t stop = bits != 0u;
                if (slot == 0 && !stop) {
#pragma unroll
                    for (int i = 0; i < CF; i++) acc[i] += rc[i];
                }
#pragma unroll
                for (uint32_t st = 0; st < 6; st++) {
                    const uint32_t off = X << st;
                    if (off >= 64u || !scans) break;
                    const uint32_t ts = __shfl_up(stop, off, 64);
                    float t[CF];
#pragma unroll
                    for (int i = 0; i < CF; i++) t[i] = __shfl_up(acc[i], off, 64);
                    if (lane >= off) {
                        if (!stop) {
#pragma unroll
                            for (int i = 0; i < CF; i++) acc[i] += t[i];
                        }
                        stop |= ts;
                    }
                }
                float cin[CF];
#pragma unroll
                for (int i = 0; i < CF; i++) {
                    const float t = __shfl_up(acc[i], X, 64);
                    cin[i] = slot ? t : rc[i];
                }
                if (has_h) {
#pragma unroll
                    for (int i = 0; i < CF; i++) h[i] += cin[i];
                    emit(hq, h);
                }
#pragma unroll
                for (int i = 0; i < CF; i++) rc[i] = __shfl(acc[i], (S - 1u) * X + xl, 64);
                qs += nclose;
                if (rnd < 4u) GS_MP_STAMP(4u + 3u * rnd);
                rnd++;
                __builtin_amdgcn_wave_barrier();
            }
            GS_MP_STAMP(14u);
            // the row open at the wave's end (if any): its partial joins the row's chain
            if (chain) {
                if (head_done)  // the slot that closed the head row
                    merge_chain_arrive<VT, CF>(w, head_first, rec, head_rec, chain_cnt, rid[q0], C, N, c0, cok, lane - xl);
                if (!closed_end && slot == 0) {
                    const uint32_t cw_ = chain[w];  // the wave closing the row
                    merge_chain_publish<CF>(rc, rec, w, N, c0, cok);
                    merge_chain_arrive<VT, CF>(cw_, chain[n_waves + cw_], rec, head_rec, chain_cnt, rid[qs], C, N, c0, cok,
                                               0u);
                }
            } else {
                if (lane == 0) rec_row[w] = closed_end ? 0xffffffffu : rid[qs];
                if (!closed_end && slot == 0 && cok) {
#pragma unroll
                    for (int k = 0; k < CF; k++) rec[(size_t)w * N + c0 + k] = rc[k];
                }
            }
            GS_MP_STAMP(15u);
#undef GS_MP_STAMP
        }
    }
}

#ifdef GS_EXPERIMENTS  // opt-in, measured slower than k_merge_path (make EXPERIMENTS=1)
// ---------------------------------------------------------------------------
// k_merge_rows -- the same merge-path plan (wave ranges wz/wq, compact rows
// ends/rid, split-row chains) with a two-phase walk per round of R = S*J
// nonzeros instead of k_merge_path's flag/scan machinery:
//   1. products: slot s owns the J consecutive nonzeros zb + s*J .. (one vector
//      load of cols and of vals, J B-row gathers in flight), multiplies them and
//      writes the fp32 products (X*CF columns per nonzero) to the wave's LDS;
//   2. rows: the rows meeting the round are dealt to the slots, S at a time; a
//      slot adds its row's products from LDS (rows of more than `solo` products
//      are summed by the whole wave, slot-strided, one xor-shuffle reduction)
//      and stores the row.  The row left open at the round's end carries its
//      partial into the next round's first row.
// Row bounds come from two 64-row batches of `ends` loaded at the wave's start
// (exchanged with shuffles; rows past them are loaded directly).  The head row
// (open at zlo) and the tail row (open at zhi) join the row's chain exactly as
// in k_merge_path (agent-scope publish, last arriver combines), or go to
// head_rec / rec + rec_row for k_merge_fixup when the launch has several column
// tiles.  Deterministic: every row is summed in a fixed order.
// ---------------------------------------------------------------------------
template <int CF>
__host__ __device__ constexpr uint32_t merge_rows_j() { return CF >= 8 ? 4u : 8u; }
// fp32 words of one wave's product buffer: R entries of X*CF words + 4 words per slot group
__host__ __device__ constexpr uint32_t merge_rows_wave_words(uint32_t X, uint32_t CF, uint32_t J) {
    return (64u / X) * J * X * CF + (64u / X) * 4u;
}

template <class VT, class CT, int CF>
__global__ __launch_bounds__(256) void k_merge_rows(const uint32_t *__restrict__ wz,   // n_waves+1
                                                    const uint32_t *__restrict__ wq,   // n_waves+1
                                                    const uint32_t *__restrict__ ends, // n_crow
                                                    const uint32_t *__restrict__ rid,  // n_crow
                                                    uint32_t n_crow, const CT *__restrict__ col,
                                                    const VT *__restrict__ val, const VT *__restrict__ B,
                                                    VT *__restrict__ C, float *__restrict__ rec,
                                                    uint32_t *__restrict__ rec_row, float *__restrict__ head_rec,
                                                    uint32_t n_waves, uint32_t N, uint32_t X,
                                                    const uint32_t *__restrict__ empty_rows, uint32_t n_empty,
                                                    uint32_t fill_blocks,
                                                    const uint32_t *__restrict__ chain,  // 2 n_waves or null
                                                    uint32_t *__restrict__ chain_cnt,    // n_waves, zero between launches
                                                    uint32_t solo) {
    constexpr uint32_t J = merge_rows_j<CF>();
    const uint32_t lb = blockIdx.x;
    if (lb < fill_blocks) {  // empty rows, as in k_merge_path
        const uint32_t rbytes = N * (uint32_t)sizeof(VT);
        const uint32_t U = rbytes % 16u == 0 ? rbytes / 16u : N;
        const uint32_t tot = blockIdx.y == 0 ? n_empty * U : 0u;
        for (uint32_t i = lb * blockDim.x + threadIdx.x; i < tot; i += fill_blocks * blockDim.x) {
            const uint32_t er = empty_rows[i / U];
            if (rbytes % 16u == 0)
                *reinterpret_cast<uint4 *>(reinterpret_cast<unsigned char *>(C) + (size_t)er * rbytes + (i % U) * 16u) =
                    make_uint4(0u, 0u, 0u, 0u);
            else
                C[(size_t)er * N + i % U] = (VT)0.f;
        }
        return;
    }
    extern __shared__ float mr_lds[];
    const uint32_t lane = threadIdx.x & 63u, wib = threadIdx.x >> 6;
    const uint32_t xl = lane & (X - 1u), slot = lane / X, S = 64u / X;
    const uint32_t R = S * J, TW = X * CF;
    float *P = mr_lds + wib * merge_rows_wave_words(X, CF, J);
    // float offset of product entry e (this lane's columns); 4 words of padding per slot group
    auto pofs = [&](uint32_t e) { return e * TW + (e / J) * 4u + xl * CF; };
    const uint32_t waves_total = (gridDim.x - fill_blocks) * (blockDim.x >> 6);
    const uint64_t slot_bits = X >= 64u ? ~0ull : ((1ull << X) - 1ull);
    typedef typename raw_vec<CF * sizeof(VT)>::t RB;
    for (uint32_t ct = blockIdx.y; ct * X * CF < N; ct += gridDim.y) {
        const uint32_t cw = ct * X * CF + xl * CF;
        const bool cok = cw < N;
        const uint32_t c0 = cok ? cw : 0u;
        for (uint32_t w = (lb - fill_blocks) * (blockDim.x >> 6) + wib; w < n_waves; w += waves_total) {
            const uint32_t zlo = wz[w], zhi = wz[w + 1], q0 = wq[w], qn = wq[w + 1];
            const uint32_t zb0 = zlo & ~(J - 1u);
            // A entries of the first round, and the first 128 rows' ends
            CT cn[J];
            VT vn[J];
            auto load_a = [&](uint32_t zb_) {
                const uint32_t b_ = zb_ + J * slot;
                if (b_ < zhi) {
                    load_raw<CT, (int)J>(col + b_, cn);
                    load_raw<VT, (int)J>(val + b_, vn);
                } else {
#pragma unroll
                    for (uint32_t k = 0; k < J; k++) { cn[k] = 0; vn[k] = (VT)0.f; }
                }
            };
            load_a(zb0);
            const uint32_t e0 = q0 + lane < n_crow ? ends[q0 + lane] : 0xffffffffu;
            const uint32_t e1 = q0 + 64u + lane < n_crow ? ends[q0 + 64u + lane] : 0xffffffffu;
            const uint32_t sq0 = q0 ? ends[q0 - 1u] : 0u;
            // end of wave row i (row q0 + i); i may differ per lane
            auto row_end = [&](uint32_t i) -> uint32_t {
                const uint32_t a0 = (uint32_t)__shfl((int)e0, (int)(i & 63u), 64);
                const uint32_t a1 = (uint32_t)__shfl((int)e1, (int)(i & 63u), 64);
                if (i < 64u) return a0;
                if (i < 128u) return a1;
                return q0 + i < n_crow ? ends[q0 + i] : 0xffffffffu;
            };
            const bool head_open = zlo > sq0;
            const uint32_t q_last = (qn < n_crow && (qn ? ends[qn - 1] : 0u) < zhi) ? qn : qn - 1u;
            const bool tail_open = ends[q_last] > zhi;
            bool head_mine = false;
            float carry[CF];
#pragma unroll
            for (int k = 0; k < CF; k++) carry[k] = 0.f;
            uint32_t qi0 = 0;  // wave row index of the round's first row
            for (uint32_t zb = zb0; zb < zhi; zb += R) {
                const uint32_t zl = max(zb, zlo), ze = min(zb + R, zhi);
                CT cc[J];
                VT vv[J];
#pragma unroll
                for (uint32_t k = 0; k < J; k++) { cc[k] = cn[k]; vv[k] = vn[k]; }
                RB braw[J];
#pragma unroll
                for (uint32_t k = 0; k < J; k++) {
                    const uint32_t z = zb + J * slot + k;
                    const bool valid = z >= zl && z < ze;
                    braw[k] = *reinterpret_cast<const RB *>(B + (size_t)(valid ? (uint32_t)cc[k] : 0u) * N + c0);
                }
                if (zb + R < zhi) load_a(zb + R);
#pragma unroll
                for (uint32_t k = 0; k < J; k++) {
                    const uint32_t z = zb + J * slot + k;
                    const float v = (z >= zl && z < ze) ? (float)vv[k] : 0.f;
                    VT bt[CF];
                    __builtin_memcpy(bt, &braw[k], sizeof(RB));
                    float pr[CF];
#pragma unroll
                    for (int i = 0; i < CF; i++) pr[i] = v * (float)bt[i];
                    float *dst = P + pofs(J * slot + k);
                    if constexpr (CF % 4 == 0) {
#pragma unroll
                        for (int i = 0; i < CF; i += 4)
                            *reinterpret_cast<float4 *>(dst + i) = make_float4(pr[i], pr[i + 1], pr[i + 2], pr[i + 3]);
                    } else {
#pragma unroll
                        for (int i = 0; i < CF; i++) dst[i] = pr[i];
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                // rows meeting [zl, ze), S at a time
                for (uint32_t bi = qi0;; bi += S) {
                    const uint32_t i = bi + slot;
                    const uint32_t q = q0 + i;
                    // (both shuffles with every lane active: a shuffle reads only active lanes)
                    const uint32_t en_ = row_end(i), st_ = row_end(i ? i - 1u : 0u);
                    const uint32_t en = q < n_crow ? en_ : 0xffffffffu;
                    const uint32_t st = i == 0u ? sq0 : st_;
                    const bool active = q < n_crow && st < ze;
                    const uint32_t rs = active ? max(st, zl) - zb : 0u, re = active ? min(en, ze) - zb : 0u;
                    const bool is_long = re - rs > solo;
                    float acc[CF];
#pragma unroll
                    for (int k = 0; k < CF; k++) acc[k] = 0.f;
                    if (active && !is_long) {
                        for (uint32_t e = rs; e < re; e++) {
                            const float *src = P + pofs(e);
#pragma unroll
                            for (int k = 0; k < CF; k++) acc[k] += src[k];
                        }
                    }
                    uint64_t lm = __ballot(is_long);
                    while (lm) {  // long rows: the whole wave, slot-strided, one at a time
                        const uint32_t l = (uint32_t)__builtin_ctzll(lm);
                        lm &= ~(slot_bits << l);
                        const uint32_t lrs = (uint32_t)__shfl((int)rs, (int)l, 64), lre = (uint32_t)__shfl((int)re, (int)l, 64);
                        float a2[CF];
#pragma unroll
                        for (int k = 0; k < CF; k++) a2[k] = 0.f;
                        for (uint32_t e = lrs + slot; e < lre; e += S) {
                            const float *src = P + pofs(e);
#pragma unroll
                            for (int k = 0; k < CF; k++) a2[k] += src[k];
                        }
                        wave_reduce_slots<CF>(a2, (int)X);
                        if (slot == l / X) {
#pragma unroll
                            for (int k = 0; k < CF; k++) acc[k] = a2[k];
                        }
                    }
                    if (bi == qi0 && slot == 0u) {  // the row carried in from the previous round
#pragma unroll
                        for (int k = 0; k < CF; k++) acc[k] += carry[k];
                    }
                    const bool closes = active && en <= ze;
                    if (closes) {
                        if (q == q0 && head_open) {
                            if (chain) {
                                merge_chain_publish<CF>(acc, head_rec, w, N, c0, cok);
                                head_mine = true;
                            } else if (cok) {
#pragma unroll
                                for (int k = 0; k < CF; k++) head_rec[(size_t)w * N + c0 + k] = acc[k];
                            }
                        } else if (cok) {
                            store_f32<VT, CF>(C + (size_t)rid[q] * N + c0, acc);
                        }
                    }
                    const uint64_t om = __ballot(active && !closes);  // the row left open at ze
                    const uint64_t am = __ballot(active);
                    if (om) {
                        const uint32_t l = (uint32_t)__builtin_ctzll(om);
#pragma unroll
                        for (int k = 0; k < CF; k++) carry[k] = __shfl(acc[k], (int)((l & ~(X - 1u)) + xl), 64);
                        qi0 = bi + l / X;
                        break;
                    }
                    if (am != ~0ull) {  // the round's rows are done; the next round opens a new row
#pragma unroll
                        for (int k = 0; k < CF; k++) carry[k] = 0.f;
                        qi0 = bi + (uint32_t)__builtin_popcountll(am) / X;
                        break;
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            // carry = the tail row's partial when the wave ends inside a row
            if (chain) {
                if (head_mine && !(head_open && tail_open && q_last == q0))
                    merge_chain_arrive<VT, CF>(w, chain[n_waves + w], rec, head_rec, chain_cnt, rid[q0], C, N, c0, cok,
                                               lane - xl);
                if (tail_open && slot == 0u) {
                    const uint32_t cw_ = chain[w];  // the wave closing the row
                    merge_chain_publish<CF>(carry, rec, w, N, c0, cok);
                    merge_chain_arrive<VT, CF>(cw_, chain[n_waves + cw_], rec, head_rec, chain_cnt, rid[q_last], C, N, c0,
                                               cok, 0u);
                }
            } else {
                if (lane == 0) rec_row[w] = tail_open ? rid[q_last] : 0xffffffffu;
                if (tail_open && slot == 0u && cok) {
#pragma unroll
                    for (int k = 0; k < CF; k++) rec[(size_t)w * N + c0 + k] = carry[k];
                }
            }
        }
    }
}

#endif  // GS_EXPERIMENTS (k_merge_rows)
// rows open across waves: C[r] = (sum of the open partials in wave order) + the
// closing wave's partial, rounded once
template <class VT>
__global__ __launch_bounds__(256) void k_merge_fixup(const uint32_t *__restrict__ rec_row,
                                                     const float *__restrict__ rec,
                                                     const float *__restrict__ head_rec, VT *__restrict__ C,
                                                     uint32_t n_waves, uint32_t N) {
    const uint32_t total = n_waves * N;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const uint32_t g = e / N, c = e % N;
        // every load of the common case (a chain of <= 8 waves) is issued at once, before
        // any of them is tested: one memory latency instead of a chain of dependent ones
        // (the records were written by other XCDs' waves in the previous kernel)
        const uint32_t r = rec_row[g];
        const uint32_t rp = g > 0 ? rec_row[g - 1] : 0xffffffffu;
        uint32_t rr[8];
        float v[8], hv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const bool in = g + k < n_waves, in1 = g + k + 1 < n_waves;
            rr[k] = in ? rec_row[g + k] : 0xffffffffu;
            v[k] = in ? rec[(size_t)(g + k) * N + c] : 0.f;
            hv[k] = in1 ? head_rec[(size_t)(g + k + 1) * N + c] : 0.f;
        }
        if (r == 0xffffffffu || rp == r) continue;
        // sum the open partials in wave order, then the closing wave's head partial
        float s = 0.f;
        uint32_t h = g;
        bool open = true;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            if (open && rr[k] == r) {
                s += v[k];
                h++;
            } else {
                open = false;
            }
        }
        while (open) {  // chains past 8 waves (long rows): 8 waves per step
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const bool in = h + k < n_waves;
                rr[k] = in ? rec_row[h + k] : 0xffffffffu;
                v[k] = in ? rec[(size_t)(h + k) * N + c] : 0.f;
            }
            const uint32_t h0 = h;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                if (open && rr[k] == r) {
                    s += v[k];
                    h++;
                } else {
                    open = false;
                }
            }
            if (h == h0) open = false;
        }
        if (h < n_waves) s += h - g <= 8 ? hv[h - g - 1] : head_rec[(size_t)h * N + c];
        C[(size_t)r * N + c] = (VT)s;
    }
}

}  // namespace gsk
