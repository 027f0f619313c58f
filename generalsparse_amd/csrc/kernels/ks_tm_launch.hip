// ks_tm_launch.hip -- launches of k_mfma_ks_tm (hip_code/mfma_ks_tm.hpp): an uploaded k_mfma_ks
// plan run on token-major activations (gs_linear's single-launch path).
// Built twice (Makefile), as ks_launch.hip is: ks_tm_launch.o holds the fp16 instantiations and the
// entry points, ks_tm_launch_bf16.o (-DGS_KS_BF16_OBJECT) only the bf16 twins behind
// launch_ks_tm_bf16, so the two sets of kernels compile in parallel.
#include "../hip_code/mfma_ks_tm.hpp"
#include "launch_common.hpp"

namespace gs {

namespace {

template <int RT, int MAXG, class ET>
void launch_ks_tm_k(const plan_state &p, const device_arrays &a, const ET *X, ET *Y, uint32_t N, hipStream_t s,
                    const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    const device_plan &d = p.dev;
    GS_CHECK(d.weights == kWNative, "k_mfma_ks_tm reads 16-bit values: a plan with FP8 weights runs its VB = 8 form (launch_ks_tm_w8)");
    if constexpr (!ks_tm_fits(RT, MAXG)) {
        throw gs_error("k_mfma_ks_tm: instantiation not built for this plan (linear_fuses)");
    } else {
        constexpr int W = (int)kKsWaves;
        auto kern = d.ks_nt ? gsk::k_mfma_ks_tm<RT, W, (int)kKsDepth, MAXG, 1, ET> : gsk::k_mfma_ks_tm<RT, W, (int)kKsDepth, MAXG, 0, ET>;
        constexpr size_t lds = gsk::ks_tm_lds_bytes(RT, W);
        grant_lds(d.device, kern, lds);
        const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
        const config_t c = get_config();
        // T token tiles on a 1-D grid of nwg * T, T in prio's bits 18..31 (T = 1: the grid and, but for
        // that bit, the arguments of the plan's own width).  slabs / arrivals: K-split state laid out
        // for T tiles (gs_linear's, T > 1), else the replica's own (one tile, shared with k_mfma_ks)
        const uint32_t T = ks_col_tiles_ct(N, 2);
        GS_CHECK(T >= 1 && T <= kKsTmMaxTiles && (uint64_t)nwg * T <= 0x7fffffffull, "k_mfma_ks_tm: token tiles outside one launch");
        GS_CHECK(d.ksplit == 1 || T == 1 || (slabs && arrivals), "k_mfma_ks_tm: K-split state for more than one token tile");
        const uint32_t prio = (uint32_t)(c.KS_PRIO & 3) | (c.KS_FORCE_TIMEOUT ? 16u : 0u) | (d.ks_gh << 8) | (T << 18);  // (ks_launch.hip)
        hipLaunchKernelGGL(kern, dim3(nwg * T), dim3(64 * W), lds, s, a.t0, (const gsk::u32x4 *)a.tcol,
                           (const gsk::u32x4 *)a.tval, (const gsk::u32x2 *)a.t1, X, Y, (uint32_t)p.K, N, (uint32_t)p.M, d.ksplit,
                           d.ks_ns, nwg, (uint32_t)d.row_base, slabs ? slabs : a.ws, arrivals ? arrivals : a.t2, prio, epi);
        HIP_OK(hipGetLastError());
    }
}

template <int RT, class ET>
void launch_ks_tm_rt(const plan_state &p, const device_arrays &a, const ET *X, ET *Y, uint32_t N, hipStream_t s,
                     const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    switch (p.dev.seg_cap) {  // MAXG: entry groups per lane per k-step
        case 1: launch_ks_tm_k<RT, 1, ET>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        case 2: launch_ks_tm_k<RT, 2, ET>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        case 3: launch_ks_tm_k<RT, 3, ET>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        case 4: launch_ks_tm_k<RT, 4, ET>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        default: throw gs_error("k_mfma_ks_tm: entry groups per k-step outside 1..4");
    }
}

template <class ET>
void launch_ks_tm_et(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                     const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    const ET *x = (const ET *)X;
    ET *y = (ET *)Y;
    switch (p.dev.maxr) {  // RT: 16-row tiles per row block
        case 2: launch_ks_tm_rt<2, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 3: launch_ks_tm_rt<3, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 4: launch_ks_tm_rt<4, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 5: launch_ks_tm_rt<5, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 6: launch_ks_tm_rt<6, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 7: launch_ks_tm_rt<7, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 8: launch_ks_tm_rt<8, ET>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        default: throw gs_error("k_mfma_ks_tm: row tiles outside 2..8");
    }
}

}  // namespace

#ifdef GS_KS_BF16_OBJECT
void launch_ks_tm_bf16(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                       const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    launch_ks_tm_et<gsk::bf16>(p, a, X, Y, N, s, epi, slabs, arrivals);
}
#else
// the bf16 twins (ks_tm_launch_bf16.o)
void launch_ks_tm_bf16(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                       const gsk::epilogue &epi, float *slabs, uint32_t *arrivals);

bool linear_fuses(const plan_state &p, uint32_t n_tokens) {
    const device_plan &d = p.dev;
    // (ks_ctw == 2: a plan built for 17 .. 32 tokens, one tile in its upload's K-split state)
    return p.uploaded && d.mfma && d.ks && !d.nm && !d.pad_rows && n_tokens >= 1 && d.ks_ctw == 2 &&
           d.waves == kKsWaves && d.ks_ap && !d.ks_p8 && !d.ks_wp && !d.ks_persist && d.ks_nt <= 1 &&
           (d.dtype == kF16 || d.dtype == kBF16) && ks_tm_fits(d.maxr, d.seg_cap) && p.K % 8 == 0 && p.K >= 8 &&
           p.K < (1ull << 27) && p.M < (1ull << 32) && get_config().LINEAR_FUSE != 0;
}

void launch_linear_fused(const plan_state &p, int replica, const void *X, void *Y, uint32_t n_tokens, hipStream_t s,
                         const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    GS_CHECK(linear_fuses(p, n_tokens) && (uintptr_t)X % 16 == 0, "k_mfma_ks_tm: not a plan or operand it runs (linear_fuses)");
    GS_CHECK(replica >= 0 && (size_t)replica < p.dev.replicas.size(), "bad replica index");
    const device_arrays &a = p.dev.replicas[(size_t)replica];
    if (p.dev.weights == kWFp8) launch_ks_tm_w8(p, a, X, Y, n_tokens, s, epi, slabs, arrivals);  // ks_tm_w8_launch.hip
    else if (p.dev.dtype == kBF16) launch_ks_tm_bf16(p, a, X, Y, n_tokens, s, epi, slabs, arrivals);
    else launch_ks_tm_et<gsk::f16>(p, a, X, Y, n_tokens, s, epi, slabs, arrivals);
}
#endif  // !GS_KS_BF16_OBJECT

}  // namespace gs
