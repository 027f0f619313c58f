// ks_tm_launch.hip -- launches of k_mfma_ks_tm (hip_code/mfma_ks_tm.hpp): an uploaded k_mfma_ks
// plan run on token-major activations (gs_linear's single-launch path).
// Built three times (Makefile; GS_KS_OBJECT, ks_dispatch.hpp): ks_tm_launch.o holds the fp16 instantiations
// and the entry points, ks_tm_launch_bf16.o only the bf16 twins behind launch_ks_tm_bf16 and
// ks_tm_w8_launch.o only the FP8-weight forms (VB = 8) behind launch_ks_tm_w8, so the three sets of kernels
// compile in parallel.
#include "../hip_code/mfma_ks_tm.hpp"
#include "ks_dispatch.hpp"

namespace gs {

namespace {

// ET: the plan's 16-bit element type.  VB: bits per value of A -- 16, or 8 on a plan uploaded with FP8
// weights (GS_W_FP8_E4M3), whose kernel takes the replica's row scales as one more argument (mfma_ks_tm.hpp)
template <int RT, int MAXG, class ET, int VB>
void launch_ks_tm_k(const plan_state &p, const device_arrays &a, const ET *X, ET *Y, uint32_t N, hipStream_t s,
                    const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    static_assert(ks_tm_fits(RT, MAXG), "k_mfma_ks_tm: the instantiations of ks_tm_fits (linear_fuses)");
    const device_plan &d = p.dev;
    constexpr int W = (int)kKsWaves, D = (int)kKsDepth;
    constexpr size_t lds = gsk::ks_tm_lds_bytes(RT, W);
    const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
    // T token tiles on a 1-D grid of nwg * T, T in prio's bits 18..31 (T = 1: the grid and, but for
    // that bit, the arguments of the plan's own width).  slabs / arrivals: K-split state laid out
    // for T tiles (gs_linear's, T > 1), else the replica's own (one tile, shared with k_mfma_ks)
    const uint32_t T = ks_col_tiles_ct(N, 2);
    GS_CHECK(T >= 1 && T <= kKsTmMaxTiles && (uint64_t)nwg * T <= 0x7fffffffull, "k_mfma_ks_tm: token tiles outside one launch");
    GS_CHECK(d.ksplit == 1 || T == 1 || (slabs && arrivals), "k_mfma_ks_tm: K-split state for more than one token tile");
    auto run = [&](auto kern, auto... w_scale) {
        grant_lds(d.device, kern, lds);
        hipLaunchKernelGGL(kern, dim3(nwg * T), dim3(64 * W), lds, s, a.t0, (const gsk::u32x4 *)a.tcol,
                           (const gsk::u32x4 *)a.tval, (const gsk::u32x2 *)a.t1, X, Y, (uint32_t)p.K, N, (uint32_t)p.M, d.ksplit,
                           d.ks_ns, nwg, (uint32_t)d.row_base, slabs ? slabs : a.ws, arrivals ? arrivals : a.t2,
                           ks_prio_word(d, T), epi, w_scale...);
        HIP_OK(hipGetLastError());
    };
    if constexpr (VB == 8)
        run(d.ks_nt ? gsk::k_mfma_ks_tm<RT, W, D, MAXG, 1, ET, 8, const float *> : gsk::k_mfma_ks_tm<RT, W, D, MAXG, 0, ET, 8, const float *>,
            (const float *)a.wscale);
    else
        run(d.ks_nt ? gsk::k_mfma_ks_tm<RT, W, D, MAXG, 1, ET> : gsk::k_mfma_ks_tm<RT, W, D, MAXG, 0, ET>);
}

// (launch_linear_fused has checked linear_fuses and X's alignment)
template <class ET, int VB>
void launch_ks_tm_et(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                     const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    const device_plan &d = p.dev;
    if constexpr (VB == 8)
        GS_CHECK(d.weights == kWFp8 && a.wscale && d.dtype == kF16, "k_mfma_ks_tm with FP8 weights: not a plan uploaded with FP8 weights");
    else
        GS_CHECK(d.weights == kWNative, "k_mfma_ks_tm reads 16-bit values: a plan with FP8 weights runs its VB = 8 form (launch_ks_tm_w8)");
    // RT: 16-row tiles per row block; MAXG: entry groups per lane per k-step
    for_value<2, 3, 4, 5, 6, 7, 8>(d.maxr, "k_mfma_ks_tm: row tiles outside 2..8", [&](auto rt) {
        for_value<1, 2, 3, 4>(d.seg_cap, "k_mfma_ks_tm: entry groups per k-step outside 1..4", [&](auto maxg) {
            launch_ks_tm_k<decltype(rt)::value, decltype(maxg)::value, ET, VB>(p, a, (const ET *)X, (ET *)Y, N, s, epi, slabs, arrivals);
        });
    });
}

}  // namespace

#if GS_KS_OBJECT == GS_KS_BF16
void launch_ks_tm_bf16(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                       const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    launch_ks_tm_et<gsk::bf16, 16>(p, a, X, Y, N, s, epi, slabs, arrivals);
}
#elif GS_KS_OBJECT == GS_KS_W8
void launch_ks_tm_w8(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                     const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    launch_ks_tm_et<gsk::f16, 8>(p, a, X, Y, N, s, epi, slabs, arrivals);
}
#else
// the bf16 twins (ks_tm_launch_bf16.o); the FP8-weight forms (ks_tm_w8_launch.o): launch_ks_tm_w8, gs_plan.hpp
void launch_ks_tm_bf16(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                       const gsk::epilogue &epi, float *slabs, uint32_t *arrivals);

bool linear_fuses(const plan_state &p, uint32_t n_tokens) {
    const device_plan &d = p.dev;
    // (ks_ctw == 2: a plan built for 17 .. 32 tokens, one tile in its upload's K-split state)
    return p.uploaded && d.mfma && d.ks && !d.nm && !d.pad_rows && n_tokens >= 1 && d.ks_ctw == 2 && ks_release_layout(d) &&
           (d.dtype == kF16 || d.dtype == kBF16) && ks_tm_fits(d.maxr, d.seg_cap) && p.K % 8 == 0 && p.K >= 8 &&
           p.K < (1ull << 27) && p.M < (1ull << 32) && get_config().LINEAR_FUSE != 0;
}

void launch_linear_fused(const plan_state &p, int replica, const void *X, void *Y, uint32_t n_tokens, hipStream_t s,
                         const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    GS_CHECK(linear_fuses(p, n_tokens) && (uintptr_t)X % 16 == 0, "k_mfma_ks_tm: not a plan or operand it runs (linear_fuses)");
    GS_CHECK(replica >= 0 && (size_t)replica < p.dev.replicas.size(), "bad replica index");
    const device_arrays &a = p.dev.replicas[(size_t)replica];
    if (p.dev.weights == kWFp8) launch_ks_tm_w8(p, a, X, Y, n_tokens, s, epi, slabs, arrivals);
    else if (p.dev.dtype == kBF16) launch_ks_tm_bf16(p, a, X, Y, n_tokens, s, epi, slabs, arrivals);
    else launch_ks_tm_et<gsk::f16, 16>(p, a, X, Y, n_tokens, s, epi, slabs, arrivals);
}
#endif

}  // namespace gs
