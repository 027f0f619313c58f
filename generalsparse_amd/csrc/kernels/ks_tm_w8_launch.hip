// ks_tm_w8_launch.hip -- launches of k_mfma_ks_tm's 8-bit form (hip_code/mfma_ks_tm.hpp, VB = 8): the
// kernel on a plan uploaded with FP8 weights (GS_W_FP8_E4M3), behind launch_linear_fused.  The
// instantiations of linear_fuses' domain at fp16 (RT 2 .. 8, MAXG 1 .. 4, KS_NT 0 / 1), in an object of
// their own.
#include "../hip_code/mfma_ks_tm.hpp"
#include "launch_common.hpp"

namespace gs {

namespace {

template <int RT, int MAXG>
void launch_ks_tm_w8_k(const plan_state &p, const device_arrays &a, const gsk::f16 *X, gsk::f16 *Y, uint32_t N, hipStream_t s,
                       const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    static_assert(ks_tm_fits(RT, MAXG), "k_mfma_ks_tm with FP8 weights: the instantiations of ks_tm_fits");
    const device_plan &d = p.dev;
    constexpr int W = (int)kKsWaves;
    // VB = 8 and the scale argument (mfma_ks_tm.hpp)
    auto kern = d.ks_nt ? gsk::k_mfma_ks_tm<RT, W, (int)kKsDepth, MAXG, 1, gsk::f16, 8, const float *>
                        : gsk::k_mfma_ks_tm<RT, W, (int)kKsDepth, MAXG, 0, gsk::f16, 8, const float *>;
    constexpr size_t lds = gsk::ks_tm_lds_bytes(RT, W);
    grant_lds(d.device, kern, lds);
    const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
    const config_t c = get_config();
    // the grid, the tiles and the K-split state: launch_ks_tm_k's (ks_tm_launch.hip), word for word
    const uint32_t T = ks_col_tiles_ct(N, 2);
    GS_CHECK(T >= 1 && T <= kKsTmMaxTiles && (uint64_t)nwg * T <= 0x7fffffffull, "k_mfma_ks_tm with FP8 weights: token tiles outside one launch");
    GS_CHECK(d.ksplit == 1 || T == 1 || (slabs && arrivals), "k_mfma_ks_tm with FP8 weights: K-split state for more than one token tile");
    const uint32_t prio = (uint32_t)(c.KS_PRIO & 3) | (c.KS_FORCE_TIMEOUT ? 16u : 0u) | (d.ks_gh << 8) | (T << 18);
    hipLaunchKernelGGL(kern, dim3(nwg * T), dim3(64 * W), lds, s, a.t0, (const gsk::u32x4 *)a.tcol, (const gsk::u32x4 *)a.tval,
                       (const gsk::u32x2 *)a.t1, X, Y, (uint32_t)p.K, N, (uint32_t)p.M, d.ksplit, d.ks_ns, nwg,
                       (uint32_t)d.row_base, slabs ? slabs : a.ws, arrivals ? arrivals : a.t2, prio, epi, (const float *)a.wscale);
    HIP_OK(hipGetLastError());
}

template <int RT>
void launch_ks_tm_w8_rt(const plan_state &p, const device_arrays &a, const gsk::f16 *X, gsk::f16 *Y, uint32_t N, hipStream_t s,
                        const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    switch (p.dev.seg_cap) {  // MAXG: entry groups per lane per k-step
        case 1: launch_ks_tm_w8_k<RT, 1>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        case 2: launch_ks_tm_w8_k<RT, 2>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        case 3: launch_ks_tm_w8_k<RT, 3>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        case 4: launch_ks_tm_w8_k<RT, 4>(p, a, X, Y, N, s, epi, slabs, arrivals); break;
        default: throw gs_error("k_mfma_ks_tm with FP8 weights: entry groups per k-step outside 1..4");
    }
}

}  // namespace

void launch_ks_tm_w8(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                     const gsk::epilogue &epi, float *slabs, uint32_t *arrivals) {
    const device_plan &d = p.dev;
    // (launch_linear_fused has checked linear_fuses and X's alignment)
    GS_CHECK(d.weights == kWFp8 && a.wscale && d.dtype == kF16, "k_mfma_ks_tm with FP8 weights: not a plan uploaded with FP8 weights");
    const gsk::f16 *x = (const gsk::f16 *)X;
    gsk::f16 *y = (gsk::f16 *)Y;
    switch (d.maxr) {  // RT: 16-row tiles per row block
        case 2: launch_ks_tm_w8_rt<2>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 3: launch_ks_tm_w8_rt<3>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 4: launch_ks_tm_w8_rt<4>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 5: launch_ks_tm_w8_rt<5>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 6: launch_ks_tm_w8_rt<6>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 7: launch_ks_tm_w8_rt<7>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        case 8: launch_ks_tm_w8_rt<8>(p, a, x, y, N, s, epi, slabs, arrivals); break;
        default: throw gs_error("k_mfma_ks_tm with FP8 weights: row tiles outside 2..8");
    }
}

}  // namespace gs
