// ks_w8_launch.hip -- launches of k_mfma_ks_w8 (hip_code/mfma_ks.hpp): k_mfma_ks on a plan uploaded with
// FP8 weights (GS_W_FP8_E4M3: 8 e4m3 codes per entry group and one fp32 scale per row of A).  The release
// layout only (ks_release_layout) -- fp16 activations, 32-column tiles (CT = 2), RT 2 .. 8, MAXG 1 .. 4: what
// check_fp8_layout admits at upload -- in an object of its own, so these instantiations build in parallel
// with ks_launch.o's.
#include "../hip_code/mfma_ks.hpp"
#include "ks_dispatch.hpp"

namespace gs {

namespace {

template <int RT, int MAXG>
void launch_ks_w8_k(const plan_state &p, const device_arrays &a, const gsk::f16 *B, gsk::f16 *C, uint32_t N, hipStream_t s,
                    const gsk::epilogue &epi) {
    const device_plan &d = p.dev;
    constexpr int CT = 2, W = (int)kKsWaves;
    auto kern = d.ks_nt ? gsk::k_mfma_ks_w8<CT, RT, W, (int)kKsDepth, MAXG, 1> : gsk::k_mfma_ks_w8<CT, RT, W, (int)kKsDepth, MAXG, 0>;
    GS_CHECK(gsk::ks_lds_bytes(CT, RT, W, true) <= d.lds_bytes, "k_mfma_ks_w8: LDS size disagrees with the upload");
    grant_lds(d.device, kern, d.lds_bytes);
    const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
    hipLaunchKernelGGL(kern, dim3(nwg, ks_col_tiles_ct(N, CT)), dim3(64 * W), d.lds_bytes, s, a.t0, (const gsk::u32x4 *)a.tcol,
                       (const gsk::u32x2 *)a.tval, (const gsk::u32x2 *)a.t1, B, C, (uint32_t)p.K, N, d.ksplit, d.ks_ns, nwg,
                       (uint32_t)d.row_base, a.ws, a.t2, ks_prio_word(d), epi, (const float *)a.wscale);
    HIP_OK(hipGetLastError());
}

}  // namespace

void launch_ks_w8(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
                  const gsk::epilogue &epi) {
    const device_plan &d = p.dev;
    // (the upload admits nothing else: check_fp8_layout)
    GS_CHECK(d.weights == kWFp8 && a.wscale && d.ks && d.dtype == kF16 && d.ks_ctw == 2 && ks_release_layout(d) && !d.pad_rows,
             "k_mfma_ks_w8: not a plan uploaded with FP8 weights in the release layout");
    GS_CHECK(N == d.lds_N, "k_mfma_ks_w8 runs the plan's dense width");
    // RT: 16-row tiles per row block; MAXG: entry groups per lane per k-step
    for_value<2, 3, 4, 5, 6, 7, 8>(d.maxr, "k_mfma_ks_w8: row tiles outside 2..8", [&](auto rt) {
        for_value<1, 2, 3, 4>(d.seg_cap, "k_mfma_ks_w8: entry groups per k-step outside 1..4", [&](auto maxg) {
            launch_ks_w8_k<decltype(rt)::value, decltype(maxg)::value>(p, a, (const gsk::f16 *)B, (gsk::f16 *)C, N, s, epi);
        });
    });
}

}  // namespace gs
