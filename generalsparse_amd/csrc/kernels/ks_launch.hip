// ks_launch.hip -- launches of k_mfma_ks (hip_code/mfma_ks.hpp), the K-split,
// B-stationary matrix-core kernel for tall BMTB row blocks.  Its own translation unit
// so the kernel's instantiations build in parallel with device_plan.hip.
// Built twice (Makefile; GS_KS_OBJECT, ks_dispatch.hpp): ks_launch.o holds the fp16 instantiations and
// every entry point, ks_launch_bf16.o only the bf16 twins behind launch_ks_bf16 / launch_ks_group_bf16, so
// the two sets of kernels compile in parallel.
#include "../hip_code/mfma_ks.hpp"
#ifdef GS_EXPERIMENTS
#include "../hip_code/mfma_bm_exp.hpp"
#endif
#include "ks_dispatch.hpp"

#include <cstring>

namespace gs {

namespace {

// ET: the plan's 16-bit element type (gsk::f16, or gsk::bf16 for GS_BF16 plans).  The bf16 twins are
// built for the release instantiations only (ks_release_layout): the experiments-build variants and
// KS_WPOS below stay fp16 kernels and refuse a bf16 plan
template <int CT, int RT, int MAXG, bool STAMPS = false, int W = (int)kKsWaves, class ET = gsk::f16>
void launch_ks_k(const plan_state &p, const device_arrays &a, const ET *B, ET *C, uint32_t N, hipStream_t s,
                 uint64_t *stamps = nullptr, const gsk::epilogue &epi = gsk::epilogue_identity()) {
    const device_plan &d = p.dev;
    constexpr bool F16 = std::is_same<ET, gsk::f16>::value;
    GS_CHECK(d.weights == kWNative, "k_mfma_ks reads 16-bit values: a plan with FP8 weights runs k_mfma_ks_w8 (launch_ks)");
    if constexpr (!F16) {
        static_assert(W == (int)kKsWaves && !STAMPS, "bf16: the release instantiations only");
        GS_CHECK(ks_release_layout(d),
                 "k_mfma_ks at bf16 is built for 8 waves, 16-bit positions and the apart LDS layout: KS_WPOS and the "
                 "experiments variants (KS_WAVES, KS_POS8, KS_APART = 0, KS_PERSIST) are fp16 kernels");
    }
    // a launch of the k_mfma_ks signature on the plan's static grid
    auto run = [&](auto k, uint32_t threads, uint32_t prio, const uint8_t *tW) {
        grant_lds(d.device, k, d.lds_bytes);
        const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
        hipLaunchKernelGGL(k, dim3(nwg, ks_col_tiles_ct(N, CT)), dim3(threads), d.lds_bytes, s, a.t0, (const gsk::u32x4 *)a.tcol,
                           (const gsk::u32x4 *)a.tval, (const gsk::u32x2 *)a.t1, B, C, (uint32_t)p.K, N, d.ksplit, d.ks_ns, nwg,
                           (uint32_t)d.row_base, a.ws, a.t2, stamps, prio, tW, epi);
        HIP_OK(hipGetLastError());
    };
#ifdef GS_EXPERIMENTS
    // KS_WAVES = 16 (fixed at upload): every instantiation spills (128 VGPRs at 4 waves per
    // SIMD; C2 48-98 us against 14-30 us with 8 waves, profiles/r04a), experiments build only
    if constexpr (F16 && W == (int)kKsWaves && !STAMPS) {
        if (d.waves == 16) {
            launch_ks_k<CT, RT, MAXG, false, 16>(p, a, B, C, N, s, stamps, epi);
            return;
        }
        // KS_WAVES = 12 (N = 32, RT <= 5): three waves per SIMD (r06 A/B)
        if constexpr (CT == 2 && RT <= 5) {
            if (d.waves == 12) {
                launch_ks_k<CT, RT, MAXG, false, 12>(p, a, B, C, N, s, stamps, epi);
                return;
            }
        }
    }
    // GS_KS_DEPTH=1/3/4 (look-ahead sweep against kKsDepth = 2, N = 32 on the C2 / attn / fc1 instantiations and the
    // layer's 112-row ones; plans uploaded with KS_HEAD = 0: the head-step layout is sized by kKsDepth)
    if constexpr (F16 && W == (int)kKsWaves && !STAMPS && CT == 2 &&
                  ((RT == 3 && MAXG == 1) || (RT == 4 && MAXG == 2) || (RT == 5 && MAXG <= 2) || (RT == 7 && MAXG >= 2))) {
        static const int dep = getenv("GS_KS_DEPTH") ? atoi(getenv("GS_KS_DEPTH")) : 0;
        if (dep == 1 || dep == 3 || dep == 4) {
            GS_CHECK(!d.ks_gh && !d.ks_nt && !d.ks_wp, "GS_KS_DEPTH: upload the plan with KS_HEAD = 0, KS_NT = 0 and u16 positions");
            auto kd = dep == 1 ? gsk::k_mfma_ks<CT, RT, W, 1, MAXG, false>
                               : dep == 3 ? gsk::k_mfma_ks<CT, RT, W, 3, MAXG, false> : gsk::k_mfma_ks<CT, RT, W, 4, MAXG, false>;
            run(kd, 64 * W, ks_prio_word(d) & kKsPrioFlags, nullptr);  // (no head steps: ks_gh is 0, checked above)
            return;
        }
    }
    // measured slower than the default form, experiments build only:
    // KS_WAVES = 4 (256-thread workgroups, overlapped LDS), KS_POS8 (8-bit positions), KS_APART = 0
    if constexpr (F16 && W == (int)kKsWaves && !STAMPS) {
        if (d.waves == 4) {
            if constexpr (CT == 2) {
                GS_CHECK(!d.ks_ap, "k_mfma_ks with 4 waves runs the overlapped LDS layout");
                GS_CHECK(!d.ks_wp, "k_mfma_ks: window positions (KS_WPOS) are built for 8 waves");
                auto k4 = d.ks_p8 ? gsk::k_mfma_ks<CT, RT, 4, (int)kKsDepth, MAXG, false, false, gsk::kKsPos8>
                                  : gsk::k_mfma_ks<CT, RT, 4, (int)kKsDepth, MAXG, false, false, gsk::kKsPosU16>;
                GS_CHECK(gsk::ks_lds_bytes(CT, RT, 4, false) <= d.lds_bytes, "k_mfma_ks: LDS size disagrees with the upload");
                run(k4, 256, ks_prio_word(d), nullptr);
                return;
            } else {
                throw gs_error("k_mfma_ks with 4 waves is built for N = 32");
            }
        }
    }
#else
    GS_CHECK(d.waves == kKsWaves && !d.ks_p8 && d.ks_ap,
             "k_mfma_ks with 4 or 16 waves, 8-bit positions or the overlapped LDS layout: experiments build");
#endif
    auto kern = gsk::k_mfma_ks<CT, RT, W, (int)kKsDepth, MAXG, STAMPS, true, gsk::kKsPosU16, 0, ET>;
    if (d.ks_nt) {  // KS_NT: A's groups by non-temporal loads (N = 32 / 128, 8 waves, the apart layout)
        if constexpr ((CT == 2 || CT == 8) && (W == (int)kKsWaves || W == 12) && !STAMPS) {
            GS_CHECK(d.ks_ap && !d.ks_p8, "k_mfma_ks: non-temporal loads are built for the apart layout, 16-bit positions");
            GS_CHECK(d.ks_nt == 1, "k_mfma_ks: KS_NT is built for A's groups (1)");
            kern = gsk::k_mfma_ks<CT, RT, W, (int)kKsDepth, MAXG, false, true, gsk::kKsPosU16, 1, ET>;
        } else {
            throw gs_error("k_mfma_ks: non-temporal loads are built for N = 32 and 128-column tiles, 8 waves");
        }
    }
    if (d.ks_wp) {  // KS_WPOS: one-byte window positions (fp16, N = 32, 8 waves, the apart layout)
        if constexpr (F16 && CT == 2 && W == (int)kKsWaves && !STAMPS) {
            GS_CHECK(d.ks_ap && !d.ks_p8 && !d.ks_persist && a.tw,
                     "k_mfma_ks: window positions are built for the apart LDS layout and the static grid");
            kern = d.ks_nt ? gsk::k_mfma_ks<CT, RT, W, (int)kKsDepth, MAXG, false, true, gsk::kKsPosWin, 1>
                           : gsk::k_mfma_ks<CT, RT, W, (int)kKsDepth, MAXG, false, true, gsk::kKsPosWin, 0>;
        } else {
            throw gs_error("k_mfma_ks: window positions (KS_WPOS) are built for fp16, N = 32, 8 waves");
        }
    }
#ifdef GS_EXPERIMENTS
    if (d.ks_p8) {  // KS_POS8: 8-bit entry positions (N = 32, 8 waves, the apart layout)
        if constexpr (F16 && CT == 2 && W == (int)kKsWaves && !STAMPS) {
            GS_CHECK(d.ks_ap, "k_mfma_ks: 8-bit positions are built with the apart LDS layout");
            kern = gsk::k_mfma_ks<CT, RT, W, (int)kKsDepth, MAXG, false, true, gsk::kKsPos8>;
        } else {
            throw gs_error("k_mfma_ks: 8-bit positions are built for N = 32, 8 waves");
        }
    }
    if (!d.ks_ap) {  // KS_APART = 0: the partial tiles reuse the stage LDS (N = 32, RT <= 5, MAXG <= 2)
        if constexpr (F16 && CT == 2 && RT <= 5 && MAXG <= 2 && W == (int)kKsWaves)
            kern = gsk::k_mfma_ks<CT, RT, W, (int)kKsDepth, MAXG, STAMPS, false>;
        else
            throw gs_error("k_mfma_ks: the overlapped-LDS layout is built for N = 32, RT <= 5, MAXG <= 2");
    }
#endif
#ifdef GS_EXPERIMENTS
    // KS_PERSIST (fixed at upload): a persistent grid of d.ks_persist workgroups pulling units
    if (d.ks_persist) {
        if constexpr (F16 && W == (int)kKsWaves && !STAMPS && (CT == 2 || CT == 8)) {
            GS_CHECK(d.ks_ap && !d.ks_p8 && !d.ks_wp && a.t3 && ks_col_tiles_ct(N, CT) == 1, "k_mfma_ks_persist: 8 waves, apart layout, 16-bit positions, one column tile");
            GS_CHECK(gsk::epilogue_is_identity(epi), "k_mfma_ks_persist takes no epilogue (epilogue_fuses: the post-pass)");
            auto kp = d.ks_nt ? gsk::k_mfma_ks_persist<CT, RT, W, (int)kKsDepth, MAXG, 1>
                              : gsk::k_mfma_ks_persist<CT, RT, W, (int)kKsDepth, MAXG, 0>;
            grant_lds(d.device, kp, d.lds_bytes);
            const uint32_t nunits = (uint32_t)d.n_rows_aux * d.ksplit;
            hipLaunchKernelGGL(kp, dim3(std::min(d.ks_persist, nunits)), dim3(64 * W), d.lds_bytes, s, a.t0,
                               (const gsk::u32x4 *)a.tcol, (const gsk::u32x4 *)a.tval, (const gsk::u32x2 *)a.t1, B, C,
                               (uint32_t)p.K, N, d.ksplit, d.ks_ns, nunits, (uint32_t)d.row_base, a.ws, a.t2, ks_prio_word(d), a.t3);
            HIP_OK(hipGetLastError());
            return;
        } else {
            throw gs_error("k_mfma_ks_persist is built for N = 32 and 128-column tiles, 8 waves");
        }
    }
#else
    GS_CHECK(!d.ks_persist, "k_mfma_ks_persist is an experiments-build kernel");
#endif
    // the LDS this instantiation needs at the plan's range width, against what the upload sized
    GS_CHECK(gsk::ks_lds_bytes(CT, RT, W, d.ks_ap) <= d.lds_bytes, "k_mfma_ks: LDS size disagrees with the upload");
    run(kern, 64 * W, ks_prio_word(d), (const uint8_t *)a.tw);
}

// the plan's (CT, RT, MAXG) as template arguments.  CT: 16-column tiles per workgroup, ks_col_tiles_ct(N, CT)
// workgroups across N; RT: 16-row tiles per row block (the upload builds RT >= 2); MAXG: entry groups per
// lane per k-step, 4 for any other count
template <class ET>
void launch_ks_et(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
                  const gsk::epilogue &epi) {
    const device_plan &d = p.dev;
    for_value<1, 2, 4, 8>(d.ks_ctw, "k_mfma_ks: bad column tile count", [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        constexpr const char *rt_err = CT == 8 ? "k_mfma_ks: 128-column tiles take row blocks of up to 48 rows"
                                               : "k_mfma_ks: row tiles outside 2..8 (6..8 for N <= 32)";
        for_value<2, 3, 4, 5, 6, 7, 8>(d.maxr, rt_err, [&](auto rt) {
            constexpr int RT = decltype(rt)::value;
            auto run = [&](auto maxg) {
                launch_ks_k<CT, RT, decltype(maxg)::value, false, (int)kKsWaves, ET>(p, a, (const ET *)B, (ET *)C, N, s, nullptr, epi);
            };
            if constexpr (CT == 8) {
                // 128 columns per workgroup: row blocks of up to 48 rows (ks_ct_rt), and only the (RT, MAXG)
                // pairs that do not spill (ks_ct8_fits): MAXG up to 3 at RT 2, 1 at RT 3
                if constexpr (RT > 3) {
                    throw gs_error(rt_err);
                } else {
                    GS_CHECK(ks_ct8_fits(RT, d.seg_cap), "k_mfma_ks: 128-column tile instantiation not built for this plan");
                    if constexpr (RT == 2) for_value<1, 2, 3>(d.seg_cap, nullptr, run);
                    else run(std::integral_constant<int, 1>{});
                }
            } else if constexpr (CT > 2 && RT > 5) {  // RT 6..8 are built for N <= 32 (CT <= 2)
                throw gs_error(rt_err);
            } else {
                for_value<1, 2, 3, 4>(d.seg_cap, nullptr, run);
            }
        });
    });
}

#ifdef GS_EXPERIMENTS
template <int CT, int RT, int W, bool STAMPS = false>
void launch_bm_k(const plan_state &p, const device_arrays &a, const gsk::f16 *B, gsk::f16 *C, uint32_t N, hipStream_t s,
                 uint64_t *stamps = nullptr) {
    const device_plan &d = p.dev;
    auto kern = gsk::k_mfma_bm<CT, RT, W, (int)gsk::bm_nbt(CT, RT), STAMPS>;
    GS_CHECK(gsk::bm_lds_bytes(CT, RT, W) <= d.lds_bytes, "k_mfma_bm: LDS size disagrees with the upload");
    grant_lds(d.device, kern, d.lds_bytes);
    const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
    hipLaunchKernelGGL(kern, dim3(nwg, ks_col_tiles(N)), dim3(64 * W), d.lds_bytes, s, a.t0, (const uint2 *)a.tcol, a.t1,
                       (const gsk::f16 *)a.tval, B, C, (uint32_t)p.K, N, d.ksplit, d.ks_ns, nwg, (uint32_t)d.row_base,
                       a.ws, a.t2, stamps);
    HIP_OK(hipGetLastError());
}

template <int CT, int RT>
void launch_bm2_k(const plan_state &p, const device_arrays &a, const gsk::f16 *B, gsk::f16 *C, uint32_t N, hipStream_t s) {
    const device_plan &d = p.dev;
    auto kern = gsk::k_mfma_bm2<CT, RT>;
    GS_CHECK(128u + (size_t)d.ks_ns * 32u * 32u * CT <= d.lds_bytes, "k_mfma_bm2: LDS size disagrees with the upload");
    grant_lds(d.device, kern, d.lds_bytes);
    const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
    hipLaunchKernelGGL(kern, dim3(nwg, ks_col_tiles(N)), dim3(64 * RT), d.lds_bytes, s, a.t0, (const uint2 *)a.tcol, a.t1,
                       (const gsk::f16 *)a.tval, B, C, (uint32_t)p.K, N, d.ksplit, d.ks_ns, nwg, (uint32_t)d.row_base,
                       a.ws, a.t2);
    HIP_OK(hipGetLastError());
}

template <int CT, int RT, int NVB>
void launch_kb_k(const plan_state &p, const device_arrays &a, const gsk::f16 *B, gsk::f16 *C, uint32_t N, hipStream_t s) {
    const device_plan &d = p.dev;
    // GS_KB_DEBUG=2/3 (diagnostics, wrong results): no value loads / no B loads
    static const int dbg = getenv("GS_KB_DEBUG") ? atoi(getenv("GS_KB_DEBUG")) : 0;
    auto kern = gsk::k_mfma_kb<CT, RT, (int)kKsWaves, (int)kKsDepth, NVB>;
    if constexpr (CT == 2 && NVB <= 2) {  // (N = 32 only)
        if (dbg == 2) kern = gsk::k_mfma_kb<CT, RT, (int)kKsWaves, (int)kKsDepth, NVB, false, 2>;
        if (dbg == 3) kern = gsk::k_mfma_kb<CT, RT, (int)kKsWaves, (int)kKsDepth, NVB, false, 3>;
    }
    GS_CHECK(d.waves == kKsWaves && gsk::kb_lds_bytes(CT, RT, kKsWaves, NVB) <= d.lds_bytes,
             "k_mfma_kb: LDS size disagrees with the upload");
    grant_lds(d.device, kern, d.lds_bytes);
    const uint32_t nwg = (uint32_t)d.n_rows_aux * d.ksplit;
    hipLaunchKernelGGL(kern, dim3(nwg, ks_col_tiles(N)), dim3(64 * kKsWaves), d.lds_bytes, s, a.t0, (const uint2 *)a.tcol,
                       a.t1, (const gsk::f16 *)a.tval, B, C, (uint32_t)p.K, N, d.ksplit, d.ks_ns, nwg,
                       (uint32_t)d.row_base, a.ws, a.t2, nullptr, ks_prio_word(d) & kKsPrioFlags);  // (the bitmap layout has no head steps)
    HIP_OK(hipGetLastError());
}

#endif  // GS_EXPERIMENTS

}  // namespace

#if GS_KS_OBJECT == GS_KS_F16
#ifdef GS_EXPERIMENTS
void launch_bm(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s) {
    const device_plan &d = p.dev;
    const gsk::f16 *b = (const gsk::f16 *)B;
    gsk::f16 *c = (gsk::f16 *)C;
    GS_CHECK(N == d.lds_N, "k_mfma_bm runs the plan's dense width");
    // CT: 16-column tiles per workgroup (4 for any wider N); RT: 16-row tiles per row block
    for_value<1, 2, 4>(ks_ct(N), nullptr, [&](auto ct) {
        constexpr int CT = decltype(ct)::value;
        for_value<1, 2, 3, 4, 5, 6>(d.maxr, "k_mfma_bm: row tiles outside 1..6", [&](auto rt) {
            constexpr int RT = decltype(rt)::value;
            if (d.bmkb)  // NVB: 1, 2, else 4
                for_value<1, 2, 4>(d.seg_cap, nullptr, [&](auto nvb) { launch_kb_k<CT, RT, decltype(nvb)::value>(p, a, b, c, N, s); });
            else if (d.bm2) launch_bm2_k<CT, RT>(p, a, b, c, N, s);
            else if (d.waves == 4) launch_bm_k<CT, RT, 4>(p, a, b, c, N, s);
            else launch_bm_k<CT, RT, 8>(p, a, b, c, N, s);
        });
    });
}

#else
void launch_bm(const plan_state &, const device_arrays &, const void *, void *, uint32_t, hipStream_t) {
    throw gs_error("k_mfma_bm is an experiments-build kernel (make -C generalsparse_amd/csrc exp)", -2);
}
#endif
#endif  // GS_KS_OBJECT == GS_KS_F16

// ---- grouped launches (gs_spmm_batch): N = 32 (CT = 2), 8 waves, one instantiation per group
namespace {
template <int RT, int MAXG, int W = (int)kKsWaves, class ET = gsk::f16>
void launch_ks_group_k(const std::vector<ks_group_item> &it, uint32_t N, hipStream_t s) {
    constexpr bool AP = W == (int)kKsWaves;
    constexpr bool F16 = std::is_same<ET, gsk::f16>::value;
    if constexpr (!F16)  // (ks_group_key admits bf16 plans of the release layout only)
        GS_CHECK(ks_release_layout(it[0].p->dev), "k_mfma_ks_group at bf16: 8 waves, 16-bit positions");
#ifdef GS_EXPERIMENTS
    if constexpr (F16 && W == (int)kKsWaves) {
        if (it[0].p->dev.waves == 4) {  // KS_WAVES = 4: 256-thread workgroups, overlapped LDS
            launch_ks_group_k<RT, MAXG, 4>(it, N, s);
            return;
        }
    }
    auto kern = gsk::k_mfma_ks_group<2, RT, W, (int)kKsDepth, MAXG, gsk::kKsPosU16, AP, 0, ET>;
    if constexpr (F16) {
        if (it[0].p->dev.ks_p8) kern = gsk::k_mfma_ks_group<2, RT, W, (int)kKsDepth, MAXG, gsk::kKsPos8, AP>;
    }
#else
    GS_CHECK(!it[0].p->dev.ks_p8, "k_mfma_ks_group: 8-bit positions are an experiments-build layout");
    auto kern = gsk::k_mfma_ks_group<2, RT, W, (int)kKsDepth, MAXG, gsk::kKsPosU16, AP, 0, ET>;
#endif
    if constexpr (AP) {
        if (it[0].p->dev.ks_nt) kern = gsk::k_mfma_ks_group<2, RT, W, (int)kKsDepth, MAXG, gsk::kKsPosU16, true, 1, ET>;
    }
    if (it[0].p->dev.ks_wp) {  // KS_WPOS (ks_group_key: every entry of the group has the layout)
        if constexpr (F16 && AP) {
            kern = it[0].p->dev.ks_nt ? gsk::k_mfma_ks_group<2, RT, W, (int)kKsDepth, MAXG, gsk::kKsPosWin, true, 1>
                                      : gsk::k_mfma_ks_group<2, RT, W, (int)kKsDepth, MAXG, gsk::kKsPosWin, true, 0>;
        } else {
            throw gs_error("k_mfma_ks_group: window positions (KS_WPOS) are built for fp16, 8 waves");
        }
    }
    GS_CHECK(!it.empty() && it.size() <= (size_t)gsk::kKsGroupMax, "k_mfma_ks_group: 1..32 entries");
    gsk::ks_group_args args;
    std::memset(&args, 0, sizeof(args));
    size_t lds = 0;
    uint32_t wg = 0;
    for (size_t i = 0; i < it.size(); i++) {
        const plan_state &p = *it[i].p;
        const device_plan &d = p.dev;
        const device_arrays &a = d.replicas[(size_t)it[i].replica];
        GS_CHECK(gsk::ks_lds_bytes(2, RT, W, AP) <= d.lds_bytes, "k_mfma_ks_group: LDS size disagrees with the upload");
        lds = std::max(lds, d.lds_bytes);
        gsk::ks_entry &e = args.e[i];
        e.tbr = a.t0;
        e.tP = (const gsk::u32x4 *)a.tcol;
        e.tV = (const gsk::u32x4 *)a.tval;
        e.steps = (const gsk::u32x2 *)a.t1;
        e.B = it[i].B;
        e.C = it[i].C;
        e.slabs = a.ws;
        e.arrivals = a.t2;
        e.K = (uint32_t)p.K;
        e.S = d.ksplit;
        e.NS = d.ks_ns;
        e.nwg = (uint32_t)d.n_rows_aux * d.ksplit;
        e.row_base = (uint32_t)d.row_base;
        e.pad0 = d.ks_gh;  // the entry's head-step group count (ks_body's prio bits 8..17)
        GS_CHECK(d.ks_wp == it[0].p->dev.ks_wp && (!d.ks_wp || a.tw), "k_mfma_ks_group: entries of different position forms");
        e.tW = (const uint8_t *)a.tw;
        e.epi = it[i].epi;
        args.begin[i] = wg;
        // each entry starts on a multiple of 8 workgroups (idle ones in between exit at once), so
        // its entry-relative block numbers share XCDs as the global ones do (xcd_block)
        wg += (e.nwg + 7u) & ~7u;
    }
    args.begin[it.size()] = wg;
    args.n = (uint32_t)it.size();
    args.N = N;
    args.pad[0] = ks_prio_word(it[0].p->dev) & kKsPrioFlags;  // (the head-step counts: each entry's pad0)
    grant_lds(it[0].p->dev.device, kern, lds);
    hipLaunchKernelGGL(kern, dim3(wg, ks_col_tiles(N)), dim3(64 * W), lds, s, args);
    HIP_OK(hipGetLastError());
}

template <class ET>
void launch_ks_group_et(const std::vector<ks_group_item> &it, uint32_t N, hipStream_t s) {
    const device_plan &d = it[0].p->dev;
    for_value<2, 3, 4, 5, 6, 7, 8>(d.maxr, "k_mfma_ks_group: row tiles outside 2..8", [&](auto rt) {
        for_value<1, 2, 3, 4>(d.seg_cap, nullptr, [&](auto maxg) {  // (MAXG 4 for any other count, as launch_ks_et)
            launch_ks_group_k<decltype(rt)::value, decltype(maxg)::value, (int)kKsWaves, ET>(it, N, s);
        });
    });
}
}  // namespace

#if GS_KS_OBJECT == GS_KS_BF16
void launch_ks_bf16(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
                    const gsk::epilogue &epi) {
    launch_ks_et<gsk::bf16>(p, a, B, C, N, s, epi);
}
void launch_ks_group_bf16(const std::vector<ks_group_item> &it, uint32_t N, hipStream_t s) {
    launch_ks_group_et<gsk::bf16>(it, N, s);
}
#else
// the bf16 twins (ks_launch_bf16.o)
void launch_ks_bf16(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
                    const gsk::epilogue &epi);
void launch_ks_group_bf16(const std::vector<ks_group_item> &it, uint32_t N, hipStream_t s);

uint32_t ks_group_key(const plan_state &p, uint32_t N) {
    const device_plan &d = p.dev;
    const bool w8 = d.waves == kKsWaves && d.ks_ap, w4 = d.waves == 4 && !d.ks_ap;
    if (!p.uploaded || !d.mfma || !d.ks || d.pad_rows || N != 32 || d.lds_N != 32 || d.ks_persist) return 0;
    if (d.weights != kWNative) return 0;  // FP8 weights: no grouped kernel is built, a batch runs single launches
    if (!ks_release_layout(d)) {
        // bf16: the grouped kernel's twins are the release instantiations (as launch_ks_k).  fp16 also groups
        // window positions (KS_WPOS, 8 waves) and, in the experiments build, 8-bit positions and 4 waves
        // with the overlapped layout; any other layout runs as single launches (which refuse it themselves)
        if (d.dtype == kBF16) return 0;
#ifdef GS_EXPERIMENTS
        if (!(w8 || w4) || (d.ks_wp && !w8)) return 0;
#else
        if (!w8 || d.ks_p8) return 0;
#endif
    }
    // position form, dtype, NT, waves, P8, RT, MAXG: fp16 and bf16 entries, and u16 and window
    // positions, never share a launch
    return (d.ks_wp ? 1u << 21 : 0u) | (d.dtype == kBF16 ? 1u << 20 : 0u) | (d.ks_nt << 18) | (w4 ? 1u << 17 : 0u) | (d.ks_p8 ? 1u << 16 : 0u) | (d.maxr << 8) |
           d.seg_cap;
}

void launch_ks_group(const std::vector<ks_group_item> &it, uint32_t N, hipStream_t s) {
    GS_CHECK(!it.empty(), "empty group");
    const uint32_t key = ks_group_key(*it[0].p, N);
    GS_CHECK(key != 0, "k_mfma_ks_group: not a groupable k_mfma_ks plan");
    for (const auto &x : it) GS_CHECK(ks_group_key(*x.p, N) == key, "k_mfma_ks_group: entries of different instantiations");
    // (the key carries the dtype: every entry holds the first one's element type)
    if (it[0].p->dev.dtype == kBF16) launch_ks_group_bf16(it, N, s);
    else launch_ks_group_et<gsk::f16>(it, N, s);
}

void launch_ks(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
               const gsk::epilogue &epi) {
    GS_CHECK(N == p.dev.lds_N, "k_mfma_ks runs the plan's dense width");
    GS_CHECK(p.dev.ks_ctw == ks_ct_rt(N, p.dev.maxr) || (p.dev.ks_ctw == 4 && ks_ct_rt(N, p.dev.maxr) == 8 &&
                                                         !ks_ct8_fits(p.dev.maxr, p.dev.seg_cap)),
             "k_mfma_ks: column tiles disagree with the upload");
    if (p.dev.weights == kWFp8) launch_ks_w8(p, a, B, C, N, s, epi);  // ks_w8_launch.hip
    else if (p.dev.dtype == kBF16) launch_ks_bf16(p, a, B, C, N, s, epi);
    else launch_ks_et<gsk::f16>(p, a, B, C, N, s, epi);
}

#ifdef GS_EXPERIMENTS  // diagnostics (s_memtime stamps)
// diagnostic: k_mfma_bm at N = 32, 65..80-row blocks, 8 waves (stamps: mfma_bm_exp.hpp)
void debug_bm_timeline(const plan_state &p, const void *B, void *C, uint32_t N, hipStream_t s, uint64_t *host,
                       size_t n_host) {
    const device_plan &d = p.dev;
    GS_CHECK(N == 32 && d.maxr == 5 && d.waves == 8, "k_mfma_bm timeline build: N=32, RT=5, 8 waves only");
    const size_t n = (size_t)d.n_rows_aux * d.ksplit * 8 * 16;
    uint64_t *dst = nullptr;
    HIP_OK(hipMalloc(&dst, n * 8));
    HIP_OK(hipMemsetAsync(dst, 0, n * 8, s));
    launch_bm_k<2, 5, 8, true>(p, d.replicas[0], (const gsk::f16 *)B, (gsk::f16 *)C, N, s, dst);
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipMemcpy(host, dst, std::min(n, n_host) * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dst);
}

// diagnostic: the C2 shape (N = 32, 65..80-row blocks, <= 128 entry groups per k-step)
void debug_ks_timeline(const plan_state &p, const void *B, void *C, uint32_t N, hipStream_t s, uint64_t *host,
                       size_t n_host) {
    const device_plan &d = p.dev;
    GS_CHECK(N == 32 && d.maxr >= 2 && d.maxr <= 5 && d.seg_cap <= 2 && d.waves == kKsWaves && d.dtype == kF16,
             "k_mfma_ks timeline build: fp16, N=32, RT 2..5, MAXG <= 2, 8 waves only");
    const size_t n = (size_t)d.n_rows_aux * d.ksplit * ks_col_tiles(N) * kKsWaves * 32;
    uint64_t *dst = nullptr;
    HIP_OK(hipMalloc(&dst, n * 8));
    HIP_OK(hipMemsetAsync(dst, 0, n * 8, s));
    const device_arrays &a = d.replicas[0];
    const gsk::f16 *b = (const gsk::f16 *)B;
    gsk::f16 *c = (gsk::f16 *)C;
    for_value<2, 3, 4, 5>(d.maxr, nullptr, [&](auto rt) {
        for_value<1, 2>(d.seg_cap, nullptr, [&](auto maxg) {
            launch_ks_k<2, decltype(rt)::value, decltype(maxg)::value, true>(p, a, b, c, N, s, dst);
        });
    });
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipMemcpy(host, dst, std::min(n, n_host) * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dst);
}

#else
void debug_bm_timeline(const plan_state &, const void *, void *, uint32_t, hipStream_t, uint64_t *, size_t) {
    throw gs_error("timeline builds are diagnostics of the experiments build (make -C generalsparse_amd/csrc exp)", -2);
}
void debug_ks_timeline(const plan_state &, const void *, void *, uint32_t, hipStream_t, uint64_t *, size_t) {
    throw gs_error("timeline builds are diagnostics of the experiments build (make -C generalsparse_amd/csrc exp)", -2);
}
#endif  // GS_EXPERIMENTS

#endif  // GS_KS_OBJECT == GS_KS_BF16

}  // namespace gs
