// kernels/ks_dispatch.hpp -- what the launch files of the k_mfma_ks family (ks_launch.hip, ks_w8_launch.hip,
// ks_tm_launch.hip, ks_tm_group_launch.hip) share: the object selection of the files built more than once, the dispatch from a plan's
// run-time values to template arguments, the prio word and the release-layout predicate.  Host code only.
#pragma once

#include "launch_common.hpp"

#include <type_traits>

// ks_launch.hip, ks_tm_launch.hip and ks_tm_group_launch.hip are built once per value (Makefile, NAME_SRC): the fp16 instantiations
// with every entry point, the bf16 twins, and (ks_tm_launch.hip) the FP8-weight forms, each set of kernels
// in an object of its own so that they compile in parallel
#define GS_KS_F16 0
#define GS_KS_BF16 1
#define GS_KS_W8 2
#ifndef GS_KS_OBJECT
#define GS_KS_OBJECT GS_KS_F16
#endif

namespace gs {

// calls f(std::integral_constant<int, n>{}) for the n of NS equal to v.  No such n: throws gs_error(err); with a
// null err it runs the last n instead (a clamp)
template <int... NS, class F>
void for_value(uint32_t v, const char *err, F &&f) {
    if (((v == (uint32_t)NS ? (f(std::integral_constant<int, NS>{}), true) : false) || ...)) return;
    if (err) throw gs_error(err);
    constexpr int ns[] = {NS...};
    f(std::integral_constant<int, ns[sizeof...(NS) - 1]>{});
}

// the prio argument of the k_mfma_ks kernels: KS_PRIO in bits 0..1, bit 4 (experiments build) forces the
// K-split combine's timeout path (KS_FORCE_TIMEOUT, the test of the device error word), the plan's groups per
// head step in bits 8..17 and k_mfma_ks_tm's token tiles in bits 18..31
inline uint32_t ks_prio_word(const device_plan &d, uint32_t tiles = 0) {
    const config_t c = get_config();
    return (uint32_t)(c.KS_PRIO & 3) | (c.KS_FORCE_TIMEOUT ? 16u : 0u) | (d.ks_gh << 8) | (tiles << 18);
}
// ... its bits below the head-step count, for the launches that carry that count elsewhere or not at all
constexpr uint32_t kKsPrioFlags = 0xffu;

// the layout of the release build's instantiations: 8 waves, the partial tiles beside the stages, 16-bit
// positions, the static grid, KS_NT 0 / 1.  The bf16 twins, the FP8-weight forms and k_mfma_ks_tm are built
// for nothing else (on the host side check_fp8_layout states the same of an mc_layout)
inline bool ks_release_layout(const device_plan &d) {
    return d.waves == kKsWaves && d.ks_ap && !d.ks_p8 && !d.ks_wp && !d.ks_persist && d.ks_nt <= 1;
}

}  // namespace gs
