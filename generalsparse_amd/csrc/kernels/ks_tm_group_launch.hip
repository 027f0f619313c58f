// ks_tm_group_launch.hip -- launches of k_mfma_ks_tm_group (hip_code/mfma_ks_tm.hpp): several k_mfma_ks_tm
// launches of one instantiation as one grid (gs_linear_batch).
// Built twice (Makefile; GS_KS_OBJECT, ks_dispatch.hpp): ks_tm_group_launch.o holds the fp16 instantiations and
// the entry points, ks_tm_group_launch_bf16.o only the bf16 twins behind launch_ks_tm_group_bf16, so the two
// sets of kernels compile in parallel -- and beside ks_tm_launch.hip's objects, whose device code this file
// leaves alone.  The release layout only (linear_fuses): 8 waves, 16-bit positions, RT 2..8, MAXG 1..4, NTL 0 / 1.
#include "../hip_code/mfma_ks_tm.hpp"
#include "ks_dispatch.hpp"

#include <cstring>

namespace gs {

namespace {

template <int RT, int MAXG, class ET>
void launch_ks_tm_group_k(const std::vector<ks_tm_group_item> &it, hipStream_t s) {
    static_assert(ks_tm_fits(RT, MAXG), "k_mfma_ks_tm_group: the instantiations of ks_tm_fits (linear_fuses)");
    constexpr int W = (int)kKsWaves, D = (int)kKsDepth;
    constexpr size_t lds = gsk::ks_tm_lds_bytes(RT, W);
    GS_CHECK(!it.empty() && it.size() <= (size_t)gsk::kKsTmGroupMax, "k_mfma_ks_tm_group: 1..32 entries");
    gsk::ks_tm_group_args args;
    std::memset(&args, 0, sizeof(args));
    uint32_t nwg[gsk::kKsTmGroupMax], tiles[gsk::kKsTmGroupMax];
    for (size_t i = 0; i < it.size(); i++) {
        const plan_state &p = *it[i].p;
        const device_plan &d = p.dev;
        GS_CHECK(it[i].replica >= 0 && (size_t)it[i].replica < d.replicas.size(), "bad replica index");
        const device_arrays &a = d.replicas[(size_t)it[i].replica];
        const uint32_t T = ks_col_tiles_ct(it[i].n_tokens, 2);
        GS_CHECK(T >= 1 && T <= kKsTmMaxTiles, "k_mfma_ks_tm_group: token tiles outside one launch");
        GS_CHECK(d.ksplit == 1 || T == 1 || (it[i].slabs && it[i].arrivals),
                 "k_mfma_ks_tm_group: K-split state for more than one token tile");
        gsk::ks_tm_entry &e = args.e[i];
        e.tbr = a.t0;
        e.tP = (const gsk::u32x4 *)a.tcol;
        e.tV = (const gsk::u32x4 *)a.tval;
        e.steps = (const gsk::u32x2 *)a.t1;
        e.X = it[i].X;
        e.Y = it[i].Y;
        // the state laid out for T tiles (gs_linear_batch's, T > 1), else the replica's own (one tile)
        e.slabs = it[i].slabs ? it[i].slabs : a.ws;
        e.arrivals = it[i].arrivals ? it[i].arrivals : a.t2;
        e.K = (uint32_t)p.K;
        e.N = it[i].n_tokens;
        e.M = (uint32_t)p.M;
        e.S = d.ksplit;
        e.NS = d.ks_ns;
        e.nwg = (uint32_t)d.n_rows_aux * d.ksplit;
        e.row_base = (uint32_t)d.row_base;
        e.gh = d.ks_gh;
        e.epi = it[i].epi;
        nwg[i] = e.nwg;
        tiles[i] = T;
    }
    GS_CHECK(ks_tm_group_layout(nwg, tiles, it.size(), args.begin), "k_mfma_ks_tm_group: the grid passes 2^31 - 1 workgroups");
    args.n = (uint32_t)it.size();
    args.prio = ks_prio_word(it[0].p->dev) & kKsPrioFlags;  // (the head-step counts and the tiles: each entry's)
    auto kern = it[0].p->dev.ks_nt ? gsk::k_mfma_ks_tm_group<RT, W, D, MAXG, 1, ET> : gsk::k_mfma_ks_tm_group<RT, W, D, MAXG, 0, ET>;
    grant_lds(it[0].p->dev.device, kern, lds);
    hipLaunchKernelGGL(kern, dim3(args.begin[it.size()]), dim3(64 * W), lds, s, args);
    HIP_OK(hipGetLastError());
}

template <class ET>
void launch_ks_tm_group_et(const std::vector<ks_tm_group_item> &it, hipStream_t s) {
    const device_plan &d = it[0].p->dev;
    for_value<2, 3, 4, 5, 6, 7, 8>(d.maxr, "k_mfma_ks_tm_group: row tiles outside 2..8", [&](auto rt) {
        for_value<1, 2, 3, 4>(d.seg_cap, "k_mfma_ks_tm_group: entry groups per k-step outside 1..4", [&](auto maxg) {
            launch_ks_tm_group_k<decltype(rt)::value, decltype(maxg)::value, ET>(it, s);
        });
    });
}

}  // namespace

#if GS_KS_OBJECT == GS_KS_BF16
void launch_ks_tm_group_bf16(const std::vector<ks_tm_group_item> &it, hipStream_t s) { launch_ks_tm_group_et<gsk::bf16>(it, s); }
#else
// the bf16 twins (ks_tm_group_launch_bf16.o)
void launch_ks_tm_group_bf16(const std::vector<ks_tm_group_item> &it, hipStream_t s);

uint32_t ks_tm_group_key(const plan_state &p, uint32_t n_tokens, const void *X) {
    const device_plan &d = p.dev;
    // what gs_linear runs as ONE k_mfma_ks_tm launch of 16-bit values: anything else keeps its own path
    if (!linear_fuses(p, n_tokens) || (uintptr_t)X % 16 != 0 || d.weights != kWNative) return 0;
    if (ks_tm_tile_split(n_tokens, ks_tm_tile_cap(d.n_rows_aux, d.ksplit, d.maxr, get_config().LINEAR_WS_KB)).size() != 1) return 0;
    // dtype, NT, RT, MAXG (bit 31: never 0)
    return 1u << 31 | (d.dtype == kBF16 ? 1u << 20 : 0u) | (d.ks_nt << 18) | (d.maxr << 8) | d.seg_cap;
}

void launch_ks_tm_group(const std::vector<ks_tm_group_item> &it, hipStream_t s) {
    GS_CHECK(!it.empty(), "empty group");
    const uint32_t key = ks_tm_group_key(*it[0].p, it[0].n_tokens, it[0].X);
    GS_CHECK(key != 0, "k_mfma_ks_tm_group: not a groupable k_mfma_ks_tm call");
    for (const auto &x : it)
        GS_CHECK(ks_tm_group_key(*x.p, x.n_tokens, x.X) == key, "k_mfma_ks_tm_group: entries of different instantiations");
    // (the key carries the dtype: every entry holds the first one's element type)
    if (it[0].p->dev.dtype == kBF16) launch_ks_tm_group_bf16(it, s);
    else launch_ks_tm_group_et<gsk::f16>(it, s);
}
#endif

}  // namespace gs
