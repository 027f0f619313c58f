// device_plan.hip -- uploads a compiled plan to HBM in the layout of its
// kernel family and dispatches the gfx950 kernels of hip_code/ through the launch files
// (gather_launch.hip, mfma_launch.hip, ks_launch.hip); k_combine_parts is launched here.
#include "../hip_code/parts.hpp"
#include "../hip_code/host_layouts.hpp"
#include "../host/index_compress.hpp"
#include "../host/device_layout.hpp"
#include "../host/gather_layout.hpp"
#include "launch_common.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

namespace gs {

namespace {

constexpr uint64_t kPad = 64;  // extra zeroed entries after every A stream

template <class T>
T *dev_copy(device_plan &d, const std::vector<T> &h, uint64_t pad = 0) {
    size_t n = h.size() + pad;
    T *p = nullptr;
    HIP_OK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    d.allocations.push_back(p);
    if (!h.empty()) HIP_OK(hipMemcpy(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    if (pad) HIP_OK(hipMemset(p + h.size(), 0, pad * sizeof(T)));
    d.bytes_A += h.size() * sizeof(T);
    return p;
}

std::vector<uint32_t> to_u32(const std::vector<uint64_t> &v, const char *what) {
    std::vector<uint32_t> o(v.size());
    for (size_t i = 0; i < v.size(); i++) {
        GS_CHECK(v[i] <= 0xffffffffull, std::string(what) + " exceeds 32 bits");
        o[i] = (uint32_t)v[i];
    }
    return o;
}

// An index array a gather kernel reads through gsk::idx_at.  With MODEL_DRIVEN_COMPRESS and
// an exact formula for it (index_compress.cc; the reference prints the same formulas into its
// kernels, code_generator.cc:2618-3063) nothing is uploaded (linear / branch / cycle kinds) or
// only the narrow residuals are; otherwise the u32 array.  type_ori: the array's compressed
// data type, which bounds the residual width as in the reference's if_residual.
uint32_t *upload_index(device_plan &d, const std::vector<uint64_t> &v, data_type type_ori, const char *what,
                       gsk::idx_formula &f) {
    f = gsk::idx_formula();
    if (get_config().MODEL_DRIVEN_COMPRESS) {
        const index_compression c = analyze_index_compression(v, type_ori, get_config().BRANCH_COMPRESS_MAX_SIZE);
        if (device_formula_of(c, f)) {
            d.index_formulas++;
            if (f.kind == gsk::IDX_RESIDUAL_U8) {
                d.index_bytes_saved += v.size() * 3;
                return (uint32_t *)dev_copy(d, std::vector<uint8_t>(c.res.begin(), c.res.end()), 4);
            }
            if (f.kind == gsk::IDX_RESIDUAL_U16) {
                d.index_bytes_saved += v.size() * 2;
                return (uint32_t *)dev_copy(d, std::vector<uint16_t>(c.res.begin(), c.res.end()), 2);
            }
            d.index_bytes_saved += v.size() * 4;
            return nullptr;
        }
    }
    return dev_copy(d, to_u32(v, what));
}

uint32_t *upload_index(device_plan &d, const meta_data_set &m, POS_TYPE pos, const char *name, int sb,
                       gsk::idx_formula &f) {
    return upload_index(d, m.u(pos, name, sb), m.get_element(pos, name, sb)->meta_data_arr->get_compress_data_type(), name,
                        f);
}

}  // namespace

// MP_COL_PARTS upload: columns ranked by degree (as MP_COL_PERM), rank r in partition r % P at
// position base[r % P] + r / P of the gathered B (k_permute_rows); per partition its entries in
// row order (so every row's partial sums its entries in the plan's order), the merge-path wave
// ranges of that CSR, the in-launch combine state and (partitions >= 1) an fp32 output that
// k_add_parts adds to C in partition order (deterministic)
static void upload_col_parts(plan_state &p, device_arrays &a, const std::vector<uint64_t> &col,
                             const universal_array &vals) {
    device_plan &d = p.dev;
    const kernel_spec &sp = p.cg->get_kernel_spec();
    const meta_data_set &m = *p.meta;
    const int sb = p.cg->get_sub_matrix_id();
    const uint32_t P = d.mp_parts;
    const uint64_t K = p.K;
    const auto &rows = m.u(GLOBAL_META, "nz_row_indices", sb);
    const uint64_t row_num = row_num_of_sub_matrix(m, sb);
    // MP_HUB_COLS = H (P = 2): partition 0 = the H densest columns (the hubs, whose B rows stay in
    // the XCDs' L2s, so a round of that pass never waits on an Infinity-Cache / HBM gather),
    // partition 1 = the rest; else ranks are dealt round-robin over the P partitions
    const uint64_t hub = P == 2 ? (uint64_t)std::max<int64_t>(0, get_config().MP_HUB_COLS) : 0;
    const col_parts split = split_col_parts(rows, col, K, P, hub);
    a.cperm = dev_copy(d, split.gather);
    const uint32_t Nd = (uint32_t)std::max<int64_t>(1, get_config().DENSE_MATRIX_SIZE);
    const size_t bb = (size_t)K * Nd * elem_bytes(d.dtype);
    HIP_OK(hipMalloc(&a.bperm, std::max<size_t>(bb, 16)));
    d.allocations.push_back(a.bperm);
    const uint64_t target = merge_path_target(Nd, elem_bytes(d.dtype));
    a.pp.assign((size_t)P * kMpPartPtrs, nullptr);
    d.mp_part_W.assign(P, 0);
    d.mp_part_rows.assign(P, 0);
    d.mp_part_fin.assign(P, 0);
    for (uint32_t x = 0; x < P; x++) {
        const std::vector<uint64_t> &rx = split.parts[x].rows;
        const std::vector<uint32_t> &cx = split.parts[x].cols;
        std::vector<float> vx(rx.size());
        for (size_t i = 0; i < vx.size(); i++) vx[i] = (float)vals.read_float_from_arr(split.parts[x].src[i]);
        void **pp = &a.pp[(size_t)x * kMpPartPtrs];
        if (d.col_bytes == 2) {
            std::vector<uint16_t> c16(cx.begin(), cx.end());
            pp[MP_PART_COL] = dev_copy(d, c16, kPad);
        } else {
            pp[MP_PART_COL] = dev_copy(d, cx, kPad);
        }
        pp[MP_PART_VAL] = dev_copy(d, vx, kPad);
        std::vector<uint64_t> lr, ln;
        merge_path_levels(rx, row_num, (uint64_t)sp.work_size, lr, ln);
        gsk_host::merge_path_layout lay;
        std::string why;
        GS_CHECK(gsk_host::merge_path_device_layout(rx, row_num, lr, ln, (uint64_t)sp.work_size, (uint32_t)d.row_base, target,
                                                     lay, why, d.n_out_rows, 2 * target),
                 "merge-path layout of column partition " + std::to_string(x) + ": " + why);
        pp[MP_PART_WZ] = dev_copy(d, lay.wz);
        pp[MP_PART_WQ] = dev_copy(d, lay.wq);
        pp[MP_PART_ENDS] = dev_copy(d, lay.ends);
        pp[MP_PART_RID] = dev_copy(d, lay.rid);
        pp[MP_PART_EMPTY] = lay.empty.empty() ? nullptr : dev_copy(d, lay.empty);
        const uint32_t W = (uint32_t)(lay.wz.size() - 1);
        pp[MP_PART_WS] = dev_copy(d, std::vector<float>((size_t)W * Nd, 0.f));
        pp[MP_PART_WS2] = dev_copy(d, std::vector<float>((size_t)W * Nd, 0.f));
        pp[MP_PART_T0] = dev_copy(d, std::vector<uint32_t>(W, 0xffffffffu));
        pp[MP_PART_CHAIN] = dev_copy(d, lay.chain);
        pp[MP_PART_CNT] = dev_copy(d, std::vector<uint32_t>(W, 0u));
        if (x > 0) pp[MP_PART_OUT] = dev_copy(d, std::vector<float>((size_t)d.n_out_rows * Nd, 0.f));
        d.mp_part_W[x] = W;
        d.mp_part_rows[x] = (uint32_t)lay.ends.size();
        d.mp_part_fin[x] = (uint32_t)lay.empty.size();
    }
    // the whole-matrix CSR is not uploaded: part 0's columns stand in for it (non-null)
    a.col = a.pp[MP_PART_COL];
    a.val = a.pp[MP_PART_VAL];
}

// the plan's column indices (u16 when they fit, else u32) and values (plan dtype) of
// one replica, padded for the kernels' aligned over-reads
void upload_csr(plan_state &p, device_arrays &a) {
    const kernel_spec &sp = p.cg->get_kernel_spec();
    const meta_data_set &m = *p.meta;
    const int sb = p.cg->get_sub_matrix_id();
    device_plan &d = p.dev;
    HIP_OK(hipSetDevice(d.device));
    const auto &col = m.u(GLOBAL_META, sp.interleaved ? "nz_col_indices_after_interlance_storage" : "nz_col_indices", sb);
    auto vals = m.get_element(GLOBAL_META, sp.interleaved ? "nz_vals_after_interlance_storage" : "nz_vals", sb)->meta_data_arr;
    const uint64_t nnz = col.size();
    if (d.mp_parts > 1) {
        upload_col_parts(p, a, col, *vals);
        return;
    }
    if (d.col_perm) {
        // MP_COL_PERM: columns renumbered by degree (most nonzeros first, ties by column), so
        // the B rows the power-law hubs gather share 128-B lines and stay in L2; each launch
        // first gathers B into that order (k_permute_rows).  Only the device copy of the
        // column indices changes; the order of every row's entries, so every sum, is the same
        const uint64_t hot = (uint64_t)std::max<int64_t>(0, get_config().MP_PERM_HOT);
        const column_ranks order = column_order(col, p.K, hot);
        const std::vector<uint32_t> &perm = order.perm, &rank = order.rank;
        std::vector<uint32_t> c32(nnz);
        for (uint64_t i = 0; i < nnz; i++) c32[i] = rank[col[i]];
        if (d.col_bytes == 2) {
            std::vector<uint16_t> c16(c32.begin(), c32.end());
            a.col = dev_copy(d, c16, kPad);
        } else {
            a.col = dev_copy(d, c32, kPad);
        }
        d.perm_scatter = get_config().MP_PERM_SCATTER != 0;
        a.cperm = dev_copy(d, d.perm_scatter ? rank : perm);  // scatter: new place of each column
        // the gathered B: K rows of the plan's dense width (launches check N <= ws_n = that width)
        const size_t bb = (size_t)p.K * (size_t)std::max<int64_t>(1, get_config().DENSE_MATRIX_SIZE) * elem_bytes(d.dtype);
        HIP_OK(hipMalloc(&a.bperm, std::max<size_t>(bb, 16)));
        d.allocations.push_back(a.bperm);
    } else if (d.col_bytes == 2) {
        std::vector<uint16_t> c16(col.begin(), col.end());
        a.col = dev_copy(d, c16, kPad);
    } else {
        a.col = dev_copy(d, to_u32(col, "column index"), kPad);
    }
    // the values in the plan's storage type (convert_values: what gs_convert_values returns)
    std::vector<float> v(nnz);
    for (uint64_t i = 0; i < nnz; i++) v[i] = (float)vals->read_float_from_arr(i);
    if (d.dtype == kF32) {
        a.val = dev_copy(d, v, kPad);
    } else {
        std::vector<uint16_t> h(nnz);
        convert_values(v.data(), nnz, d.dtype, h.data());
        a.val = dev_copy(d, h, kPad);
    }
}

namespace {

// what a family's upload reads: the plan, the replica being filled and the plan's arrays
struct upload_ctx {
    plan_state &p;
    device_plan &d;
    device_arrays &a;
    const meta_data_set &m;
    const kernel_spec &sp;
    const int sb, dtype;
    const std::vector<uint64_t> &rows, &col;
    const universal_array &vals;
    const mc_layout &mc;
    const uint64_t row_num, out_lo, out_hi;
};

// K-split combine state: zeroed fp32 slabs, the arrival counters and (err) the replica's device
// error word after them
void upload_ksplit_state(device_plan &d, device_arrays &a, size_t slab_floats, size_t counters, bool err) {
    a.ws = dev_copy(d, std::vector<float>(slab_floats, 0.f));
    a.t2 = dev_copy(d, std::vector<uint32_t>(counters + (err ? 1u : 0u), 0u));
    if (err) d.err_at = counters;
}

// col-direction BMTs that are 2:4 panels: sparse matrix cores, self-contained blocks
void upload_nm(device_plan &d, device_arrays &a, const mc_layout &mc, uint64_t bmts) {
    d.nm = true;
    d.kernel = mc.nm_ks ? "k_nm_mfma_ks" : (mc.nm4 ? "k_nm_mfma4" : "k_nm_mfma");
    d.nm4 = mc.nm4;
    d.nm_nt = mc.nm_nt;
    d.nm_tiles = mc.nm_T;
    d.KC = mc.nm_S;
    d.n_rows_aux = mc.nm_rows;
    d.n_units = bmts;
    d.waves = mc.nm_ks ? 4 : gsk::kNmWaves;
    d.nm_ks = mc.nm_ks;
    d.ksplit = mc.nm_ks || mc.nm4 ? mc.nm_split : 1;
    d.ncs = mc.nm_ncs;
    a.tcol = dev_copy(d, mc.nm_blk);
    d.bytes_tile = d.bytes_A;
    if (mc.nm_ks && mc.nm_split > 1) {  // fp32 slabs (one 64 x N tile per row group and K range) + counters
        const uint64_t ngr = (mc.nm_rows + 255) / 256 * 4;
        upload_ksplit_state(d, a, (size_t)ngr * mc.nm_split * 64 * mc.N, (size_t)ngr, false);
    }
    if (mc.nm4 && mc.nm_split > 1) {  // tagged fp32 slabs (256 x N per unit), counters + the device error word
        const uint64_t nb = (mc.nm_rows + 255) / 256;
        upload_ksplit_state(d, a, (size_t)nb * mc.nm_split * 256 * mc.N, (size_t)nb, true);
    }
}

// tall row blocks: K split over workgroups, wave-autonomous (k_mfma_ks)
void upload_ks(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const mc_layout &mc = u.mc;
    const ks_tiles &kt = mc.ks;
    d.mfma = true;
    d.ks = true;
    d.kernel = "k_mfma_ks";
    d.lds_N = mc.N;
    d.ksplit = kt.S;
    d.ks_ns = kt.NS;
    d.maxr = kt.RT;
    d.rpw_max = kt.RMAX;
    d.seg_cap = kt.MAXG;
    d.waves = kt.W;
    d.lds_bytes = kt.lds_bytes;
    const uint64_t nb = mc.tbr.size() - 1;
    d.n_rows_aux = nb;
    const size_t before = d.bytes_A;
    d.ks_gcap = kt.GCAP;
    d.ks_ctw = kt.CT;
    d.ks_ap = kt.AP;
    d.ks_p8 = kt.P8;
    d.ks_wp = kt.WP;
    d.ks_nt = kt.NT;
    d.ks_gh = kt.GH;
    d.ks_persist = (uint32_t)std::max<int64_t>(0, get_config().KS_PERSIST);
    if (d.ks_persist) a.t3 = dev_copy(d, std::vector<uint32_t>(9, 0u));  // 8 XCD heads + the exit count
    a.t0 = dev_copy(d, to_u32(mc.tbr, "BMTB first_row_indices"));
    GS_CHECK(!(kt.WP && d.ks_persist), "KS_WPOS: window positions are not built for the persistent grid (KS_PERSIST)");
    a.tcol = kt.P8 || kt.WP ? (void *)dev_copy(d, kt.pos8) : (void *)dev_copy(d, kt.pos);
    if (kt.WP) a.tw = dev_copy(d, kt.win);
    // FP8 weights: 8 bytes per group (e4m3 codes) in place of the 8 x u16
    a.tval = d.weights == kWFp8 ? (void *)dev_copy(d, kt.val8) : (void *)dev_copy(d, kt.val);
    d.ks_val_slots = kt.val.size();
    d.ks_hash = ks_layout_hash(kt);
    a.t1 = dev_copy(d, kt.steps);
    d.bytes_tile = d.bytes_A - before;
    // ... and the rows' scales (M fp32, indexed as the epilogue's bias is): bytes of A, not of its tiles
    if (d.weights == kWFp8) a.wscale = dev_copy(d, mc.w8_scale);
    if (kt.S > 1) {  // the error word: ks_slab_wait
        const uint32_t CT = kt.CT, nt = ks_col_tiles_ct(mc.N, CT);
        upload_ksplit_state(d, a, (size_t)nb * kt.S * nt * 256 * kt.RT * CT, (size_t)nb * nt, true);
    }
}

// bitmap records, fragments expanded in registers (k_mfma_bm)
void upload_bm(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const mc_layout &mc = u.mc;
    const bm_tiles &bt = mc.bm;
    d.mfma = true;
    d.bm = true;
    d.bm2 = bt.v2;
    d.bmkb = bt.kb;
    d.seg_cap = bt.NVB;  // k_mfma_kb: KB of values per k-step
    d.kernel = bt.kb ? "k_mfma_kb" : bt.v2 ? "k_mfma_bm2" : "k_mfma_bm";
    d.lds_N = mc.N;
    d.ksplit = bt.S;
    d.ks_ns = bt.NS;
    d.maxr = bt.RT;
    d.rpw_max = bt.RMAX;
    d.waves = bt.W;
    d.lds_bytes = bt.lds_bytes;
    const uint64_t nb = mc.tbr.size() - 1;
    d.n_rows_aux = nb;
    const size_t before = d.bytes_A;
    a.t0 = dev_copy(d, to_u32(mc.tbr, "BMTB first_row_indices"));
    a.tcol = dev_copy(d, bt.rec);
    a.t1 = dev_copy(d, bt.sbase);
    a.tval = dev_copy(d, bt.val);
    d.bytes_tile = d.bytes_A - before;
    if (bt.S > 1) {
        const uint32_t nt = ks_col_tiles(mc.N), CT = ks_ct(mc.N);
        a.ws = dev_copy(d, std::vector<float>((size_t)nb * bt.S * nt * 256 * bt.RT * CT, 0.f));
        // arrival counters: per (row block, column tile), per row tile too for k_mfma_bm2
        a.t2 = dev_copy(d, std::vector<uint32_t>((size_t)nb * nt * (bt.v2 ? bt.RT : 1u) + 1u, 0u));
        if (bt.kb) d.err_at = (uint64_t)nb * nt;  // k_mfma_kb: the device error word after the counters
    }
}

// the other fp16 BMTB plans: dense tiles per (BMTB, column chunk) (k_mfma_rows)
void upload_rows(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const mc_layout &mc = u.mc;
    const mfma_tiles &t = mc.rows;
    d.mfma = true;
    d.kernel = "k_mfma_rows";
    d.lds_N = mc.N;
    d.KC = 1u << t.lgKC; d.nc = t.nc; d.maxr = t.RT; d.rpw_max = t.RMAX; d.RSB = t.lgKC;
    d.seg_cap = t.gmax;
    d.mfma_glds = mc.rows_glds; d.mfma_nbg = mc.rows_nbg; d.mfma_wct = mc.rows_wct; d.mfma_maxa = mc.rows_maxa;
    d.mfma_flags = mc.rows_flags;
    const uint64_t nb = mc.tbr.size() - 1;
    d.ncs = mc.rows_ncs;
    d.ksplit = mc.rows_ksplit;
    if (d.ksplit > 1) upload_ksplit_state(d, a, (size_t)nb * d.ksplit * t.RMAX * mc.N, (size_t)nb, false);
    d.waves = kMfmaThreads / 64; d.lds_bytes = t.lds_bytes;
    const size_t before = d.bytes_A;
    a.t0 = dev_copy(d, to_u32(mc.tbr, "BMTB first_row_indices"));
    a.t1 = dev_copy(d, t.seg_start);
    a.tcol = dev_copy(d, t.pos);
    a.tval = dev_copy(d, t.val);
    d.bytes_tile = d.bytes_A - before;
    d.n_rows_aux = nb;
}

// matrix-core row blocks for fp16 plans with BMTBs (tried before the other kernels)
bool upload_row_blocks(upload_ctx &u) {
    switch (u.mc.kind) {
        case mc_layout::KS: upload_ks(u); return true;
        case mc_layout::BM: upload_bm(u); return true;
        case mc_layout::ROWS: upload_rows(u); return true;
        default: return false;
    }
}

void upload_thread_total(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const meta_data_set &m = u.m;
    const int sb = u.sb;
    const auto &fn = m.u(THREAD_META, "first_nz_indices", sb);
    const auto &fr = m.u(THREAD_META, "first_row_indices", sb);
    for (size_t i = 0; i < fr.size(); i++)
        GS_CHECK(fr[i] == i, "thread_total kernel needs one row per BMT (fixed_row_block_size 1)");
    bool al4 = true, al8 = true;
    for (uint64_t x : fn) { al4 &= (x % 4 == 0); al8 &= (x % 8 == 0); }
    d.scf = al8 ? 8 : (al4 ? 4 : 1);
    a.a0 = upload_index(d, m, THREAD_META, "first_nz_indices", sb, d.f0);
    if (m.is_exist(GLOBAL_META, "original_nz_row_indices", sb)) {
        a.a1 = upload_index(d, m, GLOBAL_META, "original_nz_row_indices", sb, d.f1);
        d.n_rows_aux = m.u(GLOBAL_META, "original_nz_row_indices", sb).size();
    } else {
        // rows were not sorted: the row of BMT i is i (the reference indexes C by it
        // directly); an identity array unless the formulas are on
        std::vector<uint64_t> order(u.row_num);
        for (uint64_t r = 0; r < u.row_num; r++) order[r] = r;
        a.a1 = upload_index(d, order, UNSIGNED_INT, "row order", d.f1);
        d.n_rows_aux = u.row_num;
    }
    d.n_units = fn.size() - 1;
}

// LDS-stationary B (k_lds_rows*: fp32 / fp16 kernels) for a BMTB plan, when its tiles fit
void upload_lds_tiles(upload_ctx &u, const std::vector<uint32_t> &rp) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const meta_data_set &m = u.m;
    const int sb = u.sb, dtype = u.dtype;
    lds_tiles t;
    std::string why;
    const uint32_t Nd = (uint32_t)get_config().DENSE_MATRIX_SIZE;
    size_t budget = (size_t)std::min<int64_t>(get_config().SHARED_MEM_TOTAL_SIZE, 160 * 1024);
    // LDS_DMA (fp32 at N = 32): chunks by LDS-DMA into two buffers (k_lds_rows_dma), at most
    // 80 KB per workgroup so two share a CU (their barriers and DMA waits interleave; the auto
    // K split below makes the grid two per CU): C2 fp32 (20,2) 37.7 -> 34.4 us (r06r)
    const bool dma = dtype == 0 && Nd == 32 && get_config().LDS_DMA != 0;
    if (dma) budget = std::min<size_t>(budget, 80 * 1024);
    // LDS_KSPLIT: S workgroups per BMTB, each over ncs consecutive chunks of K
    // (every K range non-empty), fp32 slabs + one arrival counter per BMTB.  0 (auto):
    // plans of under 128 BMTBs split K until ~256 workgroups (a workgroup's time
    // is its nonzeros: C2 fp32 (20,2) 41.5 us = (40,4) in 2 K ranges 44.5 us,
    // profiles/r06f_lds_ksplit.txt, so full grids gain nothing from a split)
    // With LDS-DMA (two workgroups per CU) the auto split aims at ~512 workgroups.
    const uint64_t nbt0 = m.u(TBLOCK_META, "first_row_indices", sb).size() - 1;
    const int64_t cfg_ks = get_config().LDS_KSPLIT;
    const uint64_t wg_aim = dma ? 512 : 256;
    const uint32_t want = cfg_ks > 0 ? (uint32_t)cfg_ks
                                     : (nbt0 * 2 <= wg_aim ? (uint32_t)std::max<uint64_t>(1, wg_aim / std::max<uint64_t>(nbt0, 1)) : 1u);
    if (!build_lds_tiles(m.u(TBLOCK_META, "first_row_indices", sb), m.u(TBLOCK_META, "first_BMW_indices", sb),
                         m.u(WARP_META, "first_row_indices", sb), rp, u.col, u.p.K, Nd, elem_bytes(dtype), budget, t, why,
                         dma, want))
        return;
    d.lds = true;
    d.lds_dma = dma;
    d.kernel = t.maxr == 8 ? "k_lds_rows_rs" : (dma ? "k_lds_rows_dma" : "k_lds_rows");
    const uint32_t ncs = (t.nc + std::min(want, t.nc) - 1) / std::min(want, t.nc);
    d.ksplit = (t.nc + ncs - 1) / ncs;
    d.ncs = ncs;
    d.lds_N = Nd;
    d.KC = t.KC; d.nc = t.nc; d.RSB = t.RSB; d.rpw_max = t.rpw_max; d.seg_cap = t.seg_cap;
    d.waves = t.waves; d.maxr = t.maxr; d.lds_bytes = t.lds_bytes;
    const size_t before = d.bytes_A;
    a.t0 = dev_copy(d, to_u32(m.u(TBLOCK_META, "first_row_indices", sb), "BMTB first_row_indices"));
    a.t1 = dev_copy(d, t.seg_start);
    a.t2 = dev_copy(d, t.seg_row_off);
    a.tcol = dev_copy(d, t.tcol, kPad);
    if (dtype == 0) {
        std::vector<float> v(t.src.size());
        for (size_t i = 0; i < v.size(); i++)
            v[i] = t.src[i] == ~0u ? 0.f : (float)u.vals.read_float_from_arr(t.src[i]);
        a.tval = dev_copy(d, v, kPad);
    } else {
        std::vector<uint16_t> v(t.src.size());
        for (size_t i = 0; i < v.size(); i++)
            v[i] = t.src[i] == ~0u ? 0 : value_bits16((float)u.vals.read_float_from_arr(t.src[i]), dtype);
        a.tval = dev_copy(d, v, kPad);
    }
    d.bytes_tile = d.bytes_A - before;
    if (d.ksplit > 1) {
        const uint64_t nbt = m.u(TBLOCK_META, "first_row_indices", sb).size() - 1;
        a.ws = dev_copy(d, std::vector<float>((size_t)nbt * d.ksplit * t.rpw_max * Nd, 0.f));
        a.t3 = dev_copy(d, std::vector<uint32_t>((size_t)nbt, 0u));
    }
}

void upload_warp_total(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const meta_data_set &m = u.m;
    const kernel_spec &sp = u.sp;
    const int sb = u.sb;
    // BMW rows and BMTB->BMW map: formulas for k_warp_rows; k_lds_rows reads the arrays
    auto upload_groups = [&](bool formulas) {
        if (formulas) {
            a.a0 = upload_index(d, m, sp.group_level, "first_row_indices", sb, d.f0);
            if (sp.tblock_parent) a.a1 = upload_index(d, m, TBLOCK_META, "first_BMW_indices", sb, d.f1);
        } else {
            a.a0 = dev_copy(d, to_u32(m.u(sp.group_level, "first_row_indices", sb), "BMW first_row_indices"));
            if (sp.tblock_parent)
                a.a1 = dev_copy(d, to_u32(m.u(TBLOCK_META, "first_BMW_indices", sb), "first_BMW_indices"));
        }
    };
    if (sp.tblock_parent) d.n_rows_aux = m.u(TBLOCK_META, "first_BMW_indices", sb).size() - 1;  // BMTB count
    std::vector<uint32_t> rp = csr_row_ptr(u.rows, u.row_num);
    a.a2 = dev_copy(d, rp);
    d.n_units = m.u(sp.group_level, "first_row_indices", sb).size() - 1;
    {
        const auto &gr = m.u(sp.group_level, "first_row_indices", sb);
        uint64_t mx = 0;
        for (size_t i = 0; i + 1 < gr.size(); i++) mx = std::max<uint64_t>(mx, gr[i + 1] - gr[i]);
        d.bmw_rows_max = (uint32_t)mx;
        d.mean_row_nnz = u.row_num ? (double)rp.back() / (double)u.row_num : 0.0;
    }
    d.scf = 4;
    if (sp.tblock_parent && upload_row_blocks(u)) {
        upload_groups(true);  // the gather fallback at other dense widths
        return;
    }
    // LDS-stationary B pays off for row blocks of >= 16 rows in BMWs of >= 2 rows
    // (C2: 20x2 31 us vs 40 us gathered; 4x1 62 us): otherwise the gather kernel.  LDS_STAGE_ANY lifts
    // that rule (off by default): the only way to the one-row-BMW forms of k_lds_rows (MAXR = 1)
    bool lds_worth = false;
    if (sp.tblock_parent) {
        const auto &tr = m.u(TBLOCK_META, "first_row_indices", sb);
        const auto &wr = m.u(WARP_META, "first_row_indices", sb);
        uint64_t mt = 0, mw = 0;
        for (size_t i = 0; i + 1 < tr.size(); i++) mt = std::max<uint64_t>(mt, tr[i + 1] - tr[i]);
        for (size_t i = 0; i + 1 < wr.size(); i++) mw = std::max<uint64_t>(mw, wr[i + 1] - wr[i]);
        lds_worth = (mt >= 16 && mw >= 2) || get_config().LDS_STAGE_ANY != 0;
    }
    if (sp.tblock_parent && get_config().LDS_STAGE_B && lds_worth && u.dtype != kBF16) upload_lds_tiles(u, rp);
    upload_groups(!d.lds);
}

void upload_block_total(upload_ctx &u) {
    device_plan &d = u.d;
    u.a.a0 = upload_index(d, u.m, TBLOCK_META, "first_row_indices", u.sb, d.f0);
    u.a.a2 = dev_copy(d, csr_row_ptr(u.rows, u.row_num));
    d.n_units = u.m.u(TBLOCK_META, "first_row_indices", u.sb).size() - 1;
    d.scf = 4;
    upload_row_blocks(u);
}

void upload_bitmap_segment(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const meta_data_set &m = u.m;
    const int sb = u.sb;
    const auto &fn = m.u(THREAD_META, "first_nz_indices", sb);
    uint64_t nb = fn.size() - 1;
    for (uint64_t i = 0; i < nb; i++) {
        GS_CHECK(fn[i + 1] - fn[i] <= 64, "bitmap kernel needs BMTs of at most 64 nnz");
        GS_CHECK(fn[i] % 8 == 0, "bitmap kernel needs 8-aligned BMTs");
    }
    a.a0 = upload_index(d, m, THREAD_META, "first_nz_indices", sb, d.f0);
    a.a1 = upload_index(d, m, THREAD_META, "first_row_indices", sb, d.f1);
    // real row starts (the plan's thread_bit_map also carries the forced BMW heads)
    a.m0 = dev_copy(d, gsk_host::row_start_masks(u.rows, fn));
    a.a2 = dev_copy(d, to_u32(m.u(THREAD_META, "segment_ptr", sb), "segment_ptr"));
    a.a3 = dev_copy(d, to_u32(m.u(THREAD_META, "segment_empty_row_indices", sb), "segment_empty_row_indices"));
    d.n_units = nb;
    d.scf = 4;
    if (u.dtype == kF32) {
        d.needs_memset = true;
        return;
    }
    // fp16 / bf16 C: rows whose nonzeros span BMTs accumulate in an fp32 workspace and
    // are rounded once by k_finalize_rows, which also writes the empty rows (no memset)
    const std::vector<uint32_t> list = bitmap_finalize_rows(u.rows, fn, csr_row_ptr(u.rows, u.row_num), u.row_num, u.p.M,
                                                            d.row_base, u.out_lo, u.out_hi);
    a.a4 = dev_copy(d, list);
    a.ws = dev_copy(d, std::vector<float>((size_t)u.p.M * std::max<uint32_t>(1, (uint32_t)get_config().DENSE_MATRIX_SIZE), 0.f));
    d.ws_n = (uint32_t)get_config().DENSE_MATRIX_SIZE;
    d.n_fin = list.size();
}

// chunks of one row: col-direction BMTs, or col-direction BMWs / BMTBs (the spec's
// first array names the level)
void upload_row_chunks(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const meta_data_set &m = u.m;
    const kernel_spec &sp = u.sp;
    const int sb = u.sb;
    const POS_TYPE L = sp.arrays[0].rfind("WARP_META", 0) == 0
                           ? WARP_META
                           : (sp.arrays[0].rfind("TBLOCK_META", 0) == 0 ? TBLOCK_META : THREAD_META);
    const auto &fn = m.u(L, "first_nz_indices", sb);
    const auto &fr = m.u(L, "first_row_indices_without_ending", sb);
    GS_CHECK(fn.size() == fr.size() + 1 && !fr.empty(), "col-direction plan: chunk arrays disagree");
    std::vector<uint32_t> br = to_u32(fr, "first_row_indices_without_ending");
    a.a0 = upload_index(d, m, L, "first_nz_indices", sb, d.f0);
    a.a1 = upload_index(d, m, L, "first_row_indices_without_ending", sb, d.f1);
    d.n_units = br.size();
    d.scf = 4;
    d.span = gsk_host::row_chunk_span(br.size());
    if (sp.interleaved && sp.interleave_parent != GLOBAL_META) {
        // per-parent interleaving: BMT b of parent j (first BMT F, first nonzero P, n BMTs)
        // has its i-th nonzero at P + (b - F) + i * n (k_row_chunks ilv_base / ilv_stride)
        const POS_TYPE pp = (POS_TYPE)sp.interleave_parent;
        const auto &pf = m.u(pp, "first_BMT_indices", sb);
        const auto &pn = m.u(pp, "first_nz_indices", sb);
        GS_CHECK(pf.size() == pn.size() && !pf.empty() && pf.back() == br.size(),
                 "interleaved parents: first_BMT_indices / first_nz_indices disagree with the BMTs");
        std::vector<uint32_t> ib(br.size()), is(br.size());
        for (size_t j = 0; j + 1 < pf.size(); j++)
            for (uint64_t b = pf[j]; b < pf[j + 1]; b++) {
                ib[b] = (uint32_t)(pn[j] + (b - pf[j]));
                is[b] = (uint32_t)(pf[j + 1] - pf[j]);
            }
        a.a2 = dev_copy(d, ib);
        a.a3 = dev_copy(d, is);
    }
    // rows shared by two waves' BMT ranges accumulate in an fp32 workspace; the
    // finalize pass rounds them and writes the rows without BMTs (no memset)
    std::vector<uint32_t> list = gsk_host::row_chunk_finalize_rows(br, u.p.M, d.span, (uint32_t)d.row_base);
    list.erase(std::remove_if(list.begin(), list.end(), [&](uint32_t r) { return r < u.out_lo || r >= u.out_hi; }),
               list.end());
    d.ws_n = (uint32_t)std::max<int64_t>(1, get_config().DENSE_MATRIX_SIZE);
    a.ws = dev_copy(d, std::vector<float>((size_t)u.p.M * d.ws_n, 0.f));
    if (!list.empty()) a.a4 = dev_copy(d, list);
    d.n_fin = list.size();
}

// wave ranges decoded from the merge-path levels; S = 64/X slots per wave as launched
void upload_merge_path(upload_ctx &u) {
    device_plan &d = u.d;
    device_arrays &a = u.a;
    const POS_TYPE L = u.sp.merge_level;
    const uint32_t Nd = (uint32_t)std::max<int64_t>(1, get_config().DENSE_MATRIX_SIZE);
    d.scf = 8;
    d.ws_n = Nd;
    if (d.mp_parts > 1) {  // the partitions' layouts are built with their CSRs (upload_col_parts)
        d.n_units = d.mp_part_W[0];
        d.kernel = "k_merge_path";
        return;
    }
    const uint64_t target = merge_path_target(Nd, elem_bytes(u.dtype));  // >= one round per wave
    gsk_host::merge_path_layout lay;
    std::string why;
    GS_CHECK(gsk_host::merge_path_device_layout(u.rows, u.row_num, u.m.u(L, "first_row_indices_without_ending", u.sb),
                                                 u.m.u(L, "first_nz_indices", u.sb), (uint64_t)u.sp.work_size,
                                                 (uint32_t)d.row_base, target, lay, why, d.n_out_rows, 2 * target),
             "merge-path layout: " + why);
    a.a0 = dev_copy(d, lay.wz);
    a.a1 = dev_copy(d, lay.wq);
    a.a2 = dev_copy(d, lay.ends);
    a.a3 = dev_copy(d, lay.rid);
    a.a4 = dev_copy(d, lay.empty);
    d.n_fin = lay.empty.size();
    d.n_units = lay.wz.size() - 1;
    d.n_rows_aux = lay.ends.size();
    a.ws = dev_copy(d, std::vector<float>((size_t)d.n_units * Nd, 0.f));
    a.ws2 = dev_copy(d, std::vector<float>((size_t)d.n_units * Nd, 0.f));
    a.t0 = dev_copy(d, std::vector<uint32_t>(d.n_units, 0xffffffffu));
    a.t1 = dev_copy(d, lay.chain);                                 // split-row chains
    a.t2 = dev_copy(d, std::vector<uint32_t>(d.n_units, 0u));     // their arrival counters
    const config_t cfg = get_config();
    d.mp_rows = cfg.MP_ROWS;
    d.mp_solo = (uint32_t)std::max<int64_t>(1, cfg.MP_SOLO);
    d.kernel = d.mp_rows ? "k_merge_rows" : "k_merge_path";
}

}  // namespace

void upload_plan(plan_state &p, int dtype, int device, int weights, const float *row_scale) {
    GS_CHECK(p.cg && p.cg->is_compiled(), "plan must be compiled before upload");
    GS_CHECK(dtype_ok(dtype), "dtype must be 0 (fp32), 1 (fp16) or 2 (bf16)");
    GS_CHECK(weights == kWNative || weights == kWFp8, "weights must be 0 (native) or 1 (FP8 e4m3)");
    GS_CHECK(weights == kWFp8 || !row_scale, "row_scale goes with FP8 weights");
    GS_CHECK(weights != kWFp8 || dtype == kF16, "FP8 weights run with fp16 activations only (dtype f16), not bf16 / f32");
    free_device(p);
    HIP_OK(hipSetDevice(device));
    const kernel_spec &sp = p.cg->get_kernel_spec();
    const meta_data_set &m = *p.meta;
    const int sb = p.cg->get_sub_matrix_id();
    device_plan &d = p.dev;
    d = device_plan();
    d.device = device;
    d.dtype = dtype;
    // a parent-indexed sub-matrix (row_nz_matrix_div_operator) writes a scratch output whose
    // row r is its row index r (capi.cc combines the scratch outputs into C)
    const bool pidx = p.parent_row_base >= 0;
    d.row_base = pidx ? 0 : m.scalar(GLOBAL_META, "begin_row_index", sb);
    // output rows this plan writes: all of C for the undivided matrix; a sub-matrix of a
    // row division (§8f rank 3) owns [begin_row_index, begin_row_index + its rows) only
    const uint64_t out_lo = sb == 0 || pidx ? 0 : d.row_base;
    const uint64_t out_hi = sb == 0 ? p.M : d.row_base + row_num_of_sub_matrix(m, sb);
    d.n_out_rows = out_hi;
    d.out_lo = out_lo;
    const auto &rows = m.u(GLOBAL_META, "nz_row_indices", sb);
    // interleaved storage (§8f rank 2): the kernel streams the permuted arrays
    const auto &col = m.u(GLOBAL_META, sp.interleaved ? "nz_col_indices_after_interlance_storage" : "nz_col_indices", sb);
    auto vals = m.get_element(GLOBAL_META, sp.interleaved ? "nz_vals_after_interlance_storage" : "nz_vals", sb)->meta_data_arr;
    if (sp.interleaved && sp.interleave_parent == GLOBAL_META)
        d.ilv = (uint32_t)m.u(GLOBAL_META, "BMT_size_of_each_blk", sb).at(0);
    uint64_t nnz = col.size();
    GS_CHECK(nnz < 0xffffffffull - kPad, "nnz exceeds 32-bit offsets");
    d.nnz_stored = nnz;
    device_arrays a;
    // FP8 weights: every refusal before the first allocation (the plan is then simply not uploaded)
    const fp8_request w8{row_scale};
    if (weights == kWFp8) {
        GS_CHECK(sb == 0 && !pidx, "FP8 weights: an undivided plan only (this is a sub-matrix of a row division)");
        GS_CHECK(row_num_of_sub_matrix(m, sb) == p.M, "FP8 weights: a plan without padded rows only");
    }
    // the matrix-core layout (device_layout.cc: the same choice the emitted program makes)
    const mc_layout mc = choose_matrix_core_layout(m, sp, sb, p.K, dtype, weights == kWFp8 ? &w8 : nullptr);
    if (weights == kWFp8) check_fp8_layout(mc, p.K);
    d.weights = weights;
    if (mc.kind == mc_layout::NM) {
        upload_nm(d, a, mc, m.u(THREAD_META, "first_nz_indices", sb).size() - 1);
        d.replicas.push_back(a);
        p.uploaded = true;
        return;
    }
    // A streams: narrowest column type that holds Kc-1 (u16 when Kc <= 65536).  fp16 BMTB
    // plans try the matrix cores first: their kernels never read the CSR arrays, which
    // are then uploaded only if a launch at another dense width falls back to a gather
    // kernel (ensure_csr), so A is not resident twice.
    uint64_t maxc = 0;
    for (uint64_t c : col) maxc = std::max(maxc, c);
    d.col_bytes = maxc <= 0xffff ? 2 : 4;
    const bool defer_csr = dtype != kF32 && get_config().MFMA_TILES &&
                           (sp.family == KF_WARP_TOTAL || sp.family == KF_BLOCK_TOTAL) &&
                           m.is_exist(TBLOCK_META, "first_row_indices", sb);
    if (sp.family == KF_MERGE_PATH) {
        // MP_COL_PERM (decided before the CSR upload, which renumbers the columns)
        const config_t cfg = get_config();
        const uint64_t b_bytes = p.K * (uint64_t)std::max<int64_t>(1, cfg.DENSE_MATRIX_SIZE) * elem_bytes(dtype);
        d.col_perm = !sp.interleaved && p.K < (1ull << 32) &&
                     (cfg.MP_COL_PERM > 0 || (cfg.MP_COL_PERM < 0 && b_bytes >= (64ull << 20)));
        // MP_COL_PARTS (fp32 plans of the whole matrix, one column tile: N <= 32): the renumbered
        // columns dealt over P partitions, one merge-path pass each (upload_col_parts)
        const int64_t Nd = std::max<int64_t>(1, cfg.DENSE_MATRIX_SIZE);
        if (d.col_perm && dtype == 0 && sb == 0 && !pidx && cfg.MP_COL_PARTS > 1 && Nd <= 32 && p.K >= 64 * (uint64_t)cfg.MP_COL_PARTS)
            d.mp_parts = (uint32_t)std::min<int64_t>(cfg.MP_COL_PARTS, 8);
    }
    if (!defer_csr) upload_csr(p, a);
    GS_CHECK(!d.col_perm || (a.cperm && a.bperm), "merge-path column permutation: arrays not uploaded");
    upload_ctx u{p, d, a, m, sp, sb, dtype, rows, col, *vals, mc, row_num_of_sub_matrix(m, sb), out_lo, out_hi};
    switch (sp.family) {
        case KF_THREAD_TOTAL: upload_thread_total(u); break;
        case KF_WARP_TOTAL: upload_warp_total(u); break;
        case KF_BLOCK_TOTAL: upload_block_total(u); break;
        case KF_BITMAP_SEGMENT: upload_bitmap_segment(u); break;
        case KF_ROW_CHUNKS: upload_row_chunks(u); break;
        case KF_MERGE_PATH: upload_merge_path(u); break;
        default: throw gs_error("no gfx950 kernel family for this plan");
    }
    if (defer_csr && !d.mfma) upload_csr(p, a);
    // row-padded plans (modify_*_by_row_pad_in_sub_matrix): the padding rows lie past the
    // output, so every launch writes a scratch output of all the plan's rows and launch_spmm
    // copies its first M rows to C
    const uint64_t prows = u.row_num;
    if (sb == 0 && !pidx && prows > p.M) {
        d.pad_rows = prows;
        d.pad_N = (uint32_t)std::max<int64_t>(1, get_config().DENSE_MATRIX_SIZE);
        a.pad_out = dev_copy(d, std::vector<uint32_t>((prows * d.pad_N * elem_bytes(dtype) + 3) / 4, 0u));
    }
    d.replicas.push_back(a);
    p.uploaded = true;
}


// The deferred CSR of a matrix-core plan, uploaded the first time the plan runs at a dense
// width other than the one its tiles were built for.  Synchronous (hipMalloc + hipMemcpy),
// so refused inside stream capture (launch_body); the caller's current device is restored.
void ensure_csr(plan_state &p) {
    bool need = false;
    for (device_arrays &a : p.dev.replicas) need |= !a.col;
    if (!need) return;
    // (the CSR would be built from the values of before the update: a stale launch through the gather fallback)
    GS_CHECK(!p.host_values_stale, "this launch needs the plan's CSR, which is built from its host values, and those are stale -- "
                                   "gs_plan_set_values changed the values on the device only; pass the values as host_values "
                                   "to gs_plan_set_values (Plan.set_values(..., host=True)) first");
    int prev = 0;
    HIP_OK(hipGetDevice(&prev));
    for (device_arrays &a : p.dev.replicas)
        if (!a.col) upload_csr(p, a);
    HIP_OK(hipSetDevice(prev));
}

void add_replica(plan_state &p) {
    GS_CHECK(p.uploaded, "upload the plan before adding replicas");
    HIP_OK(hipSetDevice(p.dev.device));
    const device_arrays &s = p.dev.replicas[0];
    device_arrays r = s;
    // every allocation of replica 0 is duplicated (same sizes)
    size_t n0 = p.dev.allocations.size();
    std::vector<void *> base(p.dev.allocations.begin(), p.dev.allocations.begin() + n0);
    auto dup = [&](void *src) -> void * {
        if (!src) return nullptr;
        size_t bytes = 0;
        HIP_OK(hipMemPtrGetInfo(src, &bytes));
        void *dst = nullptr;
        HIP_OK(hipMalloc(&dst, bytes));
        HIP_OK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToDevice));
        p.dev.allocations.push_back(dst);
        return dst;
    };
    r.col = s.pp.empty() ? dup(s.col) : nullptr;  // MP_COL_PARTS: stand-ins for part 0 (below)
    r.val = s.pp.empty() ? dup(s.val) : nullptr;
    r.a0 = (uint32_t *)dup(s.a0);
    r.a1 = (uint32_t *)dup(s.a1);
    r.a2 = (uint32_t *)dup(s.a2);
    r.a3 = (uint32_t *)dup(s.a3);
    r.a4 = (uint32_t *)dup(s.a4);
    r.m0 = (uint64_t *)dup(s.m0);
    r.tcol = dup(s.tcol);
    r.tval = dup(s.tval);
    r.tw = dup(s.tw);
    r.wscale = (float *)dup(s.wscale);
    r.t0 = (uint32_t *)dup(s.t0);
    r.t1 = (uint32_t *)dup(s.t1);
    r.t2 = (uint32_t *)dup(s.t2);
    r.t3 = (uint32_t *)dup(s.t3);
    r.t4 = (uint32_t *)dup(s.t4);
    r.ws = (float *)dup(s.ws);
    r.ws2 = (float *)dup(s.ws2);
    r.cperm = (uint32_t *)dup(s.cperm);
    r.bperm = dup(s.bperm);
    r.pad_out = dup(s.pad_out);
    for (size_t i = 0; i < s.pp.size(); i++) r.pp[i] = dup(s.pp[i]);
    if (!s.pp.empty()) {  // the whole-matrix stand-ins point at part 0 (upload_col_parts)
        r.col = r.pp[MP_PART_COL];
        r.val = r.pp[MP_PART_VAL];
    }
    p.dev.replicas.push_back(r);
}

void memset_rows(void *C, uint64_t lo, uint64_t hi, uint32_t N, size_t e, hipStream_t stream) {
    HIP_OK(hipMemsetAsync((char *)C + lo * N * e, 0, (hi - lo) * N * e, stream));
}

void combine_parts(const void *const *parts, const uint32_t *rows, uint32_t n, void *C, uint64_t row0, uint64_t P,
                   uint32_t N, int dtype, hipStream_t stream) {
    GS_CHECK(P * N < (1ull << 40) && n > 0, "combine_parts: bad sizes");
    const uint64_t total = P * N;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
    if (blocks == 0) return;
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(gsk::k_combine_parts<T>, dim3(blocks), dim3(256), 0, stream, (const T *const *)parts, rows, n,
                           (T *)C + row0 * N, total, N);
    });
    HIP_OK(hipGetLastError());
}

void free_device(plan_state &p) {
    if (!p.dev.allocations.empty()) (void)hipSetDevice(p.dev.device);
    for (void *x : p.dev.allocations) (void)hipFree(x);
    p.dev.allocations.clear();
    p.dev.replicas.clear();
    p.uploaded = false;
}

bool epilogue_fuses(const plan_state &p, uint32_t N) {
    const device_plan &d = p.dev;
    return p.uploaded && d.mfma && d.ks && !d.nm && N == d.lds_N && !d.pad_rows && !d.ks_persist &&
           get_config().EPILOGUE_FUSE != 0;
}

void launch_epilogue(void *C, uint64_t rows, uint32_t N, int dtype, const gsk::epilogue &epi, hipStream_t stream) {
    const uint64_t total = rows * N;
    GS_CHECK(total < (1ull << 40), "launch_epilogue: bad sizes");
    if (total == 0 || gsk::epilogue_is_identity(epi)) return;
    // 16-byte accesses when every row is a whole number of them and both pointers are aligned
    const size_t e = elem_bytes(dtype);
    const uint32_t vec = ((size_t)N * e) % 16 == 0 && (uintptr_t)C % 16 == 0 && (uintptr_t)epi.residual % 16 == 0;
    const uint64_t items = vec ? total / (16 / e) : total;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((items + 255) / 256, 4096);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(gsk::k_epilogue<T>, dim3(blocks), dim3(256), 0, stream, (T *)C, epi, total, N, vec);
    });
    HIP_OK(hipGetLastError());
}

void launch_tm_in(const void *X, void *B, uint64_t K, uint32_t N, int dtype, hipStream_t stream) {
    GS_CHECK(K >= 1 && N >= 1 && K < (1ull << 32) && (N + 31) / 32 <= 65535u, "launch_tm_in: bad sizes");
    const dim3 grid((uint32_t)((K + 31) / 32), (N + 31) / 32);
    if (dtype == kF32)
        hipLaunchKernelGGL(gsk::k_tm_in<float>, grid, dim3(256), 0, stream, (const float *)X, (float *)B, (uint32_t)K, N);
    else  // (the 16-bit types move as words)
        hipLaunchKernelGGL(gsk::k_tm_in<uint16_t>, grid, dim3(256), 0, stream, (const uint16_t *)X, (uint16_t *)B, (uint32_t)K, N);
    HIP_OK(hipGetLastError());
}

void launch_tm_out(const void *C, void *Y, uint64_t M, uint32_t N, int dtype, const gsk::epilogue &epi, hipStream_t stream) {
    GS_CHECK(M >= 1 && N >= 1 && M < (1ull << 32) && (N + 31) / 32 <= 65535u, "launch_tm_out: bad sizes");
    const dim3 grid((uint32_t)((M + 31) / 32), (N + 31) / 32);
    by_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL(gsk::k_tm_out<T>, grid, dim3(256), 0, stream, (const T *)C, (T *)Y, epi, (uint32_t)M, N);
    });
    HIP_OK(hipGetLastError());
}

static void launch_body(plan_state &p, int replica, const void *B, void *C, uint32_t N, hipStream_t stream,
                        const gsk::epilogue &epi) {
    // (the upload builds no other layout for a bf16 plan: choose_matrix_core_layout, LDS_STAGE_B)
    GS_CHECK(p.dev.dtype != kBF16 || (!p.dev.nm && !p.dev.lds && (!p.dev.mfma || p.dev.ks)),
             "bf16 plans run k_mfma_ks or a gather family: the other matrix-core and LDS kernels are fp16 / fp32 kernels");
    if (p.dev.nm) {
        launch_nm(p, p.dev.replicas[replica], B, C, N, stream);
        return;
    }
    if (p.dev.mfma && N == p.dev.lds_N) {
        launch_mfma(p, p.dev.replicas[replica], B, C, N, stream, epi);
        return;
    }
    GS_CHECK(gsk::epilogue_is_identity(epi), "only k_mfma_ks applies an epilogue in the kernel (epilogue_fuses)");
    if (!p.dev.replicas[replica].col) {  // matrix-core plan at another dense width
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        HIP_OK(hipStreamIsCapturing(stream, &cs));
        GS_CHECK(cs == hipStreamCaptureStatusNone,
                 "the first gs_spmm of a matrix-core plan at N != its tile width uploads its CSR "
                 "synchronously: run it once outside stream capture");
        ensure_csr(p);
    }
    launch_gather(p, p.dev.replicas[replica], B, C, N, stream);
}

void launch_spmm(plan_state &p, int replica, const void *B, void *C, uint32_t N, hipStream_t stream,
                 const gsk::epilogue *epi) {
    GS_CHECK(p.uploaded, "plan is not on the device");
    const gsk::epilogue ep = epi ? *epi : gsk::epilogue_identity();
    GS_CHECK(gsk::epilogue_is_identity(ep) || epilogue_fuses(p, N),
             "launch_spmm: this plan and width take the epilogue as a post-pass (launch_epilogue)");
    GS_CHECK(replica >= 0 && (size_t)replica < p.dev.replicas.size(), "bad replica index");
    GS_CHECK(N >= 1, "N >= 1");
    // (the CSR fall-back at another width would need a second, differently rounded copy of A)
    GS_CHECK(p.dev.weights != kWFp8 || N == p.dev.lds_N,
             "a plan with FP8 weights runs at the width it was built for (N = " + std::to_string(p.dev.lds_N) + ") only");
    if (p.dev.pad_rows) {
        GS_CHECK(N <= p.dev.pad_N, "row-padded plan built for N=" + std::to_string(p.dev.pad_N) +
                                       ": its scratch output holds no wider B (re-run the pipeline for this N)");
        void *scr = p.dev.replicas[replica].pad_out;
        launch_body(p, replica, B, scr, N, stream, ep);
        HIP_OK(hipGetLastError());
        HIP_OK(hipMemcpyAsync(C, scr, (size_t)p.M * N * elem_bytes(p.dev.dtype), hipMemcpyDeviceToDevice, stream));
        return;
    }
    launch_body(p, replica, B, C, N, stream, ep);
}

}  // namespace gs
