// gs_plan.hpp -- internal state behind the C ABI handle gs_plan_t.
#pragma once

#include "operator.hpp"
#include "device_layout.hpp"
#include "../hip_code/idx_formula.hpp"
#include "../hip_code/kernel_consts.hpp"

#include <hip/hip_runtime.h>

namespace gs {

// Device copies of the arrays one kernel family consumes, in the layout the
// gfx950 kernels want (narrowest index types, A streams padded so aligned
// over-reads stay in bounds).  One replica = one independent copy of A
// (bench.py rotates replicas past the 256 MB Infinity Cache).
struct device_arrays {
    void *col = nullptr, *val = nullptr;
    void *pad_out = nullptr;  // row-padded plans: scratch output of all the plan's rows
    void *tcol = nullptr, *tval = nullptr;  // LDS tile layout (k_lds_rows)
    void *tw = nullptr;  // k_mfma_ks with window positions (KS_WPOS): one window byte per group
    float *wscale = nullptr;  // k_mfma_ks with FP8 weights: one fp32 scale per row of A (per replica, as tval is)
    uint32_t *t0 = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr, *t4 = nullptr;
    uint32_t *a0 = nullptr, *a1 = nullptr, *a2 = nullptr, *a3 = nullptr, *a4 = nullptr;
    uint64_t *m0 = nullptr;
    float *ws = nullptr;  // k_mfma_rows K-split slabs (per replica: a replica never runs concurrently with itself)
    float *ws2 = nullptr;  // k_merge_path: partials of the rows each wave closes first (head_rec)
    uint32_t *cperm = nullptr;  // merge path, MP_COL_PERM: original column of each renumbered column (or, with
                                // perm_scatter, the new place of each column)
    void *bperm = nullptr;      // ... B gathered into that order (K x the plan's N, per replica)
    // merge path, MP_COL_PARTS: kMpPartPtrs device arrays per column partition (mp_part_* below)
    std::vector<void *> pp;
};
// per column partition x: pp[x * kMpPartPtrs + i], i = the mp_part_* index
enum { MP_PART_COL, MP_PART_VAL, MP_PART_WZ, MP_PART_WQ, MP_PART_ENDS, MP_PART_RID, MP_PART_EMPTY, MP_PART_WS,
       MP_PART_WS2, MP_PART_T0, MP_PART_CHAIN, MP_PART_CNT, MP_PART_OUT, kMpPartPtrs };

struct device_plan {
    int device = 0;
    int dtype = 1;         // 0 fp32, 1 fp16, 2 bf16 (values, B and C; device_layout.hpp kF32 / kF16 / kBF16)
    int weights = 0;       // 0 A's values in the dtype, 1 e4m3 codes + a scale per row (kWNative / kWFp8; k_mfma_ks, fp16)
    int col_bytes = 2;     // 2 (u16) or 4 (u32)
    int scf = 4;           // sparse entries per vector load
    bool needs_memset = false;
    uint64_t n_out_rows = 0;  // one past the last row of C this plan writes
    uint64_t pad_rows = 0;    // row-padded plan (modify_*_by_row_pad_in_sub_matrix): its rows, > M
    uint32_t pad_N = 0;       // ... the dense width its scratch output holds
    uint64_t out_lo = 0;      // first row of C this plan writes (a sub-matrix's range)
    uint64_t n_units = 0;     // BMTs / BMWs / BMTBs the grid walks
    uint64_t n_rows_aux = 0;  // rows covered (thread_total: rows incl. trailing empty)
    uint64_t row_base = 0;
    uint32_t ks_ctw = 0;      // k_mfma_ks: 16-column tiles per workgroup (ks_tiles::CT)
    bool ks_ap = true;        // k_mfma_ks: partial tiles beside the stages (ks_tiles::AP)
    bool ks_p8 = false;       // k_mfma_ks: 8-bit entry positions (ks_tiles::P8, KS_POS8)
    bool ks_wp = false;       // k_mfma_ks: one-byte window positions (ks_tiles::WP, KS_WPOS)
    uint32_t ks_gh = 0;       // k_mfma_ks: groups per head step (ks_tiles::GH; 0: every step by record)
    uint32_t ks_nt = 0;       // k_mfma_ks: non-temporal loads of A's groups (NTL bit 0; ks_tiles::NT, KS_NT)
    uint32_t ks_persist = 0;  // k_mfma_ks: persistent grid of this many workgroups pulling units (KS_PERSIST, experiments)
    bool nm_nt = false;       // k_nm_mfma: non-temporal panel loads (NM_NT)
    uint32_t nm_tiles = 8;    // k_nm_mfma: 16-row tiles per workgroup (mc_layout::nm_T)
    bool lds_dma = false;     // k_lds_rows_dma: fp32 N = 32 chunks by LDS-DMA into two buffers (LDS_DMA)
    // merge path, MP_COL_PARTS: the columns (renumbered by degree, MP_COL_PERM) dealt round-robin
    // over mp_parts partitions; one k_merge_path per partition, each over its own CSR and wave
    // ranges, so every pass gathers B rows of one partition only (its hubs fit each XCD's L2)
    uint32_t mp_parts = 0;
    std::vector<uint32_t> mp_part_W, mp_part_rows, mp_part_fin;
    uint64_t err_at = 0;      // K-split combine: index of the device error word in t2 (0: none)
    uint64_t nnz_stored = 0;  // padded nnz on device
    size_t bytes_A = 0;       // device bytes of A per replica (metadata + cols + vals)
    // LDS-stationary B (k_lds_rows): chunk geometry fixed for dense width lds_N
    bool lds = false;
    bool nm_ks = false;  // k_nm_mfma_ks (ksplit K ranges of ncs chunks; ws slabs + t2 counters when ksplit > 1)
    bool nm = false;    // k_nm_mfma: 2:4 panels of a col-direction plan (A blocks in tcol; k-steps in KC)
    bool nm4 = false;   // ... on k_nm_mfma4 (256-row workgroups, ksplit K ranges of ncs chunks)
    bool mfma = false;  // k_mfma_rows (uses KC, nc, lds_bytes; log2 KC in RSB; RT in maxr; RMAX in rpw_max)
    bool ks = false;    // k_mfma_ks: K split over ksplit workgroups per row block, B slice in LDS
                        // (t0 BMTB rows, tcol/tval groups; ks_ns k-steps per range,
                        // RT in maxr, MAXG in seg_cap, ws slabs + t2 arrivals when ksplit > 1)
    uint32_t ks_ns = 0, ks_gcap = 0;
    uint64_t ks_val_slots = 0;  // k_mfma_ks: 16-bit words of tval (ks_tiles::val: 8 per entry group, the spare group too)
    uint64_t ks_hash = 0;       // ... and ks_layout_hash of the uploaded layout (gs_plan_set_values' map must be its map)
    bool bmkb = false;  // ... k_mfma_kb: k_mfma_ks pipeline on the bitmap layout (8 waves)
    bool bm2 = false;   // ... k_mfma_bm2: one wave per row tile (W = RT), B slice of ks_ns k-steps in LDS
    bool bm = false;    // k_mfma_bm: bitmap records (tcol), step bases (t1), values (tval), t0 BMTB rows;
                        // ksplit K ranges of ks_ns k-steps, RT in maxr, W in waves

    bool mp_rows = false;   // merge-path plans: k_merge_rows (fixed at upload, MP_ROWS), else k_merge_path
    uint32_t mp_solo = 16;
    bool col_perm = false;  // merge path: columns renumbered by degree (cperm / bperm)
    bool perm_scatter = false;  // ... cperm holds each column's new place (k_permute_rows scatters)  // k_merge_rows: slot-alone row length (MP_SOLO)
    // k_mfma_rows variant fixed at upload (device_layout.cc): GLDS / B ring depth / compute
    // waves / entry groups per thread -- the launch uses these, not the config of the moment
    int mfma_glds = 2, mfma_nbg = 3, mfma_wct = 6, mfma_maxa = 1;
    bool mfma_flags = false;  // k_mfma_rows: LDS counter hand-offs instead of per-chunk barriers  // k_mfma_ks: k-steps per K range, entry groups per step
    std::string kernel;  // the device kernel gs_spmm launches at the plan's N (empty: the family's)
    uint32_t ksplit = 1, ncs = 0;  // k_mfma_rows workgroups per row block, chunks per workgroup
    uint32_t ws_n = 0;             // bitmap family: dense width of the fp32 workspace
    uint64_t n_fin = 0;            // bitmap family: rows k_finalize_rows writes
    uint32_t span = 0;             // k_row_chunks: BMTs per wave
    uint32_t bmw_rows_max = 0;     // k_warp_rows: most rows in one BMW
    double mean_row_nnz = 0.0;     // ... and the mean row length (slots per row)
    uint32_t ilv = 0;              // k_row_chunks: BMT size of an interleaved layout (0: contiguous)
    uint32_t lds_N = 0, KC = 0, nc = 0, RSB = 0, rpw_max = 0, seg_cap = 0, waves = 0, maxr = 0;
    size_t lds_bytes = 0, bytes_tile = 0;
    // model-driven index compression on the device (MODEL_DRIVEN_COMPRESS):
    // the formulas the gather families evaluate for a0 / a1 (kind IDX_ARRAY: read the array)
    gsk::idx_formula f0, f1;
    int index_formulas = 0;         // arrays replaced by a formula (or narrowed to residuals)
    uint64_t index_bytes_saved = 0;  // u32 index bytes per replica not uploaded because of them
    std::vector<device_arrays> replicas;
    std::vector<void *> allocations;  // everything to hipFree
};

struct plan_state {
    std::shared_ptr<meta_data_set> meta;
    std::shared_ptr<code_generator> cg;
    std::shared_ptr<operator_executer> exec;
    std::string pipeline;
    uint64_t M = 0, K = 0, nnz = 0;
    device_plan dev;
    bool uploaded = false;
    // gs_plan_set_values changed the values on the device only: the host copies (nz_vals, the pattern's val) are
    // the old ones until a host refresh or an upload; every reader of them refuses meanwhile (ensure_csr,
    // gs_plan_save, gs_plan_fp8_layout, gs_plan_pattern with values)
    bool host_values_stale = false;
    // a sub-matrix of row_nz_matrix_div_operator: its row indices refer to the divided
    // sub-matrix (rows [parent_row_base, parent_row_base + parent_rows) of C); -1 otherwise
    int64_t parent_row_base = -1;
    uint64_t parent_rows = 0;
};

// a kernel of a plan file: sub-matrix id, kernel spec, parent-indexed row range
struct loaded_kernel {
    int sub = 0;
    kernel_spec spec;
    int64_t parent_row_base = -1;
    uint64_t parent_rows = 0;
};

// plan_io.cc: binary plan files
// one file holds every kernel of a plan (one per sub-matrix of a row division); load
// returns the metadata set and the (sub-matrix id, kernel spec) list
void save_plan(const std::vector<const plan_state *> &kernels, const std::string &path);
std::shared_ptr<meta_data_set> load_plan(const std::string &path, std::vector<loaded_kernel> &kernels,
                                         std::string &pipeline);

// device_plan.hip
// weights (kWNative / kWFp8), row_scale (kWFp8: null or M scales): gs_plan_upload_ex's.  An FP8 upload is
// refused, before anything is allocated, unless the plan is the undivided matrix without padded rows,
// the dtype fp16 and the layout one check_fp8_layout admits
void upload_plan(plan_state &p, int dtype, int device, int weights = kWNative, const float *row_scale = nullptr);
void add_replica(plan_state &p);
void free_device(plan_state &p);
// zero rows [lo, hi) of a row-major C of width N, element size e (sub-matrix executor)
void memset_rows(void *C, uint64_t lo, uint64_t hi, uint32_t N, size_t e, hipStream_t stream);
// C[row0 + r] = sum of parts[q][r] over the q with r < rows[q], r < P (parent-indexed
// sub-matrices' scratch outputs; parts / rows are device arrays of n entries)
void combine_parts(const void *const *parts, const uint32_t *rows, uint32_t n, void *C, uint64_t row0, uint64_t P,
                   uint32_t N, int dtype, hipStream_t stream);
// epi (null: none): the launch's epilogue, applied inside k_mfma_ks -- only for a plan and width
// that epilogue_fuses admits; every other launch takes the post-pass launch_epilogue after it
void launch_spmm(plan_state &p, int replica, const void *B, void *C, uint32_t N, hipStream_t stream,
                 const gsk::epilogue *epi = nullptr);
// the plan runs k_mfma_ks at its tile width N through launch_mfma, writing C itself (no pad_rows
// scratch, static grid), and EPILOGUE_FUSE is on: launch_spmm applies an epilogue in the kernel
bool epilogue_fuses(const plan_state &p, uint32_t N);
// the post-pass: k_epilogue in place on C (rows x N of dtype) -- allocates nothing
void launch_epilogue(void *C, uint64_t rows, uint32_t N, int dtype, const gsk::epilogue &epi, hipStream_t stream);
// uploads the CSR arrays a matrix-core plan deferred (every replica), for a launch at another dense width
void ensure_csr(plan_state &p);
void debug_mp_timeline(const plan_state &p, const void *B, void *C, uint32_t N, hipStream_t s, uint64_t *host,
                       size_t n_host);
void debug_mfma_timeline(const plan_state &p, const void *B, void *C, uint32_t N, hipStream_t s, uint64_t *host,
                         size_t n_host);
// mfma_launch.hip: k_mfma_rows / k_nm_mfma (and k_mfma_ks through launch_ks) at the plan's N
// (epi: k_mfma_ks plans only, epilogue_fuses)
void launch_mfma(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
                 const gsk::epilogue &epi = gsk::epilogue_identity());
void launch_nm(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s);
// gather_launch.hip: the CUDA-core gather families and k_lds_rows
void launch_gather(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s);
// ks_launch.hip: k_mfma_ks (K-split, wave-autonomous matrix-core row blocks)
void launch_ks(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
               const gsk::epilogue &epi = gsk::epilogue_identity());
// the FP8-weight forms behind launch_ks and launch_linear_fused, for plans uploaded with kWFp8 (same arguments,
// plus the replica's scales): k_mfma_ks_w8 (ks_w8_launch.hip) and k_mfma_ks_tm with VB = 8 (ks_tm_launch.hip's
// object ks_tm_w8_launch.o)
void launch_ks_w8(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s,
                  const gsk::epilogue &epi);
void launch_ks_tm_w8(const plan_state &p, const device_arrays &a, const void *X, void *Y, uint32_t N, hipStream_t s,
                     const gsk::epilogue &epi, float *slabs, uint32_t *arrivals);
// ks_tm_launch.hip: k_mfma_ks_tm, a k_mfma_ks plan on token-major activations (gs_linear: Y = X * A^T,
// X: n_tokens x K, Y: n_tokens x M).  linear_fuses: the plan and its upload layout are ones the kernel
// is built for (a plan of 17 .. 32 tokens -- 32-token tiles -- 8 waves, 16-bit positions, K % 8 == 0,
// LINEAR_FUSE on), at any token count; the launch needs X 16-byte aligned as well.
// launch_linear_fused: ONE launch of ceil(n_tokens / 32) token tiles (at most kKsTmMaxTiles).  With
// K ranges and more than one tile the caller passes K-split state laid out for that tile count --
// slabs: ks_tm_tile_bytes' slab part per tile; arrivals: nb counters per tile, the device error word
// right behind them -- whose counters and slab tags are zero or left by a launch of the same tile
// count; null: the replica's own (one tile, shared with k_mfma_ks).  Allocates nothing
bool linear_fuses(const plan_state &p, uint32_t n_tokens);
void launch_linear_fused(const plan_state &p, int replica, const void *X, void *Y, uint32_t n_tokens, hipStream_t s,
                         const gsk::epilogue &epi, float *slabs = nullptr, uint32_t *arrivals = nullptr);
// device_plan.hip: the two ends of gs_linear's three-launch path (parts.hpp k_tm_in / k_tm_out)
// B (K x N) = X^T (X: N x K)
void launch_tm_in(const void *X, void *B, uint64_t K, uint32_t N, int dtype, hipStream_t stream);
// Y (N x M) = epilogue(C)^T (C: M x N; the residual N x M, as Y)
void launch_tm_out(const void *C, void *Y, uint64_t M, uint32_t N, int dtype, const gsk::epilogue &epi, hipStream_t stream);
// grouped k_mfma_ks launches (gs_spmm_batch): one grid over up to 32 entries of one
// instantiation (equal nonzero ks_group_key); every entry a distinct (plan, replica)
struct ks_group_item {
    const plan_state *p;
    int replica;
    const void *B;
    void *C;
    gsk::epilogue epi = gsk::epilogue_identity();  // applied in the kernel (store_item)
};
uint32_t ks_group_key(const plan_state &p, uint32_t N);  // 0: not groupable
void launch_ks_group(const std::vector<ks_group_item> &it, uint32_t N, hipStream_t s);
// grouped k_mfma_ks_tm launches (gs_linear_batch; ks_tm_group_launch.hip): one grid over up to kKsTmGroupMax
// entries of one instantiation (equal nonzero ks_tm_group_key), every entry a distinct (plan, replica) with its
// own token count.  slabs / arrivals: launch_linear_fused's -- K-split state laid out for the entry's
// ceil(n_tokens / 32) tiles where the plan has K ranges and the entry more than one tile, null otherwise
struct ks_tm_group_item {
    const plan_state *p;
    int replica;
    const void *X;
    void *Y;
    uint32_t n_tokens;
    gsk::epilogue epi = gsk::epilogue_identity();  // applied in the kernel (store_item)
    float *slabs = nullptr;
    uint32_t *arrivals = nullptr;
};
// 0: not groupable.  Nonzero (dtype, NT, RT, MAXG) where gs_linear would run this call as a single k_mfma_ks_tm
// launch of 16-bit values: linear_fuses, X 16-byte aligned, native weights, one launch under LINEAR_WS_KB
uint32_t ks_tm_group_key(const plan_state &p, uint32_t n_tokens, const void *X);
void launch_ks_tm_group(const std::vector<ks_tm_group_item> &it, hipStream_t s);
// sddmm_launch.hip: k_sddmm_tm (gs_sddmm).  out[e] = sum over t < n of G[t][row_e] * X[t][col_e] for the
// entries of the CSR pattern rp (M + 1 u32) / cols (col_bytes 2: u16, 4: u32) in canonical order
// (sddmm_layout.hpp); G: n x M, X: n x K of dtype (kF16 / kBF16), out: fp32.  Allocates nothing
void launch_sddmm(int dtype, int col_bytes, const void *G, const void *X, const uint32_t *rp, const void *cols, float *out,
                  uint32_t n, uint64_t M, uint64_t K, hipStream_t s);
// set_values_launch.hip: k_set_values (gs_plan_set_values).  tval: n_groups x 8 words of dtype (kF16 / kBF16) rewritten
// from values[src[slot]] (src: n_groups x 8 u32 on the device, kNoValue: the slot becomes 0).  Allocates nothing
void launch_set_values(int dtype, void *tval, const uint32_t *src, const float *values, uint64_t n_groups, hipStream_t s);
void launch_bm(const plan_state &p, const device_arrays &a, const void *B, void *C, uint32_t N, hipStream_t s);
void debug_bm_timeline(const plan_state &p, const void *B, void *C, uint32_t N, hipStream_t s, uint64_t *host,
                       size_t n_host);
void debug_ks_timeline(const plan_state &p, const void *B, void *C, uint32_t N, hipStream_t s, uint64_t *host,
                       size_t n_host);

}  // namespace gs
