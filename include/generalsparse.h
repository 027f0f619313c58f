/*
 * generalsparse.h -- C ABI of the MI355X-native GeneralSparse SpMM engine.
 *
 * This is the drop-in boundary for the reference's SpMM path.
 * Plain pointers and sizes only; every call returns 0 or a negative error
 * code (gs_last_error() has the message); nothing aborts across the ABI
 * (the reference asserts everywhere).  Reentrant per plan, one HIP stream per
 * call, no internal host threads.
 *
 * Reference interfaces each entry point replaces:
 *   gs_plan_create_from_mtx   create_init_metadata_set_from_file   metadata_set.cc:612-707
 *                             (+ get_matrix_index_and_val_from_file  struct.cc:49-261)
 *   gs_plan_create_from_coo   same, from in-memory COO (no text round trip)
 *   gs_plan_add_operator      operator_executer::add_and_run        operator_executer.cc:19-26
 *                             with the operator classes of           operator.hpp:64-1324
 *   gs_plan_run_pipeline      token_test.cc test_spmm_* functions    token_test.cc:1003-1582
 *   gs_set_config_int         set_config                              config.cc:17-40
 *   gs_get_config_int         get_config                              config.cc:42-70
 *   gs_plan_compile           code_generator::compile                code_generator.hpp:265-269
 *   gs_plan_generate_program  code_generator::generate_final_program code_generator.hpp:271-280
 *   gs_plan_upload / gs_spmm  the generated program's device copies + kernel launch
 *                             (code_generator.cc:285-600, executor.cc:6-104)
 *   gs_plan_array_*           meta_data_set::get_element / output_format_to_dir (plan arrays by key)
 *   gs_plan_from_mtx          the one-call form proposed in SURVEY.md §8b
 */
#ifndef GENERALSPARSE_H
#define GENERALSPARSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gs_plan gs_plan_t;
typedef void *gs_stream_t; /* hipStream_t; NULL = default stream */

enum { GS_OK = 0, GS_ERR = -1, GS_ERR_ARG = -2, GS_ERR_HIP = -3,
       GS_ERR_DEVICE = -4 /* a kernel reported a fault in its device error word (gs_plan_device_status) */ };
/* value types of a plan on the device (A's values, B and C alike).  GS_BF16 runs the K-split
 * matrix-core kernel (k_mfma_ks) and every gather family; plans that would take another
 * matrix-core or LDS kernel at fp16 run their gather family at bf16. */
enum { GS_F32 = 0, GS_F16 = 1, GS_BF16 = 2 };

typedef struct {
    const char *pipeline;   /* token_test pipeline name, see gs_plan_run_pipeline */
    int dtype;              /* GS_F32 / GS_F16 / GS_BF16 (A values, B and C) */
    int dense_n;            /* DENSE_MATRIX_SIZE used to size the plan (token_test argv[2]) */
    int p0, p1;             /* pipeline parameters (sparse_coarsen_factor / rows per BMTB / ...) */
    int ones_values;        /* 1: reference reader semantics, every value := 1 (struct.cc:186-200) */
    int device;             /* HIP device ordinal */
} gs_opts;

typedef struct {
    uint64_t rows, cols, nnz;     /* original matrix */
    uint64_t nnz_stored;          /* after padding */
    uint64_t n_units;             /* BMTs / BMWs / BMTBs the kernel walks */
    uint64_t device_bytes_A;      /* HBM bytes of A (metadata + cols + vals) per replica */
    int family;                   /* 1 thread_total, 2 warp_rows, 3 block_rows, 4 bitmap_segment */
    int col_bytes, dtype /* GS_F32 / GS_F16 / GS_BF16, as uploaded */, replicas, needs_memset;
    char kernel_name[64];
    /* row-block kernels built at upload for dense width lds_n: 1 = LDS-stationary B
     * (k_lds_rows, config LDS_STAGE_B), 2 = matrix cores (k_mfma_rows, MFMA_TILES),
     * 3 = 2:4 panels of a col-direction plan on the sparse matrix cores (k_nm_mfma, NM_MFMA) */
    int lds_stage;
    uint32_t lds_n, lds_kc, lds_chunks, lds_waves;
    uint64_t lds_bytes, tile_bytes;
    uint32_t ksplit;              /* k_mfma_rows workgroups per row block (K ranges, fp32 slab combine) */
    int n_kernels;                /* kernels gs_spmm runs: 1, or one per sub-matrix of a row division */
    char device_kernel[32];       /* the device kernel gs_spmm launches at the plan's N (first sub-matrix) */
    int index_formulas;           /* index arrays the kernel evaluates as formulas (MODEL_DRIVEN_COMPRESS) */
    uint64_t index_bytes_saved;   /* u32 index bytes per replica those formulas keep out of HBM */
    uint32_t ks_nt;               /* k_mfma_ks: A's groups by non-temporal loads (KS_NT) */
    uint32_t ks_head_groups;      /* k_mfma_ks: groups per head step (KS_HEAD; 0: every step by record) */
    uint32_t nm_tiles;            /* k_nm_mfma: 16-row tiles per workgroup (NM_TILES / the upload's rule) */
    uint32_t ks_wpos;             /* k_mfma_ks: one-byte window positions (KS_WPOS; 0: the u16 layout) */
    uint32_t weights;             /* GS_W_NATIVE / GS_W_FP8_E4M3, as uploaded (tile_bytes / device_bytes_A: the true bytes) */
    uint32_t host_values_stale;   /* 1 after a device-only gs_plan_set_values, 0 after a host refresh or an upload */
    uint64_t value_map_bytes;     /* device bytes of gs_plan_set_values' map (once per plan); 0 until prepared */
} gs_plan_info;

const char *gs_last_error(void);
const char *gs_version(void);

void gs_opts_default(gs_opts *o);

/* Both readers refuse (GS_ERR -1, gs_last_error names the cause) a matrix without entries
 * (struct.cc:258), rows out of order (struct.cc:120-131), a .mtx index that is not a decimal
 * >= 1, and any index past 2^32 - 2 (dims at most 2^32 - 1); the dims grow to the largest index + 1.  row / col / val hold
 * nnz entries each (val may be NULL: every value 1). */
int gs_plan_create_from_mtx(const char *path, int ones_values, gs_plan_t **out);
int gs_plan_create_from_coo(uint64_t n_rows, uint64_t n_cols, uint64_t nnz, const uint64_t *row,
                            const uint64_t *col, const float *val, gs_plan_t **out);
int gs_set_config_int(const char *key, long long value);
/* the current value of an integer / bool key (the reference reads get_config per use,
 * config.cc:42-70) */
int gs_get_config_int(const char *key, long long *value);

/* operator surface: name = reference class name; args in constructor order
 * without the code_generator / operator_context arguments */
int gs_plan_add_operator(gs_plan_t *p, const char *op_name, const long long *args, int nargs);
/* canned pipelines: thread_total(p0=sparse_cf,p1=cf), warp_total(cf=p1), block_total(p0=rows per BMTB, cf=p1),
 * thread_bit_map(p0=sparse_cf,p1=cf), warp_segment(p0=sparse_cf,p1=cf),
 * tblock_warp_total(p0=rows per BMTB, p1=rows per BMW), balanced_warp_total(p0=nnz per BMW) */
int gs_plan_run_pipeline(gs_plan_t *p, const char *name, int dense_n, int p0, int p1);
/* sub-matrices (§8f rank 3): after fixed_interval_row_matrix_div_operator
 * (operator/fixed_interval_row_matrix_div_operator.cc:85-150; new sub-matrix ids = max + 1,
 * one per non-empty row interval) each sub-matrix gets its own operators / pipeline --
 * the reference's code_generator(meta, sub) per sub-matrix (code_generator.cc:14-40).
 * Compile / upload / gs_spmm then cover every live sub-matrix, one kernel each, in id
 * order on the caller's stream (rows of empty intervals are zeroed first). */
int gs_plan_add_operator_sub(gs_plan_t *p, int sub, const char *op_name, const long long *args, int nargs);
int gs_plan_run_pipeline_sub(gs_plan_t *p, int sub, const char *name, int dense_n, int p0, int p1);
/* ids of the sub-matrices holding nonzeros (ascending); returns the count (< 0: error) */
int gs_plan_sub_matrices(gs_plan_t *p, int *ids, int cap);
int gs_plan_compile(gs_plan_t *p);
int gs_plan_generate_program(gs_plan_t *p, const char *root_dir, int repeat, char *dir_out, int dir_out_len);

/* dtype: GS_F32, GS_F16 or GS_BF16 (anything else: GS_ERR).  A's fp32 values are converted
 * with gs_convert_values; B and C of every later gs_spmm hold the same type. */
int gs_plan_upload(gs_plan_t *p, int dtype, int device);
/* the conversion gs_plan_upload applies to A's values: n elements of the dtype's storage type
 * into `out` (float for GS_F32, 16-bit words for GS_F16 / GS_BF16), round to nearest even;
 * NaN stays a quiet NaN, +-Inf stay, values past the largest finite value round to +-Inf.
 * Host only (no device is touched). */
int gs_convert_values(const float *in, uint64_t n, int dtype, void *out);
/* How A's values are held on the device.  GS_W_NATIVE: in the plan's dtype (gs_plan_upload).
 * GS_W_FP8_E4M3: one OCP e4m3fn code per stored value and one fp32 scale per row of A, value =
 * decode(code) * scale[row] -- 3 instead of 4 bytes per stored entry of a k_mfma_ks plan.  B, C, bias,
 * residual and the accumulation stay GS_F16's: the kernel decodes the codes to fp16 (exact: every finite
 * e4m3 value is an fp16 value), runs the MFMAs of the fp16 plan in their order and multiplies the fp32
 * sum of a row by its scale before the epilogue and the one rounding.  With power-of-two scales (the
 * default rule) the result is bit for bit that of a GS_W_NATIVE fp16 plan of the dequantised values.
 * row_scale: NULL (scale[r] = 2^e, the smallest e with max|A[r, :]| / 2^e <= 448; 1 for a row without
 * values) or one finite scale > 0 per row of A.
 * Accepted only for an undivided plan without padded rows that compiles to k_mfma_ks in its release layout
 * (built for 17 .. 32 dense columns, 8 waves, 16-bit positions, the static grid), dtype GS_F16, K a multiple
 * of 8; every other plan, a non-finite value of A or a bad scale is refused (GS_ERR, the condition in
 * gs_last_error) before anything is allocated: the plan is then not on the device.  Such a plan runs
 * gs_spmm / gs_spmm_ex at the width it was built for only, gs_linear at any token count (the three-launch
 * path at that width only), and a batch runs it as single launches. */
enum { GS_W_NATIVE = 0, GS_W_FP8_E4M3 = 1 };
int gs_plan_upload_ex(gs_plan_t *p, int dtype, int weights, const float *row_scale, int device);
/* The quantiser of GS_W_FP8_E4M3, host only: codes[i] = e4m3(val[i] / scale[row[i]]), an IEEE fp32
 * division rounded to nearest even and saturated at +-448 (codes 0x7f / 0xff, NaN, are never written).
 * row[i] < n_rows is the row of val[i]; row_scale NULL: the default rule above, else n_scale == n_rows
 * scales.  scale (n_rows entries) receives the scales used.  Refused: a non-finite value, a row index
 * past n_rows, a scale that is not finite and > 0, n_scale != n_rows. */
int gs_quantize_fp8_rows(const float *val, const uint64_t *row, uint64_t n, uint64_t n_rows, const float *row_scale,
                         uint64_t n_scale, uint8_t *codes, float *scale);
/* e4m3fn codes to fp32 (exact; 0x7f / 0xff give NaN).  Host only. */
int gs_fp8_decode(const uint8_t *codes, uint64_t n, float *out);
/* The 8-bit value array (8 codes per entry group, in the order of the plan's k_mfma_ks groups) and the
 * n_rows scales exactly as gs_plan_upload_ex(GS_F16, GS_W_FP8_E4M3, row_scale) would lay them out for
 * this compiled plan under the current config, without touching a device; its refusals are the upload's.
 * *n_codes receives the array's length; codes / scale are written when cap holds it. */
int gs_plan_fp8_layout(gs_plan_t *p, const float *row_scale, uint8_t *codes, uint64_t cap, uint64_t *n_codes, float *scale);
int gs_plan_add_replica(gs_plan_t *p);
/* C = A * B.  B: K x N row-major, C: M x N row-major, device pointers of the
 * plan's dtype (float, fp16 or bf16 elements: GS_F32 / GS_F16 / GS_BF16; every kernel
 * accumulates in fp32 and rounds once, to nearest even, at the store).  Enqueued on `stream`; returns without synchronising.  The library cannot
 * see the extents behind raw pointers: the caller guarantees K x N readable and M x N
 * writable elements (the Python Plan.spmm / Rotation / Batch check their tensors). */
int gs_spmm(gs_plan_t *p, const void *B, void *C, int N, gs_stream_t stream);
int gs_spmm_replica(gs_plan_t *p, int replica, const void *B, void *C, int N, gs_stream_t stream);
/* C = epilogue(A * B): gs_spmm_replica with an element-wise epilogue.  With acc the fp32 value of
 * (A * B)[r][c], in this order: t = alpha * acc; t += bias[r] (bias: fp32 device array, one per row
 * of C); t = t < 0 ? 0 : t (GS_ACT_RELU; NaN stays NaN); t += residual[r][c] (device array of the
 * plan's dtype, M x N row-major, no overlap with C); C[r][c] = t rounded once to the plan's dtype.
 * A stage with a NULL pointer / GS_ACT_NONE is skipped (alpha = 1 is exact).  epi NULL, or alpha 1
 * with nothing else, runs exactly gs_spmm_replica's launches.
 * Plans that run k_mfma_ks at their tile width apply it in the kernel's store, on the fp32 sums
 * (gs_plan_epilogue_fused = 1); every other plan or width runs its kernels and then one in-place
 * pass over C (k_epilogue; no allocation, legal under stream capture), which at GS_F16 / GS_BF16
 * rounds twice: once by the family, once by the pass.  Config EPILOGUE_FUSE = 0 sends every plan
 * through the pass.  Refused (GS_ERR) before any launch: an unknown activation, a non-finite
 * alpha, residual == C. */
enum { GS_ACT_NONE = 0, GS_ACT_RELU = 1 };
typedef struct gs_epilogue {
    float alpha;
    int activation;         /* GS_ACT_NONE / GS_ACT_RELU */
    const float *bias;      /* M fp32 values, or NULL */
    const void *residual;   /* M x N elements of the plan's dtype, or NULL */
} gs_epilogue;
int gs_spmm_ex(gs_plan_t *p, int replica, const void *B, void *C, int N, const gs_epilogue *epi, gs_stream_t stream);
/* 1: gs_spmm_ex at dense width N applies an epilogue inside the kernel (one rounding), 0: by the
 * post-pass, < 0: error (the plan is not on the device) */
int gs_plan_epilogue_fused(gs_plan_t *p, int N);
/* Y = epilogue(X * A^T).  X: n_tokens x K, Y: n_tokens x M, row-major, the plan's dtype.
 * epi may be NULL; bias is per column of Y (row of A); residual is n_tokens x M, no overlap with Y.
 * The layout a linear layer holds its activations in: with A the (out, in) weight this is
 * F.linear(X, A, bias), the epilogue's stages in gs_spmm_ex's order on the fp32 sums.
 * A k_mfma_ks plan built for 17 .. 32 tokens (8 waves, 16-bit positions, no row padding), K % 8 == 0
 * and X 16-byte aligned runs ONE kernel, k_mfma_ks_tm, on the plan as uploaded, at ANY n_tokens >= 1:
 * ceil(n_tokens / 32) token tiles in one launch, the last one partial; X is read and Y written in
 * place, the epilogue is applied in the store (one rounding); row t of Y has the same bits whatever
 * n_tokens is and wherever token t stands (gs_plan_linear_fused = 1).  One tile -- n_tokens <= 32 --
 * allocates nothing.  More tiles on a plan with K ranges (ksplit > 1) need K-split state per tile,
 * (row blocks) x (ksplit x row tiles x 2048 + 4) bytes: one buffer per plan replica, allocated by the
 * first such call and grown for more tiles, synchronously as the scratch below (refused inside stream
 * capture the first time, legal later; freed with the plan).  Config LINEAR_WS_KB (65536) caps that
 * buffer: a call whose tiles need more runs as several launches of the kernel on the stream, in
 * token order (gs_plan_linear_launches tells them).  Every other plan and alignment runs three launches: X
 * transposed into a scratch B, the plan's gs_spmm_replica launches, and the epilogue with the
 * transpose back (at GS_F16 / GS_BF16 two roundings, as gs_spmm_ex's pass).  The scratch of (K + M) x
 * n_tokens elements belongs to the plan replica; it is allocated by the first call at a token count
 * (grown for a larger one, freed with the plan), synchronously: inside stream capture that first call
 * is refused, later ones are legal.  Config LINEAR_FUSE = 0 sends every plan through the three
 * launches; EPILOGUE_FUSE is not consulted.  Refused (GS_ERR) before any launch: a plan that is not
 * on the device, a bad replica, n_tokens < 1, an unknown activation, a non-finite alpha, a
 * residual that overlaps Y anywhere in its n_tokens x M elements. */
int gs_linear(gs_plan_t *p, int replica, const void *X, void *Y, int n_tokens, const gs_epilogue *epi, gs_stream_t stream);
/* 1: gs_linear at n_tokens runs k_mfma_ks_tm (given an aligned X), 0: the three-launch path (also for a
 * plan that is not on the device), < 0: error */
int gs_plan_linear_fused(gs_plan_t *p, int n_tokens);
/* how gs_linear would enqueue n_tokens (given an aligned X): returns the number of k_mfma_ks_tm
 * launches and the token tiles (of 32) each carries in tiles[0 .. min(count, cap)), in token order;
 * 0: the three-launch path; < 0: a bad argument or a plan that is not on the device.  Allocates nothing. */
int gs_plan_linear_launches(gs_plan_t *p, int n_tokens, int *tiles, int cap);
/* the arithmetic behind it, host only: a plan of row_blocks row blocks of row_tiles 16-row tiles over
 * k_ranges K ranges, LINEAR_WS_KB = ws_kb.  *tile_bytes (may be NULL) gets the K-split state of one
 * token tile; the return value and tiles[] are gs_plan_linear_launches' for such a plan (k_ranges = 1
 * needs no state: only the limit of 16383 tiles per launch splits a call) */
int gs_linear_tile_split(uint64_t row_blocks, int k_ranges, int row_tiles, int n_tokens, long long ws_kb,
                         unsigned long long *tile_bytes, int *tiles, int cap);
/* n gs_linear calls as one call on one stream: entry i is gs_linear(plans[i], replicas[i], X[i], Y[i],
 * n_tokens[i], epi[i], stream) -- its own plan, operands and token count; epi may be NULL, and so may any
 * epi[i]; several entries may read one X.  Consecutive entries that gs_linear would each run as ONE
 * k_mfma_ks_tm launch of the same instantiation run as ONE launch of k_mfma_ks_tm_group -- one grid, each entry
 * on its own share of it, with its own token tiles -- so a model's Q/K/V projections, an MLP's gate / up pair or
 * a set of experts with ragged token counts pay one launch instead of one each.  An entry's Y has the bits
 * of its own gs_linear call, grouped or not.  Entries share a launch when all of this holds for each:
 * gs_plan_linear_fused = 1, X 16-byte aligned, 16-bit weights (not GS_W_FP8_E4M3), a single launch under
 * LINEAR_WS_KB (gs_plan_linear_launches = 1), and the same dtype, KS_NT, row tiles and entry groups per k-step
 * as its neighbours; at most gs_linear_group_max() (32) entries per launch, and a (plan, replica) that repeats
 * starts a new launch (it would share K-split tickets and slabs: give such layers replicas of their own,
 * gs_plan_add_replica).  Every other entry, and a run of one entry, goes through gs_linear's own code:
 * FP8 weights, the gather families, a misaligned X, LINEAR_FUSE = 0, a call LINEAR_WS_KB splits.
 * gs_linear_batch_launches tells the launches.  The epilogue is applied in the grouped kernel's store (one
 * rounding), as in k_mfma_ks_tm.  K-split state: a grouped entry with K ranges and more than one token tile runs on
 * its replica's gs_linear state (allocated by the first call that needs it -- refused inside stream capture that
 * first time -- and zeroed on the stream ahead of the launch where it may hold another tile count's layout), an
 * entry of one tile on the upload's own; a timeout of the K-split combine reaches gs_plan_device_status as from
 * gs_linear.  Refused (GS_ERR) before the first launch, every Y untouched: a null plan, X or Y, a plan that
 * is not on the device, a bad replica, n_tokens[i] < 1, an invalid epilogue, a residual that overlaps its Y. */
int gs_linear_batch(gs_plan_t *const *plans, const int *replicas, const void *const *X, void *const *Y,
                    const int *n_tokens, const gs_epilogue *const *epi, int n, gs_stream_t stream);
/* how gs_linear_batch would enqueue these entries: returns the number of launches and writes the entries of
 * each to entries_per_launch[0 .. min(count, cap)), in order.  A grouped launch counts its entries; an entry
 * that runs through gs_linear counts as 1, whatever gs_linear enqueues for it.  < 0: a bad argument, a plan
 * that is not on the device, a bad replica.  Allocates nothing. */
int gs_linear_batch_launches(gs_plan_t *const *plans, const int *replicas, const void *const *X, const int *n_tokens,
                             int n, int *entries_per_launch, int cap);
/* the grid of one grouped launch, host only: entry i of n has nwg[i] workgroups per token tile (row blocks x
 * K ranges) and tiles[i] token tiles, and owns workgroups [begin[i], begin[i] + nwg[i] * tiles[i]); every begin
 * is a multiple of 8 and begin[n] is the grid.  GS_ERR, begin untouched: n < 1 or past gs_linear_group_max(), an
 * entry without workgroups, a grid past 2^31 - 1. */
int gs_linear_group_layout(const uint32_t *nwg, const uint32_t *tiles, int n, uint32_t *begin);
/* the most entries of one grouped launch (the kernel's arguments fit the 4 KB kernarg segment) */
int gs_linear_group_max(void);
/* The plan's pattern in one canonical order, host only: by original row, then by column; stored duplicates
 * of one coordinate are adjacent and keep their input order (for a row-major dense weight: the order of
 * its non-zeros).  row / col / val receive the original row, the column and the fp32 value the plan
 * holds of every entry; *nnz their number.  cap == 0 only returns *nnz; a smaller cap than nnz is
 * refused.  The pattern is taken when the plan is created, so it is the same after any pipeline (a
 * sorted plan's row order, interleaved storage and padding entries never reach it) and needs no upload.
 * A plan read by gs_plan_load has it unless its pipeline padded or divided the matrix (GS_ERR).
 * val may be NULL: only row / col are filled (and the call stays legal while the host values are stale, below). */
int gs_plan_pattern(gs_plan_t *p, uint64_t *row, uint64_t *col, float *val, uint64_t cap, uint64_t *nnz);
/* Value update of an uploaded plan ON THE DEVICE: only the 16-bit value words of a k_mfma_ks layout change
 * when the weight's values do; the pattern, the k-step records and the entry positions stay.  A fixed
 * gather map -- one u32 per slot of the layout's value array: the index in gs_plan_pattern's order of the
 * entry the slot holds, 0xffffffff for a slot without one -- is built on the host once, and one kernel,
 * k_set_values, rewrites the array in place from a device array of new fp32 values: per entry group 32 B of
 * map and up to 32 B of values read, 16 B written in one store; converted as gs_convert_values does, bit for
 * bit (so the plan then holds the bits of a fresh upload of those values).
 * gs_plan_values_prepare: builds the map and uploads it to the plan's device (4 B per slot, about the
 *   bytes of the plan's A itself; one map per plan, shared by its replicas, freed with the plan and by
 *   gs_plan_upload).  Synchronous, refused inside stream capture; a second call does nothing.
 * gs_plan_set_values: dev_values (a device pointer to nnz fp32 values in gs_plan_pattern's order, or NULL)
 *   enqueues one k_set_values per replica on `stream`, ordered there like any launch; keeping it ordered
 *   against launches of the same plan on OTHER streams is the caller's job.  The first call prepares the map
 *   (so it is refused inside a capture unless gs_plan_values_prepare ran); later calls allocate nothing.
 *   host_values (a host pointer to nnz fp32 values, or NULL) rewrites the plan's host copies, its stored
 *   values and the pattern's: gs_plan_pattern, gs_plan_save, a later gs_plan_upload and the deferred CSR then
 *   see them.  Given alone it is the deferred host refresh of earlier device-only updates: the caller vouches
 *   that these are the values the device holds.  Both NULL: GS_ERR.
 * Refused (GS_ERR, the reason in gs_last_error; nothing launched, the plan unchanged) unless the plan is on
 * the device, undivided, on k_mfma_ks without padded rows, at GS_F16 or GS_BF16 with GS_W_NATIVE weights,
 * holds a pattern without a coordinate stored twice (the layout sums such entries: no gather expresses
 * that), and has no CSR resident: a plan that ran at another dense width uploaded its deferred CSR, a second
 * copy of the values in another order, and updating that copy is out of scope (upload the plan again).
 * Stale host values: after an update with host_values == NULL the host copies are the old ones
 * (gs_plan_info.host_values_stale = 1) until a call with host_values or a gs_plan_upload (which uses the
 * host values and so brings the OLD ones back).  Meanwhile every reader of them refuses with a message that
 * names the cure: the first launch at another dense width or on gs_linear's three-launch path at another
 * token count (the deferred CSR), gs_plan_save, gs_plan_fp8_layout, gs_plan_pattern with val.
 * gs_plan_add_replica copies device arrays and stays legal.
 * gs_plan_value_sources: host only, no device: the map in src and, when vals16 is not NULL, the 16-bit value
 *   words exactly as gs_plan_upload(dtype) would lay them out under the current config (the analogue of
 *   gs_plan_fp8_layout).  *n_slots receives their number; cap == 0 only counts.  In the layouts that pad a
 *   group with copies of one of its entries (KS_WPOS, KS_POS8) the copies name that entry too. */
int gs_plan_values_prepare(gs_plan_t *p);
int gs_plan_set_values(gs_plan_t *p, const float *dev_values, const float *host_values, gs_stream_t stream);
int gs_plan_value_sources(gs_plan_t *p, int dtype, uint32_t *src, uint64_t cap, uint64_t *n_slots, uint16_t *vals16);
/* The sampled product on token-major operands (the weight gradient of gs_linear):
 *   out[e] = sum over t < n_tokens of G[t][row_e] * X[t][col_e],  e = 0 .. nnz - 1 in gs_plan_pattern's order.
 * G: n_tokens x M and X: n_tokens x K, row-major, one row per token, exactly as gs_linear gives Y and
 * takes X, in the plan's dtype; out: nnz fp32 values (the sums are not rounded to 16 bits).  One kernel,
 * k_sddmm_tm, whatever the plan's kernel family: it reads only the pattern.  fp32 accumulation over the
 * tokens in one fixed order, no atomics: out[e] depends on column row_e of G, column col_e of X and
 * n_tokens only, and two calls give the same bits.  A non-finite value makes the entries of its row of
 * the pattern (G) or of its column (X) NaN, and no others.
 * The plan must be on the device (for the dtype and the device) at GS_F16 or GS_BF16; an FP8-weight plan
 * is an f16 plan here.  A GS_F32 plan is refused (GS_ERR).  The pattern arrays (M + 1 offsets, nnz columns
 * of 2 bytes where K <= 65536, else 4) go to the device once per plan -- by the first call, or by
 * gs_plan_sddmm_prepare -- and are freed with the plan; the upload is synchronous, so a first call inside
 * stream capture is refused unless gs_plan_sddmm_prepare ran before.  Every argument is checked before
 * anything is uploaded or launched.  The caller guarantees the extents behind the raw pointers. */
int gs_sddmm(gs_plan_t *p, const void *G, const void *X, int n_tokens, float *out, gs_stream_t stream);
int gs_plan_sddmm_prepare(gs_plan_t *p);
/* k_sddmm_tm's tiling: output features per workgroup, input features per wave strip, tokens per chunk */
int gs_sddmm_geometry(int *row_block, int *col_strip, int *token_chunk);
/* `count` SpMMs enqueued back to back from native code, call i using replica
 * (first + i) % replicas with B_ptrs / C_ptrs entry (first + i) % n_ptrs
 * (bench rotation without a host round trip per launch) */
int gs_spmm_rotate(gs_plan_t *p, int count, int first, const void *const *B_ptrs, void *const *C_ptrs, int n_ptrs,
                   int N, gs_stream_t stream);
/* n SpMMs (plans[i], replicas[i], B[i], C[i]) enqueued on `stream` in order: a batch of
 * independent matrices (a layer's weights).  Replaces the reference's one launch per
 * sub-matrix in its multi-kernel executor (operator_executer.hpp:62-76, executor.cc:6-104):
 * consecutive entries whose plans run the K-split matrix-core kernel at N = 32 with one
 * instantiation (up to 32 of them, each a distinct (plan, replica)) are ONE grouped launch
 * (k_mfma_ks_group); the others launch as gs_spmm_replica does. */
int gs_spmm_batch(gs_plan_t *const *plans, const int *replicas, const void *const *B, void *const *C, int n, int N,
                  gs_stream_t stream);

/* gs_spmm_batch with one epilogue per entry (epi NULL, or epi[i] NULL: none for that entry).  The
 * launches are gs_spmm_batch's: an epilogue never splits a group; the entries of a grouped launch
 * apply theirs in the kernel, a single entry as gs_spmm_ex does.  Every epilogue is checked before
 * the first launch. */
int gs_spmm_batch_ex(gs_plan_t *const *plans, const int *replicas, const void *const *B, void *const *C,
                     const gs_epilogue *const *epi, int n, int N, gs_stream_t stream);

/* how gs_spmm_batch would enqueue the batch: returns the number of launches (< 0: error) and
 * the entries each launch carries in entries_per_launch[0 .. min(count, cap)) (a grouped
 * k_mfma_ks_group launch carries up to 32) */
int gs_batch_launches(gs_plan_t *const *plans, const int *replicas, int n, int N, int *entries_per_launch, int cap);
/* synchronises the device (every stream: launches of the plan on side streams must have
 * ended before the words are read and cleared; `stream` is kept for the signature) and reads
 * the plan's device error words (every replica, every
 * sub-matrix kernel): GS_ERR_DEVICE when a launch reported a fault since the last call --
 * a K-split combine that gave up waiting for a partial slab (its rows of C are NaN) --
 * 0 otherwise.  The words are cleared once reported.  The reference asserts on the host
 * after its kernels (executor.cc:6-104 checks cudaGetLastError); this is the device side. */
int gs_plan_device_status(gs_plan_t *p, gs_stream_t stream);

int gs_plan_info_get(gs_plan_t *p, gs_plan_info *info);
int gs_plan_array_count(gs_plan_t *p);
int gs_plan_array_key(gs_plan_t *p, int i, char *buf, int buf_len);
long long gs_plan_array_len(gs_plan_t *p, const char *key);      /* -1 if absent */
int gs_plan_array_is_float(gs_plan_t *p, const char *key);
int gs_plan_array_read_u64(gs_plan_t *p, const char *key, uint64_t *out, uint64_t n);
int gs_plan_array_read_f64(gs_plan_t *p, const char *key, double *out, uint64_t n);
int gs_plan_log(gs_plan_t *p, char *buf, int buf_len); /* operator / transform history */

/* model-driven index compression of one integer plan array (code_generator.cc:2618-3063,
 * the if_*_compress / get_*_compress pairs; honours MODEL_DRIVEN_COMPRESS): kind_out gets
 * "none" | "linear" | "branch" | "cycle_linear" | "cycle_increase" | "residual", expr_out the
 * expression of `idx` the generated kernel evaluates; *exact = 1 when the formula reproduces
 * the array (the reference's acceptance tests admit some it does not).  A residual adds
 * "<POS>_<name>_res_<sub>" to the plan. */
int gs_plan_index_compression(gs_plan_t *p, const char *key, char *kind_out, int kind_len, char *expr_out,
                              int expr_len, int *exact);
/* the same analysis of a raw array (type_ori: the gs data_type code of its storage type) */
int gs_index_compression_of_array(const uint64_t *a, uint64_t n, int type_ori, int branch_max, char *kind_out,
                                  int kind_len, uint64_t *params /* coef, intercept, cycle, aa, bb */, int *exact);

/* diagnostics (not part of the reference surface): one launch of the matrix-core
 * kernel's timestamped build; stamps[g*64 + i] = s_memtime of phase i in workgroup g
 * (0 start, 1 loads issued, 2 first barrier, 3 first chunk staged, 4+5j.. per chunk j:
 * top barrier, loads+clear issued, MFMA done, mid barrier, next chunk staged; 63 end) */
int gs_debug_mfma_timeline(gs_plan_t *p, const void *B, void *C, int N, gs_stream_t stream, uint64_t *stamps,
                           uint64_t n_stamps);

/* binary plan files: a compiled plan (kernel selection + every plan
 * array) in one file, loaded without re-running the transforms; upload before gs_spmm */
int gs_plan_save(gs_plan_t *p, const char *path);
int gs_plan_load(const char *path, gs_plan_t **out);

/* logical_check (metadata_set.cc:806-1890): cross-array consistency of the plan's metadata
 * (the reference's checks, with its relative-vs-absolute checks made exact); 0 consistent,
 * 1 a violation (described in msg), < 0 error.  gs_plan_compile runs it and fails on a
 * violation, as token_test asserts it after every pipeline. */
int gs_plan_logical_check(gs_plan_t *p, char *msg, int msg_len);
/* metadata editing (tools and tests): entry i of an integer plan array */
int gs_plan_array_set_u64(gs_plan_t *p, const char *key, uint64_t i, uint64_t value);

/* one call: read + pipeline + compile + upload */
int gs_plan_from_mtx(const char *path, const gs_opts *opts, gs_plan_t **out);
void gs_plan_free(gs_plan_t *p);

#ifdef __cplusplus
}
#endif
#endif
