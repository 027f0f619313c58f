// host/device_layout.hpp -- the HBM layouts of the matrix-core kernels (k_mfma_rows,
// k_mfma_ks, k_nm_mfma), built on the host from a compiled plan.  Shared by the device
// upload (kernels/device_plan.hip) and the code generator (code_generator.cc), so the
// program generate_final_program emits launches exactly the layout gs_spmm runs.
#pragma once

#include "gs_core.hpp"
#include "code_generator.hpp"
#include "sddmm_layout.hpp"
#include "../hip_code/kernel_consts.hpp"

#include <algorithm>
#include <string>
#include <vector>

namespace gs {

constexpr uint32_t kMfmaThreads = 64 * gsk::kMfmaWaves;
// k_mfma_ks workgroup waves, entry sets in flight per wave (look-ahead D: 2 measured fastest
// over C2 and the OPT-30B shapes -- 1-12% under D = 4, D = 1 / 3 / 6 slower, profiles/r04o_*)
constexpr uint32_t kKsWaves = 8, kKsDepth = 2;

// fp32 -> fp16 bits, round to nearest even (bit-identical to the device conversion)
uint16_t f32_to_f16_bits(float f);
// fp32 -> bf16 bits, round to nearest even (NaN stays a quiet NaN, overflow rounds to Inf)
uint16_t f32_to_bf16_bits(float f);

// the plan dtypes (include/generalsparse.h GS_F32 / GS_F16 / GS_BF16)
constexpr int kF32 = 0, kF16 = 1, kBF16 = 2;
inline bool dtype_ok(int dtype) { return dtype == kF32 || dtype == kF16 || dtype == kBF16; }
// bytes of one element of A's values, B and C
inline uint32_t elem_bytes(int dtype) { return dtype == kF32 ? 4u : 2u; }
// the 16-bit storage word of a value at a 16-bit dtype (the upload's conversion; gs_convert_values)
inline uint16_t value_bits16(float f, int dtype) { return dtype == kBF16 ? f32_to_bf16_bits(f) : f32_to_f16_bits(f); }
// gs_convert_values: n values into the dtype's storage type (float or 16-bit words)
void convert_values(const float *in, uint64_t n, int dtype, void *out);

// ---- FP8 weight values (GS_W_FP8_E4M3): A's values of a k_mfma_ks plan as OCP e4m3fn codes, one
// byte each, and one fp32 scale per row of A: value = decode(code) * scale[row].  B, C, bias, residual and
// the accumulation stay the plan dtype's (fp16 in, fp32 sums, one rounding).
constexpr int kWNative = 0, kWFp8 = 1;  // include/generalsparse.h GS_W_NATIVE / GS_W_FP8_E4M3
// fp32 -> e4m3fn code, round to nearest even, saturated at +-448 (0x7e / 0xfe); x finite.  The NaN
// codes 0x7f / 0xff are never produced
uint8_t f32_to_e4m3_bits(float x);
// e4m3fn code -> fp32 (exact; 0x7f / 0xff: NaN)
float e4m3_bits_to_f32(uint8_t c);
// the default scale of a row whose largest magnitude is amax: 2^e with the smallest integer e such
// that amax / 2^e <= 448 (amax / scale in (224, 448]), from amax's exponent and fraction (frexp), never
// through a logarithm; amax == 0: 1.  e is kept at -126 or above, so the scale is a normal fp32
float fp8_default_scale(float amax);
// gs_quantize_fp8_rows: codes[i] = e4m3(val[i] / scale[row[i]]) (an IEEE fp32 division).  row_scale null:
// scale[r] = fp8_default_scale(max |val| of row r), 1 for a row without values; else the caller's n_rows
// scales, each finite and > 0.  Refused: a non-finite value (e4m3fn has no infinity), a row index past
// n_rows, a bad scale.  scale: n_rows entries
void quantize_fp8_rows(const float *val, const uint64_t *row, uint64_t n, uint64_t n_rows, const float *row_scale,
                       uint8_t *codes, float *scale);
// FP8 weights asked of choose_matrix_core_layout: the caller's scales (null: the default rule)
struct fp8_request {
    const float *row_scale = nullptr;
};

struct canon_rows {
    std::vector<uint32_t> rp;
    std::vector<uint64_t> col;
    std::vector<float> val;
};

canon_rows canonical_rows(const std::vector<uint32_t> &rp, const std::vector<uint64_t> &col, const universal_array &vals);

// k_mfma_rows upload layout (mfma_rows.hpp): per (BMTB g, 2^lgKC-column chunk j), the
// chunk's entries in groups of 8 = [8 x u16 halfword position in the dense image] +
// [8 x f16]; seg_start[g*nc + j] the first group
struct mfma_tiles {
    uint32_t lgKC = 0, nc = 0, RT = 0, RMAX = 0, MAXA = 0, gmax = 0;
    size_t lds_bytes = 0;
    std::vector<uint32_t> seg_start;  // in groups
    std::vector<uint16_t> pos, val;   // 8 u16 per group each, + one spare group
};

size_t mfma_lds_bytes(uint32_t lgKC, uint32_t CT, uint32_t RMAX);
// LDS one k_mfma_rows variant needs (B ring + dense images, or the compute waves' partial tiles)
size_t mfma_rows_lds_need(uint32_t lgKC, uint32_t CT, uint32_t RT, uint32_t RMAX, int glds, int nbg, int wct);
bool build_mfma_tiles(const std::vector<uint64_t> &tb_rows, const std::vector<uint32_t> &row_ptr,
                      const std::vector<uint64_t> &col, const std::vector<float> &vals, uint64_t K, uint32_t N,
                      size_t lds_budget, int64_t max_fill, mfma_tiles &t, std::string &why);

// k_mfma_ks upload layout (device_layout.cc build_ks_tiles): the groups of every (BMTB g,
// K range q, 32-column k-step s) back to back in (unit u = g*S + q, s) order, located by
// steps[2*(u*NS + s)] = first group and steps[2*(u*NS + s) + 1] = group count (at most
// GCAP, the plan's largest step: it sets MAXG), + one spare group
struct ks_tiles {
    uint32_t S = 0, NS = 0, RT = 0, RMAX = 0, MAXG = 0, GCAP = 0, W = 0;
    uint32_t CT = 0;  // 16-column MFMA tiles per workgroup (ks_ct_rt)
    bool AP = true;   // partial tiles beside the stages (ks_red_apart; KS_APART)
    bool P8 = false;  // 8-bit positions (KS_POS8): pos8 instead of pos, see build_ks_tiles
    // window positions (KS_WPOS; fp16, CT = 2, 8 waves, apart layout): pos8 holds 8 bytes per group, each
    // an entry's halfword inside the group's window of the wave image, and win one byte per group,
    // the window (image rows [5w, 5w + 5)); see build_ks_tiles
    bool WP = false;
    uint32_t NT = 0;  // k_mfma_ks NTL: 1 = A's groups by non-temporal loads (KS_NT; N = 32, 8 waves, apart layout)
    // head steps (KS_HEAD): the first W x kKsDepth k-steps of every unit -- the ones each wave loads
    // in its prologue -- have their groups at a fixed place, (unit * HS + step) * GH with HS =
    // min(W * kKsDepth, NS), padded with
    // zero-row groups to GH groups, so the prologue's group loads need no record round trip; their
    // records still describe them (first group, count), so a kernel may also take them by record
    uint32_t GH = 0;  // groups per head step (0: no head region)
    size_t lds_bytes = 0;
    std::vector<uint16_t> pos, val;  // 8 u16 per group each
    std::vector<uint8_t> val8;       // FP8 weights: 8 e4m3 codes per group in place of val (pad slots: code 0)
    std::vector<uint8_t> pos8;       // P8 / WP: 8 bytes per group
    std::vector<uint8_t> win;        // WP: one window byte per group
    std::vector<uint32_t> steps;     // per (unit, k-step): first group, group count
};

// k_mfma_ks column tiles: CT 16-column MFMA tiles per workgroup (N = 8 runs one partial
// tile), ks_col_tiles(N) tiles in the grid's y dimension (N = 128: two)
inline uint32_t ks_ct(uint32_t N) { return N <= 16 ? 1u : (N <= 32 ? 2u : 4u); }
inline uint32_t ks_col_tiles(uint32_t N) { return (N + 16 * ks_ct(N) - 1) / (16 * ks_ct(N)); }
// k_mfma_ks's own choice: N >= 128 with row blocks of at most 48 rows (RT <= 3) runs 128 columns
// per workgroup (CT = 8: 96 fp32 accumulators, 255 VGPRs, no spill), so A is read once at N = 128
// instead of once per 64-column tile; taller blocks keep CT = 4 (their accumulators would spill)
inline uint32_t ks_ct_rt(uint32_t N, uint32_t RT) { return N >= 128 && RT <= 3 ? 8u : ks_ct(N); }
// ... and the 128-column instantiations that hold their registers (no spill): 32-row blocks with up to
// 192 entry groups per k-step, 48-row blocks with up to 64; other plans at N >= 128 take CT = 4
inline bool ks_ct8_fits(uint32_t RT, uint32_t MAXG) { return (RT == 2 && MAXG <= 3) || (RT == 3 && MAXG == 1); }
// k_mfma_ks_tm (gs_linear's single launch; 32-token tiles): the (RT, MAXG) instantiations that are built --
// those that hold their registers (the kernel's resource table); other plans take the three-launch path
constexpr bool ks_tm_fits(uint32_t RT, uint32_t MAXG) { return RT >= 2 && RT <= 8 && MAXG >= 1 && MAXG <= 4; }
inline uint32_t ks_col_tiles_ct(uint32_t N, uint32_t CT) { return (N + 16 * CT - 1) / (16 * CT); }
// k_mfma_ks_tm at any token count: T = ceil(n / 32) token tiles on a 1-D grid of nb * S * T workgroups
// (nb row blocks, S K ranges, RT row tiles), T in 14 bits of the kernel's `prio` argument.
// K-split state of one tile (S > 1): a 32-token fp32 slab per (row block, K range) -- 256 * RT * 2 floats
// -- and an arrival counter per row block
constexpr uint32_t kKsTmMaxTiles = 16383;
inline uint64_t ks_tm_tile_bytes(uint64_t nb, uint32_t S, uint32_t RT) { return nb * S * RT * 2048u + nb * 4u; }
// the most tiles one launch carries: the 14 bits, a grid below 2^31 workgroups and, with S > 1, the tiles
// whose state fits ws_kb KB (LINEAR_WS_KB; at least 1: a single tile runs on the upload's own state)
inline uint32_t ks_tm_tile_cap(uint64_t nb, uint32_t S, uint32_t RT, int64_t ws_kb) {
    uint64_t cap = std::min<uint64_t>(kKsTmMaxTiles, 0x7fffffffull / std::max<uint64_t>(1, nb * S));
    if (S > 1) cap = std::min<uint64_t>(cap, (uint64_t)std::max<int64_t>(0, ws_kb) * 1024u / ks_tm_tile_bytes(nb, S, RT));
    return (uint32_t)std::max<uint64_t>(1, cap);
}
// the launches of an n-token call, in token order: tiles per launch, each at most `cap`
inline std::vector<uint32_t> ks_tm_tile_split(uint32_t n_tokens, uint32_t cap) {
    std::vector<uint32_t> out;
    for (uint32_t left = (n_tokens + 31u) / 32u; left; left -= out.back()) out.push_back(std::min(left, cap));
    return out;
}
// the grid of one k_mfma_ks_tm_group launch (gs_linear_batch): entry i of n owns workgroups [begin[i], begin[i] +
// nwg[i] * tiles[i]); every begin is rounded up to a multiple of 8 (the entry's block numbers keep the XCD residues
// xcd_block assumes; the workgroups in between exit at once) and begin[n] is the grid.  False -- begin untouched --
// for no entry, more than kKsTmGroupMax, an entry without workgroups or a grid past 2^31 - 1
inline bool ks_tm_group_layout(const uint32_t *nwg, const uint32_t *tiles, size_t n, uint32_t *begin) {
    if (n < 1 || n > (size_t)gsk::kKsTmGroupMax) return false;
    uint64_t at[gsk::kKsTmGroupMax + 1] = {0};
    for (size_t i = 0; i < n; i++) {
        const uint64_t wg = (uint64_t)nwg[i] * tiles[i];
        if (wg < 1 || wg > 0x7fffffffull) return false;
        at[i + 1] = i + 1 < n ? (at[i] + wg + 7u) & ~7ull : at[i] + wg;
        if (at[i + 1] > 0x7fffffffull) return false;
    }
    for (size_t i = 0; i <= n; i++) begin[i] = (uint32_t)at[i];
    return true;
}

bool build_ks_tiles(const std::vector<uint64_t> &tb_rows, const std::vector<uint32_t> &row_ptr,
                    const std::vector<uint64_t> &col, const std::vector<float> &vals, uint64_t K, uint32_t N,
                    int64_t s_cfg, int64_t min_rows, int64_t max_fill, ks_tiles &t, std::string &why, int dtype = kF16,
                    const std::vector<uint8_t> *codes = nullptr,  // codes: vals' e4m3 codes -> t.val8, t.val left empty
                    std::vector<uint32_t> *src = nullptr);  // src: per slot of t.val the index into vals of its entry (kNoValue: none)

// a slot of ks_tiles::val that holds no entry: a group's zero-row padding, a head slot's spare groups, the spare group
constexpr uint32_t kNoValue = 0xffffffffu;

// k_mfma_bm upload layout: unit u = (BMTB g, K range q) of NS 32-column k-steps; per
// (u*NS + step)*64 + lane one 8-byte record (rec[2i] = mask bytes of tiles 0..3, rec[2i+1]
// = tiles 4..5 | u16 value offset << 16), sbase[u*NS + step] the step's first value, the
// values (f16 bits) lane after lane, tile after tile, ascending columns (+ 16 halves pad)
struct bm_tiles {
    uint32_t S = 0, NS = 0, RT = 0, RMAX = 0, W = 0;
    bool kb = false;  // k_mfma_kb (8 waves, k_mfma_ks pipeline)
    uint32_t NVB = 0;  // ... KB of values per k-step (1, 2 or 4)
    bool v2 = false;  // k_mfma_bm2 (one wave per row tile, B slice resident in LDS)
    size_t lds_bytes = 0;
    std::vector<uint32_t> rec;
    std::vector<uint32_t> sbase;
    std::vector<uint16_t> val;
};

bool build_bm_tiles(const std::vector<uint64_t> &tb_rows, const std::vector<uint32_t> &row_ptr,
                    const std::vector<uint64_t> &col, const std::vector<float> &vals, uint64_t K, uint32_t N,
                    int64_t s_cfg, int64_t waves, int64_t max_fill, bm_tiles &t, std::string &why);

// k_nm_mfma upload layout: one 4,608-B block per (64-row group, 64-column k-step)
bool build_nm_panels(const std::vector<uint64_t> &rows, const std::vector<uint64_t> &col, const universal_array &vals,
                     uint64_t row_num, uint64_t K, std::vector<unsigned char> &blk, uint32_t &S, std::string &why,
                     uint32_t T = 8);
// k_nm_mfma's 16-row tiles per workgroup for a row count (NM_TILES = 0): among T = 8, 7, 4, 2
// (7 only below N = 128) the fewest tiles per CU (ceil(workgroups / 256 CUs) x T), ties to the
// larger T
uint32_t nm_tiles_for(uint64_t row_num, int64_t cfg_tiles, uint32_t N);

// The matrix-core layout gs_spmm runs for a compiled plan at its dense width
// (DENSE_MATRIX_SIZE), chosen and built once here for both the device upload and the
// emitted program: k_nm_mfma for col-direction 2:4 panels, k_mfma_ks for row blocks of
// >= KS_MIN_ROWS rows, k_mfma_rows for the other fp16 BMTB plans; NONE = a gather family.
// The k_mfma_rows variant (B by LDS-DMA or registers, ring depth, compute waves) is fixed
// here from the config, so the LDS size and the launch agree whatever changes later.
struct mc_layout {
    enum kind_t { NONE, ROWS, KS, NM, BM } kind = NONE;
    uint32_t N = 0;
    std::vector<uint64_t> tbr;  // BMTB first rows (ROWS, KS)
    mfma_tiles rows;
    uint32_t rows_ksplit = 1, rows_ncs = 0;  // k_mfma_rows K ranges per row block, chunks per range
    int rows_glds = 2, rows_nbg = 3, rows_wct = 6, rows_maxa = 1;  // k_mfma_rows template arguments
    bool rows_flags = false;  // ... FLG (MFMA_FLAGS: LDS counter hand-offs, GLDS 2 / NBG 3 / 6 compute waves)
    ks_tiles ks;
    bm_tiles bm;
    std::vector<unsigned char> nm_blk;  // k_nm_mfma blocks
    uint32_t nm_S = 0;                  // ... k-steps per row group
    uint32_t nm_T = 8;                  // ... 16-row tiles per workgroup (nm_tiles_for)
    uint64_t nm_rows = 0;
    bool nm_ks = false;                    // k_nm_mfma_ks (256-row workgroups, K split) instead of k_nm_mfma
    bool nm4 = false;                      // k_nm_mfma4 (256-row workgroups of 8 waves, K split, B by LDS-DMA)
    bool nm_nt = false;                    // k_nm_mfma: A's panel blocks by non-temporal loads (NM_NT)
    uint32_t nm_split = 1, nm_ncs = 0;     // ... K ranges per row block, 256-column chunks per range
    std::vector<float> w8_scale;  // FP8 weights (KS): the scale of every row of the plan
    // value sources (KS, asked for by choose_matrix_core_layout's want_src): per slot of ks.val the canonical
    // entry it holds (kNoValue: none), and the canonical rows themselves (the plan's stored row order)
    std::vector<uint32_t> ks_src, cr_rp;
    std::vector<uint64_t> cr_col;
    std::string why;  // why NONE
};
// w8 (null: the dtype's own values): a k_mfma_ks layout gets ks.val8 and w8_scale instead of ks.val; the
// caller checks the layout with check_fp8_layout
mc_layout choose_matrix_core_layout(const meta_data_set &m, const kernel_spec &sp, int sb, uint64_t K, int dtype,
                                    const fp8_request *w8 = nullptr, bool want_src = false);

// The value-source map of a compiled k_mfma_ks plan (gs_plan_set_values, k_set_values): where every slot of
// the layout's value array -- ks_tiles::val, on the device device_arrays::tval -- takes its value from.
//   src[slot]     index in the plan's pattern (canonical order) of the entry the slot holds, kNoValue for a
//                 slot without one.  The layouts that pad a group with copies of one of its entries (KS_WPOS,
//                 KS_POS8) name that entry in the copies too: both slots scatter to one place
//   host_pos[e]   position of pattern entry e in the plan's stored nz_vals
//   vals16        the value words exactly as the upload lays them out at `dtype` under the current config
// Built from the same choose_matrix_core_layout call as the upload's, so it is the map of that layout.
// Throws a gs_error: a plan off k_mfma_ks, with padded rows or padding entries, interleaved storage, or a
// pattern that holds a coordinate twice (canonical_rows sums those: no gather expresses that)
struct value_map {
    std::vector<uint32_t> src, host_pos;
    std::vector<uint16_t> vals16;
    uint64_t layout_hash = 0;  // ks_layout_hash of the layout the map belongs to
};
// a hash of everything that places a k_mfma_ks layout's values (positions, windows, step records, geometry): the
// upload keeps it, so a map built later -- under a config that may have changed -- is known to be that layout's
uint64_t ks_layout_hash(const ks_tiles &t);
value_map build_value_map(const meta_data_set &m, const kernel_spec &sp, int sb, uint64_t M, uint64_t K, int dtype,
                          const sddmm_pattern &pat);
// FP8 weights run on k_mfma_ks in the release layout only (CT = 2: a plan built for 17 .. 32 columns, 8
// waves, the apart layout, 16-bit positions, the static grid, ks_tm_fits, K % 8 == 0): throws a gs_error
// that names the condition a layout misses
void check_fp8_layout(const mc_layout &mc, uint64_t K);

}  // namespace gs
