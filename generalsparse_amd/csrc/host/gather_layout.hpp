// host/gather_layout.hpp -- the HBM layouts of the gather, merge-path, bitmap and LDS-staged
// families (k_lds_rows*, k_merge_path, k_bitmap_segment), built on the host from plan arrays.
// Plain C++ (no GPU call): kernels/device_plan.hip only copies what these return.
#pragma once

#include "device_layout.hpp"
#include "../hip_code/host_layouts.hpp"

#include <string>
#include <vector>

namespace gs {

// CSR row pointer of the (possibly padded, row-sorted) COO, row indices checked
std::vector<uint32_t> csr_row_ptr(const std::vector<uint64_t> &row, uint64_t row_num);

inline uint32_t pow2ceil(uint32_t x) {
    uint32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}

// lanes per dense row of the gather families: N columns in pieces of 16 B when N allows (else
// one element), rounded up to a power of two, at most one wave
inline uint32_t lanes_per_row(uint32_t N, uint32_t ebytes) {
    const uint32_t cfv = 16u / ebytes, cf = N % cfv == 0 ? cfv : 1u;
    return std::min<uint32_t>(64u, pow2ceil((N + cf - 1) / cf));
}
// merge-path steps a wave's range aims at: one round (kMpItems steps) per 64 / X row slot
inline uint64_t merge_path_target(uint32_t N, uint32_t ebytes) {
    return (uint64_t)gsk::kMpItems * (64u / lanes_per_row(N, ebytes));
}

// ------------------------------------------------------------------ LDS tiles
// Chunk-major A layout for k_lds_rows (lds_rows.hpp): for BMTB g and column
// chunk j = [j*KC, (j+1)*KC), the entries of g's rows whose columns fall in the
// chunk, row after row, each row padded to 4 entries (its last column of the chunk, value 0) and
// the segment padded to 8 entries so it stages as whole 16-B units.
struct lds_tiles {
    uint32_t KC = 0, nc = 0, RSB = 0, rpw_max = 0, seg_cap = 0, waves = 0, maxr = 0;
    size_t lds_bytes = 0;
    std::vector<uint32_t> seg_start, seg_row_off;
    std::vector<uint16_t> tcol;
    std::vector<uint32_t> src;  // source entry per tile entry (~0u: padding)
};

constexpr int kLdsMaxU = 12;  // 16-B staging registers per thread (k_lds_rows MAXU)

// returns false (and the reason) when the plan/shape does not fit the kernel
bool build_lds_tiles(const std::vector<uint64_t> &tb_rows, const std::vector<uint64_t> &tb_bmw,
                     const std::vector<uint64_t> &bmw_rows, const std::vector<uint32_t> &row_ptr,
                     const std::vector<uint64_t> &col, uint64_t K, uint32_t N, uint32_t vbytes, size_t lds_budget,
                     lds_tiles &t, std::string &why, bool dma = false, uint64_t want = 1);

// merge-path levels of a compact CSR walked at `work_size` steps of the path (rows consumed +
// nonzeros consumed): level w at diagonal p = w * work_size has consumed j rows (row i is consumed
// at path position ends[i] + i + 1) and p - j nonzeros -- the split the reference's merge-path
// operators produce (get_begin_rows_of_level_after_merge_path.cc), for CSRs the plan never held
// (the column partitions of MP_COL_PARTS)
void merge_path_levels(const std::vector<uint64_t> &rows, uint64_t row_num, uint64_t work_size,
                       std::vector<uint64_t> &lr, std::vector<uint64_t> &ln);

// Columns ranked by degree: perm[r] = the column of rank r, rank[c] = the rank of column c.
// hot = 0 (or >= K): most nonzeros first, ties by column (a stable sort).  hot = H (MP_PERM_HOT):
// the H densest columns first (by degree, then column), the rest in their own order
struct column_ranks {
    std::vector<uint32_t> perm, rank;
};
column_ranks column_order(const std::vector<uint64_t> &col, uint64_t K, uint64_t hot);

// MP_COL_PARTS: columns ranked by degree (column_order), rank r in partition r % P at position
// base[r % P] + r / P of the gathered B; hub = H (P = 2): partition 0 = the H densest columns,
// partition 1 = the rest.  Per partition its entries in row order: row, position of the column
// in the gathered B, source entry
struct col_part {
    std::vector<uint64_t> rows;
    std::vector<uint32_t> cols, src;
};
struct col_parts {
    std::vector<uint64_t> base;    // P + 1: first position of each partition
    std::vector<uint32_t> gather;  // column at each position of the gathered B
    std::vector<col_part> parts;
};
col_parts split_col_parts(const std::vector<uint64_t> &rows, const std::vector<uint64_t> &col, uint64_t K, uint32_t P,
                          uint64_t hub);

// bitmap family at a 16-bit C: the output rows k_finalize_rows writes -- rows of [out_lo, out_hi)
// that are empty or outside the plan's rows, and rows a BMT boundary (first_nz) splits
std::vector<uint32_t> bitmap_finalize_rows(const std::vector<uint64_t> &rows, const std::vector<uint64_t> &first_nz,
                                           const std::vector<uint32_t> &row_ptr, uint64_t row_num, uint64_t M,
                                           uint64_t row_base, uint64_t out_lo, uint64_t out_hi);

}  // namespace gs
