// host/sddmm_layout.hpp -- the pattern of a plan in one canonical order, and the device form of it
// that k_sddmm_tm (hip_code/sddmm.hpp) samples by.  Pure host code: no device, no HIP.
//
// Canonical order: by original row, then by column; stored duplicates of one coordinate are adjacent
// and keep their input order.  For a row-major dense weight this is the order of its non-zeros.
#pragma once

#include <cstdint>
#include <vector>

namespace gs {

struct sddmm_pattern {
    std::vector<uint32_t> rp;   // rows + 1 offsets into col / val (empty: no pattern)
    std::vector<uint32_t> col;  // nnz columns, ascending inside a row
    std::vector<float> val;     // nnz values, as the plan holds them (fp32)
    uint64_t rows() const { return rp.empty() ? 0 : rp.size() - 1; }
    uint64_t nnz() const { return col.size(); }
};

// The canonical pattern of nnz entries (row[i], col[i], val[i]) given in any order.  orig_row (null:
// the identity) maps a stored row index to the original row, as a sorted plan's
// original_nz_row_indices does; n_rows counts original rows.  Throws gs_error: an index outside
// n_rows x 2^32, orig_row not covering a stored row, nnz beyond 32-bit offsets.
sddmm_pattern build_sddmm_pattern(uint64_t n_rows, uint64_t nnz, const uint64_t *row, const uint64_t *col, const float *val,
                                  const uint64_t *orig_row = nullptr, uint64_t n_orig = 0);
// (values held as doubles, as a plan's metadata holds them: each rounded to fp32)
sddmm_pattern build_sddmm_pattern(uint64_t n_rows, uint64_t nnz, const uint64_t *row, const uint64_t *col, const double *val,
                                  const uint64_t *orig_row = nullptr, uint64_t n_orig = 0);

// the device form: rp as it stands (rows + 1 u32), the columns as u16 where K <= 65536 (the CSR
// upload's choice), else u32
inline int sddmm_col_bytes(uint64_t K) { return K <= 65536 ? 2 : 4; }
// the columns as u16 (sddmm_col_bytes(K) == 2); throws when a column does not fit
std::vector<uint16_t> sddmm_cols_u16(const sddmm_pattern &p);

}  // namespace gs
