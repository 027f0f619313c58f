// host/sddmm_layout.cc -- see sddmm_layout.hpp
#include "sddmm_layout.hpp"

#include "gs_core.hpp"

#include <algorithm>
#include <string>

namespace gs {

namespace {
template <class V>
sddmm_pattern build_pattern(uint64_t n_rows, uint64_t nnz, const uint64_t *row, const uint64_t *col, const V *val,
                            const uint64_t *orig_row, uint64_t n_orig) {
    GS_CHECK(n_rows >= 1 && n_rows < 0xffffffffull, "pattern: row count outside 32 bits");
    GS_CHECK(nnz < 0xffffffffull, "pattern: nnz exceeds 32-bit offsets");
    GS_CHECK(nnz == 0 || (row && col && val), "pattern: null argument");
    auto orig = [&](uint64_t i) {
        uint64_t r = row[i];
        if (orig_row) {
            GS_CHECK(r < n_orig, "pattern: stored row " + std::to_string(r) + " has no original row");
            r = orig_row[r];
        }
        GS_CHECK(r < n_rows, "pattern: row " + std::to_string(r) + " outside the matrix");
        return r;
    };
    sddmm_pattern p;
    p.rp.assign(n_rows + 1, 0);
    for (uint64_t i = 0; i < nnz; i++) {
        GS_CHECK(col[i] <= 0xffffffffull, "pattern: column outside 32 bits");
        p.rp[orig(i) + 1]++;
    }
    for (uint64_t r = 0; r < n_rows; r++) p.rp[r + 1] += p.rp[r];
    // entries that come in canonical order already (a row-major dense weight, a sorted CSR) are copied
    bool canonical = true;
    for (uint64_t i = 1; canonical && i < nnz; i++) {
        const uint64_t a = orig(i - 1), b = orig(i);
        canonical = a < b || (a == b && col[i - 1] <= col[i]);
    }
    if (canonical) {
        p.col.resize(nnz);
        for (uint64_t i = 0; i < nnz; i++) p.col[i] = (uint32_t)col[i];
        p.val.resize(nnz);
        for (uint64_t i = 0; i < nnz; i++) p.val[i] = (float)val[i];
        return p;
    }
    // a stable counting sort by row: entries of one row keep their input order ...
    std::vector<uint32_t> at(p.rp.begin(), p.rp.end() - 1), src(nnz);
    for (uint64_t i = 0; i < nnz; i++) src[at[orig(i)]++] = (uint32_t)i;
    // ... then a stable sort by column inside the rows that need one
    for (uint64_t r = 0; r < n_rows; r++) {
        auto b = src.begin() + p.rp[r], e = src.begin() + p.rp[r + 1];
        bool ordered = true;
        for (auto it = b; ordered && it != e && it + 1 != e; ++it) ordered = col[*it] <= col[*(it + 1)];
        if (!ordered) std::stable_sort(b, e, [&](uint32_t x, uint32_t y) { return col[x] < col[y]; });
    }
    p.col.resize(nnz);
    p.val.resize(nnz);
    for (uint64_t i = 0; i < nnz; i++) {
        p.col[i] = (uint32_t)col[src[i]];
        p.val[i] = (float)val[src[i]];
    }
    return p;
}
}  // namespace

sddmm_pattern build_sddmm_pattern(uint64_t n_rows, uint64_t nnz, const uint64_t *row, const uint64_t *col, const float *val,
                                  const uint64_t *orig_row, uint64_t n_orig) {
    return build_pattern(n_rows, nnz, row, col, val, orig_row, n_orig);
}
sddmm_pattern build_sddmm_pattern(uint64_t n_rows, uint64_t nnz, const uint64_t *row, const uint64_t *col, const double *val,
                                  const uint64_t *orig_row, uint64_t n_orig) {
    return build_pattern(n_rows, nnz, row, col, val, orig_row, n_orig);
}

std::vector<uint16_t> sddmm_cols_u16(const sddmm_pattern &p) {
    std::vector<uint16_t> out(p.col.size());
    for (size_t i = 0; i < out.size(); i++) {
        GS_CHECK(p.col[i] <= 0xffffu, "pattern: column does not fit 16 bits");
        out[i] = (uint16_t)p.col[i];
    }
    return out;
}

}  // namespace gs
