// hip_code/host_layouts.hpp -- host-only (no HIP header needed).
// ---------------------------------------------------------------------------
// Host-side helpers shared by the library (kernels/device_plan.hip) and the
// programs code_generator emits: the kernel-side layouts derived from plan
// arrays.
// ---------------------------------------------------------------------------
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace gsk_host {

// CSR row pointer (u32) of a row-sorted COO row array
inline std::vector<uint32_t> csr_row_ptr(const std::vector<uint64_t> &row, uint64_t row_num) {
    std::vector<uint32_t> rp(row_num + 1, 0);
    for (uint64_t r : row) rp[r + 1]++;
    for (uint64_t i = 0; i < row_num; i++) rp[i + 1] += rp[i];
    return rp;
}

// per fixed-nnz BMT, bit i set iff its i-th nz starts a row (no forced BMW heads)
inline std::vector<uint64_t> row_start_masks(const std::vector<uint64_t> &row, const std::vector<uint64_t> &first_nz) {
    std::vector<uint64_t> mask(first_nz.size() - 1, 0);
    for (size_t i = 0; i + 1 < first_nz.size(); i++) {
        uint64_t mm = 0;
        for (uint64_t j = first_nz[i]; j < first_nz[i + 1]; j++)
            if (j == 0 || row[j] != row[j - 1]) mm |= 1ull << (j - first_nz[i]);
        mask[i] = mm;
    }
    return mask;
}

// k_row_chunks: BMTs per wave (enough waves to fill 256 CUs eight deep)
inline uint32_t row_chunk_span(size_t n_bmt) {
    const size_t u = (n_bmt + 8191) / 8192;
    return (uint32_t)(u < 8 ? 8 : u);
}

// rows k_row_chunks leaves to k_finalize_rows: rows without BMTs and rows whose
// BMTs straddle two waves' ranges (output rows = row_base + plan row)
inline std::vector<uint32_t> row_chunk_finalize_rows(const std::vector<uint32_t> &bmt_row, uint64_t M, uint32_t U,
                                                     uint32_t row_base) {
    std::vector<uint8_t> fin(M, 1);
    for (uint32_t r : bmt_row) fin[r + row_base] = 0;
    for (size_t i = U; i < bmt_row.size(); i += U)
        if (bmt_row[i] == bmt_row[i - 1]) fin[bmt_row[i] + row_base] = 1;
    std::vector<uint32_t> list;
    for (uint64_t r = 0; r < M; r++)
        if (fin[r]) list.push_back((uint32_t)r);
    return list;
}

// k_merge_path: nz-exact wave ranges from the plan's merge-path levels, and the
// compact non-empty rows.  Level w starts at path step p = w*work_size; the
// reference records (row j's index, p - j) for the first non-empty row j with
// total_path[j] > p (get_begin_{rows,nzs}_of_level_after_merge_path.cc:84-94).
// total_path[j] = ends[j] + j, so p == ends[j-1] + j - 1 is the step that
// closes row j-1: the nonzeros consumed there are ends[j-1] = (p - j) + 1;
// otherwise p - j.  Consecutive levels are grouped into waves of at least
// target_steps path steps; waves never have an empty nz range.  snap > 0: a wave
// boundary strictly inside a row of at most `snap` nonzeros moves to the nearer end of
// that row, so the row is summed by one wave (no cross-wave combine for it; the
// reference's own merge path splits such rows over threads and adds them atomically).
struct merge_path_layout {
    std::vector<uint32_t> wz, wq, ends, rid, empty;  // empty: output rows without nonzeros
    // rows split across waves: chain[w] = the wave closing the row open at w's end,
    // chain[W + w] = the first wave of the row w closes at its head (~0: none)
    std::vector<uint32_t> chain;
};

// the split-row chains of a layout (k_merge_path's in-launch combine)
inline void merge_path_chains(merge_path_layout &L) {
    const size_t W = L.wz.size() - 1;
    L.chain.assign(2 * W, 0xffffffffu);
    uint32_t start = 0xffffffffu;
    size_t q_last = 0;
    for (size_t w = 0; w < W; w++) {
        const uint32_t zlo = L.wz[w], zhi = L.wz[w + 1], q0 = L.wq[w];
        const bool head_open = zlo > (q0 ? L.ends[q0 - 1] : 0u);
        q_last = std::max<size_t>(q_last, q0);
        while (L.ends[q_last] < zhi) q_last++;  // the row holding position zhi - 1
        const bool end_open = L.ends[q_last] > zhi;
        const bool through = head_open && end_open && q_last == q0;  // the row spans the whole wave
        if (head_open && !through) {
            L.chain[W + w] = start;
            for (uint32_t v = start; v < w; v++) L.chain[v] = (uint32_t)w;
            start = 0xffffffffu;
        }
        if (end_open && !through) start = (uint32_t)w;
    }
}

inline bool merge_path_device_layout(const std::vector<uint64_t> &row, uint64_t row_num,
                                     const std::vector<uint64_t> &lvl_rows, const std::vector<uint64_t> &lvl_nzs,
                                     uint64_t work_size, uint32_t row_base, uint64_t target_steps,
                                     merge_path_layout &out, std::string &why, uint64_t out_rows = 0,
                                     uint64_t snap = 0) {
    out = merge_path_layout();
    std::vector<uint32_t> cnt(row_num, 0);
    for (uint64_t r : row) {
        if (r >= row_num) { why = "row index beyond the row count"; return false; }
        cnt[r]++;
    }
    std::vector<uint64_t> crow;  // plan row of compact row j
    uint64_t acc = 0;
    for (uint64_t r = 0; r < row_num; r++)
        if (cnt[r]) {
            acc += cnt[r];
            if (acc > 0xffffffffull) { why = "nnz exceeds 32 bits"; return false; }
            out.ends.push_back((uint32_t)acc);
            out.rid.push_back((uint32_t)(r + row_base));
            crow.push_back(r);
        } else {
            out.empty.push_back((uint32_t)(r + row_base));
        }
    for (uint64_t r = row_base + row_num; r < out_rows; r++) out.empty.push_back((uint32_t)r);
    const uint64_t R = crow.size();
    if (R == 0 || lvl_rows.empty() || lvl_nzs.size() != lvl_rows.size() + 1 || lvl_nzs.back() != acc || work_size == 0) {
        why = "merge-path level arrays do not match the matrix";
        return false;
    }
    uint64_t j = 0, gz = 0, gp = 0;
    out.wz.push_back(0);
    out.wq.push_back(0);
    for (uint64_t w = 0; w < lvl_rows.size(); w++) {
        while (j < R && crow[j] < lvl_rows[w]) j++;
        const uint64_t p = w * work_size;
        if (j == R || crow[j] != lvl_rows[w] || p < j || lvl_nzs[w] != p - j) {
            why = "merge-path level " + std::to_string(w) + " is not on the path";
            return false;
        }
        uint64_t z = (j >= 1 && p == (uint64_t)out.ends[j - 1] + j - 1) ? (uint64_t)out.ends[j - 1] : p - j;
        uint64_t q = j;
        if (w == 0 || p - gp < target_steps) continue;
        if (snap && q < R) {
            const uint64_t rs = q ? out.ends[q - 1] : 0, re = out.ends[q];
            if (z > rs && re - rs <= snap) {
                if (z - rs <= re - z) {
                    z = rs;
                } else {
                    z = re;
                    q++;
                }
            }
        }
        if (z <= gz || z >= acc) continue;
        out.wz.push_back((uint32_t)z);
        out.wq.push_back((uint32_t)q);
        gz = z;
        gp = p;
    }
    out.wz.push_back((uint32_t)acc);
    out.wq.push_back((uint32_t)R);
    merge_path_chains(out);
    return true;
}

}  // namespace gsk_host
