// host/gather_layout.cc -- see gather_layout.hpp
#include "gather_layout.hpp"

#include <algorithm>

namespace gs {

std::vector<uint32_t> csr_row_ptr(const std::vector<uint64_t> &row, uint64_t row_num) {
    for (uint64_t r : row) GS_CHECK(r < row_num, "row index beyond row count");
    return gsk_host::csr_row_ptr(row, row_num);
}

// returns false (and the reason) when the plan/shape does not fit the kernel
bool build_lds_tiles(const std::vector<uint64_t> &tb_rows, const std::vector<uint64_t> &tb_bmw,
                     const std::vector<uint64_t> &bmw_rows, const std::vector<uint32_t> &row_ptr,
                     const std::vector<uint64_t> &col, uint64_t K, uint32_t N, uint32_t vbytes, size_t lds_budget,
                     lds_tiles &t, std::string &why, bool dma, uint64_t want) {
    const uint64_t nb = tb_rows.size() - 1;
    if (nb == 0 || K == 0) { why = "empty plan"; return false; }
    if ((N * vbytes) % 16 != 0) { why = "B rows are not whole 16-B units"; return false; }
    const uint32_t UB = N * vbytes / 16;
    if (UB > 64 || (UB & (UB - 1))) { why = "16-B units per B row must be a power of two <= 64"; return false; }
    uint32_t waves = 0, maxr = 0, rpw = 0;
    for (uint64_t g = 0; g < nb; g++) {
        const uint64_t w0 = tb_bmw[g], w1 = tb_bmw[g + 1];
        if (w1 <= w0 || bmw_rows[w0] != tb_rows[g] || bmw_rows[w1] != tb_rows[g + 1]) {
            why = "BMWs do not tile their BMTB";
            return false;
        }
        waves = std::max<uint32_t>(waves, (uint32_t)(w1 - w0));
        rpw = std::max<uint32_t>(rpw, (uint32_t)(tb_rows[g + 1] - tb_rows[g]));
        for (uint64_t w = w0; w < w1; w++) maxr = std::max<uint32_t>(maxr, (uint32_t)(bmw_rows[w + 1] - bmw_rows[w]));
    }
    if (waves > 16) { why = "more than 16 BMWs per BMTB"; return false; }
    // BMWs of 5..8 rows: one row per slot (k_lds_rows_rs; fp32 N = 32 by LDS-DMA only)
    const bool rowslot = dma && vbytes == 4 && N == 32 && maxr > 4 && maxr <= 8;
    if (maxr > 4 && !rowslot) { why = "more than 4 rows per BMW"; return false; }
    maxr = maxr <= 1 ? 1 : (maxr <= 2 ? 2 : (maxr <= 4 ? 4 : 8));
    // B rows in LDS at an odd count of 16-B units (bank spread for random rows), except fp32 at
    // N = 32 (8 lanes x 16 B per row, 8 slots per wave): rows at 128 B, so a row starts on bank 0
    // or 32 by its parity, and each row's entries are ordered so that the slots whose B reads
    // share an LDS cycle (ds_read_b128 lane groups: slots {0,3} and {1,2} of each half-wave) read
    // rows of opposite parity -- conflict-free (pair_banks below; r06 PMC: 42% of the LDS cycles
    // were bank conflicts with the odd stride)
    const bool pair_banks = vbytes == 4 && N == 32;
    const uint32_t RSB = pair_banks ? N * vbytes : N * vbytes + (UB % 2 == 0 ? 16u : 0u);
    const uint32_t ebytes = 2 + vbytes;
    const uint64_t nthr = 64ull * waves;
    const uint64_t max_kc = std::min<uint64_t>(K, 65536);
    // smallest chunk count whose largest segment still fits LDS and the staging registers
    uint64_t nc = std::max<uint64_t>(1, (K * RSB * (dma ? 2 : 1) + lds_budget / 2) / (lds_budget * 3 / 4));
    // want > 1 (the plan's K split): past the first chunk count that fits, a few more are tried and
    // the one with the fewest columns in the longest K range is kept -- a range is whole chunks, so
    // 32 chunks in 6 ranges (6+6+6+6+6+2) run 6 chunks of 160 columns where 36 would run 6 of 144
    // (C2 fp32 (64,8): 27.6 -> 25.8 us, profiles/r06zj)
    bool found = false;
    uint64_t nc_first = 0, best_cost = 0;
    for (;; nc++) {
        uint64_t KC = (K + nc - 1) / nc;
        KC = (KC + 7) / 8 * 8;
        if (KC > max_kc) continue;
        if (KC < 64 && nc > 1) {
            if (found) break;
            why = "column chunks would be under 64 rows of B";
            return false;
        }
        const uint64_t ncc = (K + KC - 1) / KC;
        uint64_t cap = 0;
        std::vector<uint64_t> segl(ncc);
        for (uint64_t g = 0; g < nb; g++) {
            std::fill(segl.begin(), segl.end(), 0);
            for (uint64_t r = tb_rows[g]; r < tb_rows[g + 1]; r++) {
                uint64_t e = row_ptr[r];
                while (e < row_ptr[r + 1]) {
                    const uint64_t j = col[e] / KC;
                    uint64_t e1 = e;
                    while (e1 < row_ptr[r + 1] && col[e1] / KC == j) e1++;
                    segl[j] += (e1 - e + 3) / 4 * 4;
                    e = e1;
                }
            }
            for (uint64_t j = 0; j < ncc; j++) cap = std::max(cap, (segl[j] + 7) / 8 * 8);
        }
        const uint64_t lds = KC * RSB + cap * ebytes + (rpw + 1) * 4;
        const uint64_t units = KC * UB + cap * ebytes / 16;
        // k_lds_rows_dma / _rs: two buffers of B rows + columns + values (row offsets by loads)
        const uint64_t buf = KC * RSB + std::max<uint64_t>(cap, 8) * ebytes;
        const bool fits = dma ? 2 * buf <= lds_budget : lds <= lds_budget && units <= (uint64_t)kLdsMaxU * nthr;
        if (fits) {
            const uint64_t w = std::max<uint64_t>(1, std::min<uint64_t>(want, ncc));
            const uint64_t cost = (ncc + w - 1) / w * KC;  // columns of the longest K range
            if (!found || cost < best_cost) {
                t.KC = (uint32_t)KC;
                t.nc = (uint32_t)ncc;
                t.seg_cap = (uint32_t)std::max<uint64_t>(cap, 8);
                t.lds_bytes = dma ? (size_t)(2 * buf + 15) / 16 * 16
                                  : (size_t)(KC * RSB + (uint64_t)t.seg_cap * ebytes + (rpw + 1) * 4 + 15) / 16 * 16;
                best_cost = cost;
            }
            if (!found) {
                found = true;
                nc_first = nc;
            }
        }
        if (found && (want <= 1 || nc >= nc_first + 2 * want)) break;
        if (nc > K) {
            if (found) break;
            why = "no chunking fits LDS";
            return false;
        }
    }
    if (rowslot && (uint64_t)t.KC * RSB > 65536) { why = "row-per-slot chunks over 511 B rows"; return false; }
    t.RSB = RSB;
    t.rpw_max = rpw;
    t.waves = waves;
    t.maxr = maxr;
    t.seg_start.assign(1, 0);
    t.seg_row_off.assign(nb * t.nc * (rpw + 1), 0);
    std::vector<uint64_t> cur(rpw);
    std::vector<uint32_t> slot_of(rpw);  // rowslot: a row's slot = its place in its BMW
    for (uint64_t g = 0; g < nb; g++) {
        const uint64_t r0 = tb_rows[g], nr = tb_rows[g + 1] - r0;
        for (uint64_t i = 0; i < nr; i++) cur[i] = row_ptr[r0 + i];
        if (rowslot)
            for (uint64_t w = tb_bmw[g]; w < tb_bmw[g + 1]; w++)
                for (uint64_t r = bmw_rows[w]; r < bmw_rows[w + 1]; r++) slot_of[r - r0] = (uint32_t)(r - bmw_rows[w]);
        for (uint32_t j = 0; j < t.nc; j++) {
            const uint64_t lim = (uint64_t)(j + 1) * t.KC, base = t.tcol.size();
            uint32_t *off = &t.seg_row_off[(g * t.nc + j) * (rpw + 1)];
            for (uint64_t i = 0; i < nr; i++) {
                off[i] = (uint32_t)(t.tcol.size() - base);
                uint64_t e = cur[i];
                const uint64_t e_end = row_ptr[r0 + i + 1];
                for (; e < e_end && col[e] < lim; e++) {
                    t.tcol.push_back((uint16_t)(col[e] - (uint64_t)j * t.KC));
                    t.src.push_back((uint32_t)e);
                }
                cur[i] = e;
                // padding entries (value 0) repeat the row's last column of this chunk, never a column
                // the row does not hold: 0 x a non-finite B value must not reach another row's result
                // (a row with no entry in the chunk ends on a multiple of 4 and gets no padding)
                while ((t.tcol.size() - base) % 4) { t.tcol.push_back(t.tcol.back()); t.src.push_back(~0u); }
                if (rowslot) {
                    // slot s reads entry 4i + q of its row in the q-th read of iteration i: slots
                    // {0,1,4,5} take column parity k & 1 at entry k, slots {2,3,6,7} the opposite
                    // (the b128 lane groups pair slots {0,3} and {1,2} of each half-wave)
                    const size_t rs = base + off[i], re = t.tcol.size();
                    const uint32_t ph = (slot_of[i] & 2u) ? 1u : 0u;
                    std::vector<std::pair<uint16_t, uint32_t>> ev, od;
                    for (size_t k = rs; k < re; k++) (t.tcol[k] & 1u ? od : ev).push_back({t.tcol[k], t.src[k]});
                    std::reverse(ev.begin(), ev.end());
                    std::reverse(od.begin(), od.end());
                    for (size_t k = rs; k < re; k++) {
                        const bool want_odd = ((k - rs + ph) & 1u) != 0u;
                        auto &v = (want_odd && !od.empty()) || ev.empty() ? od : ev;
                        t.tcol[k] = v.back().first;
                        t.src[k] = v.back().second;
                        v.pop_back();
                    }
                } else if (pair_banks) {
                    // per 32-entry block of the row (slot s takes entries 4s..4s+3, entry q in the
                    // q-th read): the reads of slots (0,3), (1,2), (4,7), (5,6) at one q get one
                    // even and one odd column while both kinds last (any entry order sums the row)
                    static const int pairs[4][2] = {{0, 3}, {1, 2}, {4, 7}, {5, 6}};
                    const size_t rs = base + off[i], re = t.tcol.size();
                    for (size_t b0 = rs; b0 < re; b0 += 32) {
                        const size_t n = std::min<size_t>(32, re - b0);
                        std::vector<std::pair<uint16_t, uint32_t>> ev, od;
                        for (size_t k = 0; k < n; k++) (t.tcol[b0 + k] & 1u ? od : ev).push_back({t.tcol[b0 + k], t.src[b0 + k]});
                        auto take = [&](bool want_odd) {
                            auto &v = (want_odd && !od.empty()) || ev.empty() ? od : ev;
                            const auto x = v.back();
                            v.pop_back();
                            return x;
                        };
                        for (int q = 0; q < 4; q++)
                            for (const auto &pr : pairs) {
                                const size_t pa = (size_t)pr[0] * 4 + q, pb = (size_t)pr[1] * 4 + q;
                                if (pa < n) {
                                    const auto x = take(ev.size() < od.size());
                                    t.tcol[b0 + pa] = x.first;
                                    t.src[b0 + pa] = x.second;
                                    if (pb < n) {
                                        const auto y = take(!(x.first & 1u));
                                        t.tcol[b0 + pb] = y.first;
                                        t.src[b0 + pb] = y.second;
                                    }
                                } else if (pb < n) {
                                    const auto y = take(false);
                                    t.tcol[b0 + pb] = y.first;
                                    t.src[b0 + pb] = y.second;
                                }
                            }
                    }
                }
            }
            for (uint64_t i = nr; i <= rpw; i++) off[i] = (uint32_t)(t.tcol.size() - base);
            // rowslot: the chunk's columns as LDS byte offsets of their B rows (column x 128 B, < 64 KB
            // for KC <= 511), so the kernel adds its lane's 16-B piece and reads (no shift, no mask)
            if (rowslot)
                for (size_t k = base; k < t.tcol.size(); k++) t.tcol[k] = (uint16_t)(t.tcol[k] * RSB);
            while ((t.tcol.size() - base) % 8) { t.tcol.push_back(0); t.src.push_back(~0u); }
            GS_CHECK(t.tcol.size() - base <= t.seg_cap, "LDS tile segment exceeds its capacity");
            GS_CHECK(t.tcol.size() < 0xffffffffull, "LDS tile layout exceeds 32-bit offsets");
            t.seg_start.push_back((uint32_t)t.tcol.size());
        }
    }
    return true;
}

void merge_path_levels(const std::vector<uint64_t> &rows, uint64_t row_num, uint64_t work_size,
                       std::vector<uint64_t> &lr, std::vector<uint64_t> &ln) {
    std::vector<uint64_t> cnt(row_num, 0);
    for (uint64_t r : rows) cnt[r]++;
    std::vector<uint64_t> ends, crow;
    uint64_t acc = 0;
    for (uint64_t r = 0; r < row_num; r++)
        if (cnt[r]) {
            acc += cnt[r];
            ends.push_back(acc);
            crow.push_back(r);
        }
    lr.clear();
    ln.clear();
    uint64_t j = 0;
    for (uint64_t p = 0;; p += work_size) {
        while (j < ends.size() && ends[j] + j + 1 <= p) j++;
        if (j >= ends.size()) break;
        lr.push_back(crow[j]);
        ln.push_back(p - j);
    }
    ln.push_back(acc);
}

column_ranks column_order(const std::vector<uint64_t> &col, uint64_t K, uint64_t hot) {
    std::vector<uint32_t> deg(K, 0u), perm(K), rank(K);
    for (uint64_t c : col) deg[c]++;
    for (uint32_t i = 0; i < (uint32_t)K; i++) perm[i] = i;
    if (hot == 0 || hot >= K) {
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return deg[x] > deg[y]; });
    } else {  // MP_PERM_HOT: the `hot` densest columns first (by degree), the rest in their own order
        std::vector<uint32_t> byd(perm);
        std::nth_element(byd.begin(), byd.begin() + hot, byd.end(), [&](uint32_t x, uint32_t y) {
            return deg[x] != deg[y] ? deg[x] > deg[y] : x < y;
        });
        byd.resize(hot);
        std::sort(byd.begin(), byd.end(), [&](uint32_t x, uint32_t y) { return deg[x] != deg[y] ? deg[x] > deg[y] : x < y; });
        std::vector<uint8_t> is_hot(K, 0);
        for (uint32_t c : byd) is_hot[c] = 1;
        size_t w = 0;
        for (uint32_t c : byd) perm[w++] = c;
        for (uint32_t c = 0; c < (uint32_t)K; c++)
            if (!is_hot[c]) perm[w++] = c;
    }
    for (uint32_t i = 0; i < (uint32_t)K; i++) rank[perm[i]] = i;
    return {perm, rank};
}

col_parts split_col_parts(const std::vector<uint64_t> &rows, const std::vector<uint64_t> &col, uint64_t K, uint32_t P,
                          uint64_t hub) {
    const uint64_t nnz = col.size();
    const std::vector<uint32_t> perm = column_order(col, K, 0).perm;
    std::vector<uint32_t> pos(K);
    std::vector<uint64_t> base(P + 1, 0);
    if (hub > 0 && hub < K) {
        base[1] = hub;
        base[2] = K;
    } else {
        for (uint32_t x = 0; x < P; x++) base[x + 1] = base[x] + (K > x ? (K - x + P - 1) / P : 0);
    }
    std::vector<uint32_t> gather(K);
    for (uint32_t r = 0; r < (uint32_t)K; r++) {
        const uint32_t c = perm[r];
        const uint32_t q = hub > 0 && hub < K ? r : (uint32_t)(base[r % P] + r / P);
        pos[c] = q;
        gather[q] = c;
    }
    std::vector<uint8_t> part(nnz);
    std::vector<uint64_t> cnt(P, 0);
    for (uint64_t e = 0; e < nnz; e++) {
        const uint32_t q = pos[col[e]];
        uint32_t x = 0;
        while (q >= base[x + 1]) x++;
        part[e] = (uint8_t)x;
        cnt[x]++;
    }
    col_parts out;
    out.parts.resize(P);
    for (uint32_t x = 0; x < P; x++) {
        std::vector<uint64_t> &rx = out.parts[x].rows;
        std::vector<uint32_t> &cx = out.parts[x].cols, &sx = out.parts[x].src;
        rx.reserve(cnt[x]);
        cx.reserve(cnt[x]);
        sx.reserve(cnt[x]);
        for (uint64_t e = 0; e < nnz; e++)
            if (part[e] == x) {
                rx.push_back(rows[e]);
                cx.push_back(pos[col[e]]);
                sx.push_back((uint32_t)e);
            }
        GS_CHECK(!rx.empty(), "MP_COL_PARTS: a column partition without entries (fewer columns than partitions?)");
    }
    out.base = base;
    out.gather = gather;
    return out;
}

std::vector<uint32_t> bitmap_finalize_rows(const std::vector<uint64_t> &rows, const std::vector<uint64_t> &fn,
                                           const std::vector<uint32_t> &rp, uint64_t row_num, uint64_t M, uint64_t rb,
                                           uint64_t out_lo, uint64_t out_hi) {
    std::vector<uint8_t> fin(M, 0);
    for (uint64_t r = out_lo; r < out_hi; r++)
        if (r < rb || r - rb >= row_num || rp[r - rb] == rp[r - rb + 1]) fin[r] = 1;
    for (uint64_t i = 1; i + 1 < fn.size(); i++) {  // a BMT boundary strictly inside a row
        const uint64_t z = fn[i];
        if (z == 0 || z >= rows.size()) continue;
        if (rows[z] == rows[z - 1]) fin[rows[z] + rb] = 1;
    }
    std::vector<uint32_t> list;
    for (uint64_t r = 0; r < M; r++)
        if (fin[r]) list.push_back((uint32_t)r);
    return list;
}

}  // namespace gs
