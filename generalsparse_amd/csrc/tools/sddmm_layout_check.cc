// sddmm_layout_check -- the pattern of a plan in canonical order and its device form
// (host/sddmm_layout.cc) on hand-written patterns, as a stand-alone host program: no GPU, no Python.
// Built against the ASan/UBSan host objects by `make san_check` (Makefile), so the layout code runs
// instrumented.  Every result is compared with a table written here.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../host/gs_core.hpp"
#include "../host/sddmm_layout.hpp"

using namespace gs;

static int g_bad = 0;

template <class A, class B>
static void expect_eq(const char *what, const std::vector<A> &got, const std::vector<B> &want) {
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < got.size(); i++) ok = (uint64_t)got[i] == (uint64_t)want[i];
    if (!ok) {
        std::printf("FAIL %s\n", what);
        g_bad++;
    }
}

static void expect_val(const char *what, const std::vector<float> &got, const std::vector<float> &want) {
    bool ok = got.size() == want.size();
    for (size_t i = 0; ok && i < got.size(); i++) ok = got[i] == want[i];
    if (!ok) {
        std::printf("FAIL %s\n", what);
        g_bad++;
    }
}

template <class F>
static void expect_throw(const char *what, F &&f) {
    try {
        f();
    } catch (const gs_error &) {
        return;
    }
    std::printf("FAIL %s: accepted\n", what);
    g_bad++;
}

int main() {
    // 1. row-major input (a dense weight's non-zeros): copied.  Row 1 is empty, row 2 full (K = 4)
    {
        const std::vector<uint64_t> row = {0, 0, 2, 2, 2, 2, 3}, col = {1, 3, 0, 1, 2, 3, 2};
        const std::vector<float> val = {1, 2, 3, 4, 5, 6, 7};
        const sddmm_pattern p = build_sddmm_pattern(4, row.size(), row.data(), col.data(), val.data());
        expect_eq("row-major rp", p.rp, std::vector<uint32_t>{0, 2, 2, 6, 7});
        expect_eq("row-major col", p.col, col);
        expect_val("row-major val", p.val, val);
        expect_eq("row-major u16", sddmm_cols_u16(p), col);
    }
    // 2. unsorted columns inside rows, one coordinate stored three times ((1, 4): input order 20, 21, 22)
    {
        const std::vector<uint64_t> row = {0, 0, 0, 1, 1, 1, 1, 1}, col = {5, 0, 3, 4, 9, 4, 1, 4};
        const std::vector<double> val = {10, 11, 12, 20, 30, 21, 40, 22};
        const sddmm_pattern p = build_sddmm_pattern(3, row.size(), row.data(), col.data(), val.data());
        expect_eq("unsorted rp", p.rp, std::vector<uint32_t>{0, 3, 8, 8});
        expect_eq("unsorted col", p.col, std::vector<uint32_t>{0, 3, 5, 1, 4, 4, 4, 9});
        expect_val("unsorted val", p.val, {11, 12, 10, 40, 20, 21, 22, 30});
    }
    // 3. rows in a sorted plan's order (longest first), mapped back through orig_row; the entries of the
    // stored rows come in any order
    {
        const std::vector<uint64_t> orig = {2, 0, 3, 1};  // stored row -> original row
        const std::vector<uint64_t> row = {1, 0, 0, 2, 0, 1}, col = {7, 2, 1, 0, 6, 3};
        const std::vector<float> val = {1, 2, 3, 4, 5, 6};
        const sddmm_pattern p = build_sddmm_pattern(4, row.size(), row.data(), col.data(), val.data(), orig.data(), orig.size());
        expect_eq("sorted rp", p.rp, std::vector<uint32_t>{0, 2, 2, 5, 6});
        expect_eq("sorted col", p.col, std::vector<uint32_t>{3, 7, 1, 2, 6, 0});
        expect_val("sorted val", p.val, {6, 1, 3, 2, 5, 4});
        expect_throw("stored row without an original row",
                     [&] { build_sddmm_pattern(4, row.size(), row.data(), col.data(), val.data(), orig.data(), 2); });
    }
    // 4. K on both sides of 65536: the last column 65535 fits u16, 65536 does not
    {
        const std::vector<uint64_t> row = {0, 1}, lo = {65535, 0}, hi = {65536, 0};
        const std::vector<float> val = {1, 2};
        const sddmm_pattern a = build_sddmm_pattern(2, 2, row.data(), lo.data(), val.data());
        const sddmm_pattern b = build_sddmm_pattern(2, 2, row.data(), hi.data(), val.data());
        if (sddmm_col_bytes(65536) != 2 || sddmm_col_bytes(65537) != 4) {
            std::printf("FAIL col bytes\n");
            g_bad++;
        }
        expect_eq("K = 65536 u16", sddmm_cols_u16(a), lo);
        expect_eq("K = 65537 u32", b.col, hi);
        expect_throw("K = 65537 as u16", [&] { sddmm_cols_u16(b); });
    }
    // 5. refusals: a row outside the matrix, a column outside 32 bits
    {
        const std::vector<uint64_t> row = {0, 5}, col = {0, 0}, wide = {0, 1ull << 32};
        const std::vector<float> val = {1, 2};
        expect_throw("row outside", [&] { build_sddmm_pattern(5, 2, row.data(), col.data(), val.data()); });
        expect_throw("column outside", [&] { build_sddmm_pattern(6, 2, row.data(), wide.data(), val.data()); });
    }
    if (g_bad) return 1;
    std::printf("sddmm_layout_check: ok\n");
    return 0;
}
