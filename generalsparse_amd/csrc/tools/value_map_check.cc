// value_map_check -- the value-source map of k_mfma_ks plans (gs_plan_value_sources: host/device_layout.cc
// build_value_map, build_ks_tiles' source mode) as a stand-alone host program: no GPU, no Python.
// Built against the ASan/UBSan host objects by `make san_check` (Makefile), so the layout code runs
// instrumented.  For every layout variant of the default build (head steps, K ranges, window positions;
// f16 and bf16), with and without sort_operator: plan B's values gathered through plan A's map are plan
// B's value words, the maps agree, every entry has a slot; a duplicated coordinate is refused.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "generalsparse.h"

#define CK(x)                                                                    \
    do {                                                                         \
        if ((x) != GS_OK) {                                                      \
            std::fprintf(stderr, "%s: %s\n", #x, gs_last_error());               \
            return 2;                                                            \
        }                                                                        \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

struct coo {
    uint64_t M, K;
    std::vector<uint64_t> row, col;
};

// uneven rows (so that sort_operator permutes them), an entry at column 0 and at column K - 1
static coo make_pattern(uint64_t M, uint64_t K, bool even) {
    coo c{M, K, {}, {}};
    for (uint64_t r = 0; r < M; r++) {
        const uint32_t keep = even ? 0 : 10 + rnd() % 60;  // percent of a 30%-dense row
        for (uint64_t k = 0; k < K; k++) {
            const bool on = even ? (r + k) % 3 == 0  // (no row is empty: k == r % K)
                                 : (rnd() % 1000 < 3 * keep) || ((k == 0 || k == K - 1) && r % 40 == 39) || k == r % K;
            if (on) {
                c.row.push_back(r);
                c.col.push_back(k);
            }
        }
    }
    return c;
}

static std::vector<float> make_values(size_t n) {
    std::vector<float> v(n);
    for (float &x : v) x = ((int)(rnd() % 20001) - 10000) / 4099.0f;
    return v;
}

static int make_plan(const coo &c, const std::vector<float> &v, bool sort, gs_plan_t **out) {
    CK(gs_plan_create_from_coo(c.M, c.K, c.row.size(), c.row.data(), c.col.data(), v.data(), out));
    if (sort) CK(gs_plan_add_operator(*out, "sort_operator", nullptr, 0));
    CK(gs_plan_run_pipeline(*out, "block_total", 32, 40, 1));
    CK(gs_plan_compile(*out));
    return 0;
}

static int sources(gs_plan_t *p, int dtype, std::vector<uint32_t> &src, std::vector<uint16_t> &vals) {
    uint64_t n = 0;
    CK(gs_plan_value_sources(p, dtype, nullptr, 0, &n, nullptr));
    src.assign(n, 0);
    vals.assign(n, 0);
    CK(gs_plan_value_sources(p, dtype, src.data(), n, &n, vals.data()));
    return 0;
}

int main() {
    CK(gs_set_config_int("MFMA_MAX_FILL", 1ll << 30));  // these small patterns take the matrix-core layout
    long bad = 0, cases = 0;
    for (int shape = 0; shape < 3; shape++) {
        const coo c = shape == 0 ? make_pattern(131, 40, false) : shape == 1 ? make_pattern(131, 1176, false) : make_pattern(120, 1184, true);
        const std::vector<float> v1 = make_values(c.row.size()), v2 = make_values(c.row.size());
        for (int sort = 0; sort < 2; sort++) {
            gs_plan_t *A = nullptr, *B = nullptr;
            if (make_plan(c, v1, sort, &A) || make_plan(c, v2, sort, &B)) return 2;
            for (int dtype : {GS_F16, GS_BF16})
                for (int head = 0; head < 2; head++)
                    for (int wpos = 0; wpos < (dtype == GS_F16 ? 2 : 1); wpos++)
                        for (int split : {0, 1, 2}) {
                            CK(gs_set_config_int("KS_HEAD", head));
                            CK(gs_set_config_int("KS_WPOS", wpos));
                            CK(gs_set_config_int("KS_SPLIT", split));
                            std::vector<uint32_t> sa, sb;
                            std::vector<uint16_t> va, vb;
                            if (sources(A, dtype, sa, va) || sources(B, dtype, sb, vb)) return 2;
                            std::vector<uint16_t> w2(v2.size());
                            CK(gs_convert_values(v2.data(), v2.size(), dtype, w2.data()));
                            std::vector<uint32_t> seen(v2.size(), 0);
                            long b0 = bad;
                            bad += sa != sb || sa.size() != vb.size() || sa.size() % 8 != 0;
                            for (size_t k = 0; k < sa.size() && k < vb.size(); k++) {
                                if (sa[k] == 0xffffffffu) {
                                    bad += vb[k] != 0;
                                    continue;
                                }
                                if (sa[k] >= v2.size()) {
                                    bad++;
                                    continue;
                                }
                                bad += vb[k] != w2[sa[k]];
                                seen[sa[k]]++;
                            }
                            for (uint32_t n : seen) bad += wpos ? n < 1 : n != 1;
                            if (bad != b0)
                                std::fprintf(stderr, "shape %d sort %d dtype %d head %d wpos %d split %d: %ld mismatches\n", shape, sort,
                                             dtype, head, wpos, split, bad - b0);
                            cases++;
                        }
            gs_plan_free(A);
            gs_plan_free(B);
        }
        // a coordinate stored twice: refused
        coo d = c;
        d.row.insert(d.row.begin() + 7, d.row[7]);
        d.col.insert(d.col.begin() + 7, d.col[7]);
        std::vector<float> vd = make_values(d.row.size());
        gs_plan_t *D = nullptr;
        if (make_plan(d, vd, false, &D)) return 2;
        uint64_t n = 0;
        bad += gs_plan_value_sources(D, GS_F16, nullptr, 0, &n, nullptr) != GS_ERR || !std::strstr(gs_last_error(), "twice");
        gs_plan_free(D);
    }
    std::printf("value_map_check: %ld layouts, %ld mismatches\n", cases, bad);
    return bad ? 1 : 0;
}
