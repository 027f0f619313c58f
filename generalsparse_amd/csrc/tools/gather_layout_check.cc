// gather_layout_check -- the host-side layouts of the LDS-staged, merge-path and bitmap families
// (host/gather_layout.cc) on matrices from a fixed LCG, as a stand-alone host program: no GPU, no
// Python.  Built against the ASan/UBSan host objects by `make san_check` (Makefile), so the layout
// code runs instrumented; `make build/gather_layout_check` links the plain objects.
// Every output array is also hashed (FNV-1a-64) and compared with kExpect: the values the code
// printed when it had just been moved, unedited, out of kernels/device_plan.hip, except tcol of the
// LDS cases and src of their fp32 ones, printed again when a row's padding became copies of the row's
// last column of the chunk (the invariants below held).  `--print` prints the hashes as an
// initializer instead of comparing them; do that only when every invariant passes.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../host/gather_layout.hpp"

using namespace gs;

static const uint64_t kExpect[] = {
    0x6c2fb0e69354de86ull,  // fp16 N=32 20x2 scalars
    0xdaa04f15cca56916ull,  // fp16 N=32 20x2 seg_start
    0xd2304bf5d1073431ull,  // fp16 N=32 20x2 seg_row_off
    0x95a3dd3daf2c783aull,  // fp16 N=32 20x2 tcol
    0xc0c05cec53050638ull,  // fp16 N=32 20x2 src
    0x33648a8904d2b95eull,  // fp32 N=32 pair_banks 20x2 scalars
    0xed852e7d3e96cdd3ull,  // fp32 N=32 pair_banks 20x2 seg_start
    0xf8aa0665022883f5ull,  // fp32 N=32 pair_banks 20x2 seg_row_off
    0x395711456277b894ull,  // fp32 N=32 pair_banks 20x2 tcol
    0x883aa8ecf9aabee5ull,  // fp32 N=32 pair_banks 20x2 src
    0x4cdcfdca926a18b0ull,  // fp32 N=32 pair_banks 16x4 scalars
    0x28170f11f6504e52ull,  // fp32 N=32 pair_banks 16x4 seg_start
    0x0e56c4dfc28f1315ull,  // fp32 N=32 pair_banks 16x4 seg_row_off
    0xd86757127db70c5full,  // fp32 N=32 pair_banks 16x4 tcol
    0x5d317ad6cd9bb50dull,  // fp32 N=32 pair_banks 16x4 src
    0x3c7740e7b62bc870ull,  // fp32 N=32 dma 20x4 scalars
    0xa56fe196e43f0475ull,  // fp32 N=32 dma 20x4 seg_start
    0x63a27f4b8f2f621dull,  // fp32 N=32 dma 20x4 seg_row_off
    0x540d9f93dd795425ull,  // fp32 N=32 dma 20x4 tcol
    0x4aba1fc8b5cb9fd1ull,  // fp32 N=32 dma 20x4 src
    0x5ecd8e2a1bbe70b3ull,  // fp32 N=32 rowslot 20x5 scalars
    0xd3ca24b00cd7e137ull,  // fp32 N=32 rowslot 20x5 seg_start
    0xbbf8167af7bb34e1ull,  // fp32 N=32 rowslot 20x5 seg_row_off
    0x9695c94c957d2db9ull,  // fp32 N=32 rowslot 20x5 tcol
    0x474359b18c892bf5ull,  // fp32 N=32 rowslot 20x5 src
    0xed32955309ae8cfcull,  // fp32 N=32 rowslot 24x6 scalars
    0x8b02dcf1d844cb60ull,  // fp32 N=32 rowslot 24x6 seg_start
    0xcd52ba2c22d5aa21ull,  // fp32 N=32 rowslot 24x6 seg_row_off
    0x03577aabfcc0a3a6ull,  // fp32 N=32 rowslot 24x6 tcol
    0x8ed9c923c44bd921ull,  // fp32 N=32 rowslot 24x6 src
    0xdd907d9c06931951ull,  // fp32 N=32 rowslot 32x8 scalars
    0x9bd89bc5b1b160c9ull,  // fp32 N=32 rowslot 32x8 seg_start
    0xac58413948778285ull,  // fp32 N=32 rowslot 32x8 seg_row_off
    0x32b063bf7df3c986ull,  // fp32 N=32 rowslot 32x8 tcol
    0x0f444a242a0da994ull,  // fp32 N=32 rowslot 32x8 src
    0xecbf805e1c9758e6ull,  // fp32 N=32 want=3 scalars
    0x5330298ecc181bd6ull,  // fp32 N=32 want=3 seg_start
    0x473da6e16b06c155ull,  // fp32 N=32 want=3 seg_row_off
    0x38c73947fdfbca29ull,  // fp32 N=32 want=3 tcol
    0x46a5b4cdd7968008ull,  // fp32 N=32 want=3 src
    0x1fa9cc26d8801edaull,  // fp32 N=32 rowslot want=3 scalars
    0xe2b720f147518f4full,  // fp32 N=32 rowslot want=3 seg_start
    0xc37c98cd23588265ull,  // fp32 N=32 rowslot want=3 seg_row_off
    0x59c20b9abdf2ed8bull,  // fp32 N=32 rowslot want=3 tcol
    0xdcd0cfe64f88bafdull,  // fp32 N=32 rowslot want=3 src
    0xf85ee3923ea3c245ull,  // column_order hot=0 perm
    0x024bd0e37d1f2ec5ull,  // column_order hot=0 rank
    0x24edec81a2df85f5ull,  // column_order hot=17 perm
    0x25554c5ad22067f5ull,  // column_order hot=17 rank
    0xf85ee3923ea3c245ull,  // column_order hot=K perm
    0x024bd0e37d1f2ec5ull,  // column_order hot=K rank
    0x50c28adede72f637ull,  // col parts P=3 rows
    0x8476d5cbb5e1e6aeull,  // col parts P=3 cols
    0x21021421e24625ebull,  // col parts P=3 src
    0x6611c4d38febdb22ull,  // col parts P=3 rows
    0xe6a4227c96b6c519ull,  // col parts P=3 cols
    0x2af2bec168af68cdull,  // col parts P=3 src
    0x5d4fe2f8444744e0ull,  // col parts P=3 rows
    0x55bbe030f13e8de2ull,  // col parts P=3 cols
    0x8bf18c7d674b894aull,  // col parts P=3 src
    0xea16bd9dec8a8f08ull,  // col parts P=3 base
    0xf7350fecfa7cfb25ull,  // col parts P=3 gather
    0xb6591ef6a0190268ull,  // col parts P=2 hub=10 rows
    0xe16cd35bf72be688ull,  // col parts P=2 hub=10 cols
    0xc6fae5e05338b98full,  // col parts P=2 hub=10 src
    0x4abbfc5bc64efef8ull,  // col parts P=2 hub=10 rows
    0x2b9e5a177ae40e64ull,  // col parts P=2 hub=10 cols
    0x9626708d9cd6ddbeull,  // col parts P=2 hub=10 src
    0xe1371f1cabc23c47ull,  // col parts P=2 hub=10 base
    0xf85ee3923ea3c245ull,  // col parts P=2 hub=10 gather
    0x65d8b900f4176f3cull,  // col parts P=2 rows
    0x5457ddb755a9b2faull,  // col parts P=2 cols
    0xa737aec5e6a3eecfull,  // col parts P=2 src
    0x622ab25f3c7a6eccull,  // col parts P=2 rows
    0x6aaade274026bf34ull,  // col parts P=2 cols
    0x3f70697aa25de17eull,  // col parts P=2 src
    0x21d8213475477229ull,  // col parts P=2 base
    0xd29fd4aaf3d79db5ull,  // col parts P=2 gather
    0x898b15eb1a8037a7ull,  // merge_path_levels ws=7 level rows
    0x1bf9b2989d9e6880ull,  // merge_path_levels ws=7 level nonzeros
    0x32560122c54b3d14ull,  // merge_path_levels ws=1 level rows
    0xd3cdcce55d4a318dull,  // merge_path_levels ws=1 level nonzeros
    0x02a1ae15ed95ba14ull,  // merge_path_levels ws=64 level rows
    0xeddef0abef5bdeceull,  // merge_path_levels ws=64 level nonzeros
    0x2a25b28b1c1c6487ull,  // bitmap rows finalize rows
    0x7cc79a10c6209da1ull,  // bitmap rows row masks
    0xb27e99aba141bc36ull,  // bitmap rows, sub-matrix finalize rows
    0xe8b15acf9791e3adull,  // bitmap rows, sub-matrix row masks
    0x783059749349a729ull,  // edge fp16 N=8 20x2 want=1 scalars
    0xfc82fec943079b84ull,  // edge fp16 N=8 20x2 want=1 seg_start
    0xfa301640a1313de9ull,  // edge fp16 N=8 20x2 want=1 seg_row_off
    0x9d39a525be61c6ccull,  // edge fp16 N=8 20x2 want=1 tcol
    0xf3e2c60f026f2e79ull,  // edge fp16 N=8 20x2 want=1 src
    0x783059749349a729ull,  // edge fp16 N=8 20x2 want=2 scalars
    0xfc82fec943079b84ull,  // edge fp16 N=8 20x2 want=2 seg_start
    0xfa301640a1313de9ull,  // edge fp16 N=8 20x2 want=2 seg_row_off
    0x9d39a525be61c6ccull,  // edge fp16 N=8 20x2 want=2 tcol
    0xf3e2c60f026f2e79ull,  // edge fp16 N=8 20x2 want=2 src
    0x7a703c8b160e685bull,  // edge fp16 N=8 20x2 want=auto scalars
    0x0a5d4b599198d33dull,  // edge fp16 N=8 20x2 want=auto seg_start
    0xa274f047b9bd7ebdull,  // edge fp16 N=8 20x2 want=auto seg_row_off
    0x6c80b6fcf34e4089ull,  // edge fp16 N=8 20x2 want=auto tcol
    0x77222d9865adec29ull,  // edge fp16 N=8 20x2 want=auto src
    0x071d3dbd65fd335eull,  // edge fp32 N=32 pair_banks 20x2 want=1 scalars
    0xfc82fec943079b84ull,  // edge fp32 N=32 pair_banks 20x2 want=1 seg_start
    0xfa301640a1313de9ull,  // edge fp32 N=32 pair_banks 20x2 want=1 seg_row_off
    0xcd390d0afcd7d4b4ull,  // edge fp32 N=32 pair_banks 20x2 want=1 tcol
    0x333df5dbfe757981ull,  // edge fp32 N=32 pair_banks 20x2 want=1 src
    0x071d3dbd65fd335eull,  // edge fp32 N=32 pair_banks 20x2 want=2 scalars
    0xfc82fec943079b84ull,  // edge fp32 N=32 pair_banks 20x2 want=2 seg_start
    0xfa301640a1313de9ull,  // edge fp32 N=32 pair_banks 20x2 want=2 seg_row_off
    0xcd390d0afcd7d4b4ull,  // edge fp32 N=32 pair_banks 20x2 want=2 tcol
    0x333df5dbfe757981ull,  // edge fp32 N=32 pair_banks 20x2 want=2 src
    0xefdc22e3ecffcbaaull,  // edge fp32 N=32 pair_banks 20x2 want=auto scalars
    0x0a5d4b599198d33dull,  // edge fp32 N=32 pair_banks 20x2 want=auto seg_start
    0xa274f047b9bd7ebdull,  // edge fp32 N=32 pair_banks 20x2 want=auto seg_row_off
    0x63c2f9cf65b6d8d9ull,  // edge fp32 N=32 pair_banks 20x2 want=auto tcol
    0x95ccabeff7e270edull,  // edge fp32 N=32 pair_banks 20x2 want=auto src
    0xa46dd4b38ee6eb0cull,  // edge fp32 N=32 dma 20x2 want=1 scalars
    0xfc82fec943079b84ull,  // edge fp32 N=32 dma 20x2 want=1 seg_start
    0xfa301640a1313de9ull,  // edge fp32 N=32 dma 20x2 want=1 seg_row_off
    0xcd390d0afcd7d4b4ull,  // edge fp32 N=32 dma 20x2 want=1 tcol
    0x333df5dbfe757981ull,  // edge fp32 N=32 dma 20x2 want=1 src
    0xa46dd4b38ee6eb0cull,  // edge fp32 N=32 dma 20x2 want=2 scalars
    0xfc82fec943079b84ull,  // edge fp32 N=32 dma 20x2 want=2 seg_start
    0xfa301640a1313de9ull,  // edge fp32 N=32 dma 20x2 want=2 seg_row_off
    0xcd390d0afcd7d4b4ull,  // edge fp32 N=32 dma 20x2 want=2 tcol
    0x333df5dbfe757981ull,  // edge fp32 N=32 dma 20x2 want=2 src
    0x18f3356bb1060f3dull,  // edge fp32 N=32 dma 20x2 want=auto scalars
    0x0a5d4b599198d33dull,  // edge fp32 N=32 dma 20x2 want=auto seg_start
    0xa274f047b9bd7ebdull,  // edge fp32 N=32 dma 20x2 want=auto seg_row_off
    0x63c2f9cf65b6d8d9ull,  // edge fp32 N=32 dma 20x2 want=auto tcol
    0x95ccabeff7e270edull,  // edge fp32 N=32 dma 20x2 want=auto src
    0xe75d47d98cb8a0a2ull,  // edge fp32 N=32 rowslot 40x5 want=1 scalars
    0x134b450ae1e4e95dull,  // edge fp32 N=32 rowslot 40x5 want=1 seg_start
    0x62bcca7e2eff7a7eull,  // edge fp32 N=32 rowslot 40x5 want=1 seg_row_off
    0x5eadfab72be43d15ull,  // edge fp32 N=32 rowslot 40x5 want=1 tcol
    0x95b6871224daae71ull,  // edge fp32 N=32 rowslot 40x5 want=1 src
    0xe75d47d98cb8a0a2ull,  // edge fp32 N=32 rowslot 40x5 want=2 scalars
    0x134b450ae1e4e95dull,  // edge fp32 N=32 rowslot 40x5 want=2 seg_start
    0x62bcca7e2eff7a7eull,  // edge fp32 N=32 rowslot 40x5 want=2 seg_row_off
    0x5eadfab72be43d15ull,  // edge fp32 N=32 rowslot 40x5 want=2 tcol
    0x95b6871224daae71ull,  // edge fp32 N=32 rowslot 40x5 want=2 src
    0x242715fe8ac9d06aull,  // edge fp32 N=32 rowslot 40x5 want=auto scalars
    0xd11f4272cdc9a991ull,  // edge fp32 N=32 rowslot 40x5 want=auto seg_start
    0x90bca010ffaebd52ull,  // edge fp32 N=32 rowslot 40x5 want=auto seg_row_off
    0xa3fbed9919d73a67ull,  // edge fp32 N=32 rowslot 40x5 want=auto tcol
    0x54ee7c4ed81706e9ull,  // edge fp32 N=32 rowslot 40x5 want=auto src
    0x0b1ac642e0b51857ull,  // edge fp32 N=32 rowslot 64x8 want=1 scalars
    0xee1c0a01ca124d09ull,  // edge fp32 N=32 rowslot 64x8 want=1 seg_start
    0xf6a8c2b414fb3810ull,  // edge fp32 N=32 rowslot 64x8 want=1 seg_row_off
    0x3892f914e73cc495ull,  // edge fp32 N=32 rowslot 64x8 want=1 tcol
    0x9bc6193a1960b575ull,  // edge fp32 N=32 rowslot 64x8 want=1 src
    0x0b1ac642e0b51857ull,  // edge fp32 N=32 rowslot 64x8 want=2 scalars
    0xee1c0a01ca124d09ull,  // edge fp32 N=32 rowslot 64x8 want=2 seg_start
    0xf6a8c2b414fb3810ull,  // edge fp32 N=32 rowslot 64x8 want=2 seg_row_off
    0x3892f914e73cc495ull,  // edge fp32 N=32 rowslot 64x8 want=2 tcol
    0x9bc6193a1960b575ull,  // edge fp32 N=32 rowslot 64x8 want=2 src
    0x66ffcd642a5d939dull,  // edge fp32 N=32 rowslot 64x8 want=auto scalars
    0x1eb52246dea82e81ull,  // edge fp32 N=32 rowslot 64x8 want=auto seg_start
    0x6d46d7b2d50e869dull,  // edge fp32 N=32 rowslot 64x8 want=auto seg_row_off
    0x74bc3c70045ddbcfull,  // edge fp32 N=32 rowslot 64x8 want=auto tcol
    0x10638f5d9da020f9ull,  // edge fp32 N=32 rowslot 64x8 want=auto src
};

static long g_bad = 0;
static bool g_print = false;
static size_t g_hash_at = 0;

#define EXPECT(c, ...)                                     \
    do {                                                   \
        if (!(c) && ++g_bad < 20) {                        \
            std::fprintf(stderr, "%s: ", g_case.c_str());  \
            std::fprintf(stderr, __VA_ARGS__);             \
            std::fprintf(stderr, " (%s)\n", #c);           \
        }                                                  \
    } while (0)
static std::string g_case;

static uint64_t g_lcg = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t n) {
    g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_lcg >> 33) % n);
}

template <class T>
static void hash_array(const char *what, const std::vector<T> &v) {
    uint64_t h = 0xcbf29ce484222325ull;
    const unsigned char *b = reinterpret_cast<const unsigned char *>(v.data());
    for (size_t i = 0; i < v.size() * sizeof(T); i++) h = (h ^ b[i]) * 0x100000001b3ull;
    const size_t at = g_hash_at++;
    if (g_print) {
        std::printf("    0x%016llxull,  // %s %s\n", (unsigned long long)h, g_case.c_str(), what);
        return;
    }
    const size_t n = sizeof(kExpect) / sizeof(kExpect[0]);
    EXPECT(at < n && kExpect[at] == h, "%s: hash %016llx differs from the moved code's", what, (unsigned long long)h);
}

struct coo {
    uint64_t M = 0, K = 0;
    std::vector<uint64_t> row, col;  // row-sorted, columns ascending within a row
    std::vector<uint32_t> rp;
};

// row 0: 60 entries in columns 0..59 (one chunk holds them all: chunks are >= 64 columns), row 1:
// even columns only, rows 2, 3 and every seventh row empty, the others ~`mean` random columns
static coo make_matrix(uint64_t M, uint64_t K, uint32_t mean) {
    coo a;
    a.M = M;
    a.K = K;
    for (uint64_t r = 0; r < M; r++) {
        std::vector<uint64_t> c;
        if (r == 0) {
            for (uint64_t x = 0; x < 60; x++) c.push_back(x);
        } else if (r == 1) {
            for (uint64_t x = 0; x < K; x += 2)
                if (rnd(4) == 0) c.push_back(x);
        } else if (r == 2 || r == 3 || (r % 7 == 6 && r + 1 < M)) {
        } else {
            const uint32_t n = 1 + rnd(2 * mean);
            for (uint32_t i = 0; i < n; i++) c.push_back(rnd((uint32_t)K));
            std::sort(c.begin(), c.end());
            c.erase(std::unique(c.begin(), c.end()), c.end());
        }
        for (uint64_t x : c) {
            a.row.push_back(r);
            a.col.push_back(x);
        }
    }
    a.rp = csr_row_ptr(a.row, M);
    return a;
}

// The size of the GPU tests' edge pattern (tests/test_gpu_edges.py: 131 x 203), rows of 0..256 entries, from
// an LCG of its own (the cases above keep their matrices): rows 0, 5, 37, 38, 90 and the three
// trailing rows empty, row 20 with every column and 53 of them twice (256 entries), row 2 with 40 even
// columns, rows 10..13 with 1, 7, 8 and 9 entries, rows 1 and 127 with columns 0 and K - 1, the
// others 2..20 random columns
static coo make_edge() {
    const uint64_t M = 131, K = 203;
    uint64_t lcg = 0x2545f4914f6cdd1dull;
    auto r32 = [&](uint32_t n) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)((lcg >> 33) % n);
    };
    coo a;
    a.M = M;
    a.K = K;
    for (uint64_t r = 0; r < M; r++) {
        std::vector<uint64_t> c;
        const bool empty = r == 0 || r == 5 || r == 37 || r == 38 || r == 90 || r >= 128;
        if (r == 20) {
            for (uint64_t x = 0; x < K; x++) c.push_back(x);
            for (uint64_t x = 0; x < 53; x++) c.push_back((x * 23 + 3) % K);  // 23 and 203 are coprime: 53 distinct
            std::sort(c.begin(), c.end());
        } else if (r == 2) {
            for (uint64_t x = 0; x < 40; x++) c.push_back(4 * x + 2 * (x % 2));
        } else if (!empty) {
            const uint32_t n = r >= 10 && r <= 13 ? (r == 10 ? 1u : (uint32_t)(r - 4)) : 2 + r32(19);
            for (uint32_t i = 0; i < n; i++) c.push_back(r32((uint32_t)K));
            if (r == 1 || r == 127) {
                c.push_back(0);
                c.push_back(K - 1);
            }
            std::sort(c.begin(), c.end());
            c.erase(std::unique(c.begin(), c.end()), c.end());
        }
        for (uint64_t x : c) {
            a.row.push_back(r);
            a.col.push_back(x);
        }
    }
    a.rp = csr_row_ptr(a.row, M);
    return a;
}

// a small integer value per CSR entry, never 0 (the value-level check of lds_case)
static int64_t value_of(uint64_t e) {
    const int64_t v = (int64_t)(e * 2654435761ull % 6) - 3;  // -3 .. 2
    return v >= 0 ? v + 1 : v;                              // -3 .. -1, 1 .. 3
}

struct blocks {
    std::vector<uint64_t> tb_rows, tb_bmw, bmw_rows;
};

// BMTBs of tbr rows in BMWs of bwr rows (the last of each may be short)
static blocks make_blocks(uint64_t M, uint64_t tbr, uint64_t bwr) {
    blocks b;
    for (uint64_t r0 = 0; r0 < M; r0 += tbr) {
        b.tb_rows.push_back(r0);
        b.tb_bmw.push_back(b.bmw_rows.size());
        for (uint64_t r = r0; r < std::min(M, r0 + tbr); r += bwr) b.bmw_rows.push_back(r);
    }
    b.tb_rows.push_back(M);
    b.tb_bmw.push_back(b.bmw_rows.size());
    b.bmw_rows.push_back(M);
    return b;
}

// edge: the matrix of make_edge() instead of make_matrix(M, K, 8), with the chunking the case pins
// (KC columns in nc chunks) instead of the three or more chunks the small budgets of the other cases force
static void lds_case(const char *name, uint64_t M, uint64_t K, uint64_t tbr, uint64_t bwr, uint32_t N, uint32_t vbytes,
                     size_t budget, bool dma, uint64_t want, const coo *edge = nullptr, uint32_t pin_kc = 0,
                     uint32_t pin_nc = 0) {
    g_case = name;
    const coo a = edge ? *edge : make_matrix(M, K, 8);
    const blocks b = make_blocks(M, tbr, bwr);
    EXPECT(M % tbr != 0, "the last BMTB must be short");
    lds_tiles t;
    std::string why;
    const bool ok = build_lds_tiles(b.tb_rows, b.tb_bmw, b.bmw_rows, a.rp, a.col, K, N, vbytes, budget, t, why, dma, want);
    EXPECT(ok, "refused: %s", why.c_str());
    if (!ok) return;
    const uint64_t nb = b.tb_rows.size() - 1, nnz = a.col.size();
    const bool rowslot = t.maxr == 8, pair_banks = vbytes == 4 && N == 32 && !rowslot;
    EXPECT((uint64_t)t.KC * t.nc >= K && t.KC % 8 == 0, "KC %u x %u chunks", t.KC, t.nc);
    if (edge) EXPECT(t.KC == pin_kc && t.nc == pin_nc, "KC %u x %u chunks, pinned %u x %u", t.KC, t.nc, pin_kc, pin_nc);
    else EXPECT(t.nc >= 3, "%u chunks", t.nc);
    EXPECT(t.lds_bytes <= budget, "%zu B of LDS over the budget", t.lds_bytes);
    EXPECT(t.rpw_max == tbr && t.waves == (tbr + bwr - 1) / bwr, "rpw_max %u, waves %u", t.rpw_max, t.waves);
    EXPECT(t.seg_start.size() == nb * t.nc + 1 && t.seg_start[0] == 0 && t.seg_start.back() == t.tcol.size() &&
               t.src.size() == t.tcol.size() && t.seg_row_off.size() == nb * t.nc * (t.rpw_max + 1),
           "array sizes");
    std::vector<uint32_t> seen(nnz, 0);
    // the rows' sums of value x (column + 1) as the kernels walk the tiles: row i of BMTB g over its
    // [off[i], off[i+1]) of every chunk, a padding entry at value 0
    std::vector<int64_t> walked(M, 0);
    bool big_row = false, even_row = false;
    for (uint64_t g = 0; g < nb; g++)
        for (uint32_t j = 0; j < t.nc; j++) {
            const uint32_t s0 = t.seg_start[g * t.nc + j], s1 = t.seg_start[g * t.nc + j + 1];
            const uint32_t *off = &t.seg_row_off[(g * t.nc + j) * (t.rpw_max + 1)];
            const uint64_t r0 = b.tb_rows[g], nr = b.tb_rows[g + 1] - r0;
            EXPECT(s1 >= s0 && (s1 - s0) % 8 == 0 && s1 - s0 <= t.seg_cap, "segment of %u entries, cap %u", s1 - s0, t.seg_cap);
            EXPECT(off[0] == 0 && (off[t.rpw_max] + 7) / 8 * 8 == s1 - s0, "row offsets against the segment's length");
            for (uint64_t i = 0; i < t.rpw_max; i++) {
                EXPECT(off[i + 1] >= off[i] && (off[i + 1] - off[i]) % 4 == 0, "row segment %u..%u", off[i], off[i + 1]);
                if (i >= nr) EXPECT(off[i + 1] == off[i], "rows past a short BMTB hold entries");
            }
            for (uint32_t k = s0 + off[t.rpw_max]; k < s1; k++) EXPECT(t.tcol[k] == 0 && t.src[k] == ~0u, "segment padding");
            for (uint64_t i = 0; i < nr; i++) {
                const uint64_t r = r0 + i;
                const uint32_t k0 = s0 + off[i], k1 = s0 + off[i + 1];
                // the row's CSR entries of this chunk: a contiguous run (columns ascend)
                uint64_t e0 = a.rp[r], e1;
                while (e0 < a.rp[r + 1] && a.col[e0] < (uint64_t)j * t.KC) e0++;
                for (e1 = e0; e1 < a.rp[r + 1] && a.col[e1] < (uint64_t)(j + 1) * t.KC; e1++) {}
                std::vector<uint32_t> got;
                std::vector<unsigned> par;  // column parity per entry, padding included
                std::vector<uint32_t> padc;  // the padding entries' columns
                bool all_even = true;
                // a row without an entry in the chunk gets no padding
                if (e1 == e0) EXPECT(k1 == k0, "row %llu chunk %u: %u entries of padding alone", (unsigned long long)r, j, k1 - k0);
                for (uint32_t k = k0; k < k1; k++) {
                    uint32_t c = t.tcol[k];
                    if (rowslot) {
                        EXPECT(c % t.RSB == 0, "rowslot column is not a byte offset of a B row");
                        c /= t.RSB;
                    }
                    par.push_back(c & 1u);
                    if (t.src[k] == ~0u) {
                        padc.push_back(c);
                        continue;
                    }
                    if (t.src[k] < nnz) walked[r] += value_of(t.src[k]) * (int64_t)((uint64_t)j * t.KC + c + 1);
                    EXPECT(t.src[k] < nnz, "source entry out of range");
                    if (t.src[k] >= nnz) continue;
                    seen[t.src[k]]++;
                    got.push_back(t.src[k]);
                    EXPECT(a.col[t.src[k]] == (uint64_t)j * t.KC + c, "column of entry %u", t.src[k]);
                    all_even &= !(c & 1u);
                }
                // padding (value 0) carries a column that an entry of this row in this chunk carries: 0 x a
                // non-finite B value then stays in a row that holds the column
                for (uint32_t c : padc) {
                    bool held = false;
                    for (uint64_t e = e0; e < e1; e++) held |= a.col[e] == (uint64_t)j * t.KC + c;
                    EXPECT(held, "row %llu chunk %u: padding with column %u, which the row does not hold there",
                           (unsigned long long)r, j, c);
                }
                EXPECT(padc.size() < 4, "row %llu chunk %u: %zu padding entries", (unsigned long long)r, j, padc.size());
                std::sort(got.begin(), got.end());
                EXPECT(got.size() == e1 - e0 && (got.empty() || (got.front() == e0 && got.back() == e1 - 1)),
                       "row %llu chunk %u: entries are not the row's CSR entries", (unsigned long long)r, j);
                big_row |= got.size() > 32;
                even_row |= got.size() > 1 && all_even;
                if (pair_banks) {
                    static const int pairs[4][2] = {{0, 3}, {1, 2}, {4, 7}, {5, 6}};
                    for (size_t b0 = 0; b0 < par.size(); b0 += 32) {
                        const size_t n = std::min<size_t>(32, par.size() - b0);
                        int same = -1;  // parity of the first pair that had one parity twice
                        for (int q = 0; q < 4; q++)
                            for (const auto &pr : pairs) {
                                const size_t pa = (size_t)pr[0] * 4 + q, pb = (size_t)pr[1] * 4 + q;
                                if (pa >= n || pb >= n) continue;
                                const unsigned x = par[b0 + pa], y = par[b0 + pb];
                                if (same >= 0) EXPECT(x == (unsigned)same && y == (unsigned)same, "pair_banks: a pair after the kinds ran out");
                                else if (x == y) same = (int)x;
                            }
                    }
                }
                if (rowslot) {
                    uint64_t w = b.tb_bmw[g];
                    while (b.bmw_rows[w + 1] <= r) w++;
                    const unsigned ph = ((r - b.bmw_rows[w]) & 2u) ? 1u : 0u;
                    int rest = -1;  // parity of the first entry that missed its slot's parity
                    for (size_t k = 0; k < par.size(); k++) {
                        if (rest >= 0) EXPECT(par[k] == (unsigned)rest, "rowslot: an entry after one kind ran out");
                        else if (par[k] != ((k + ph) & 1u)) rest = (int)par[k];
                    }
                }
            }
        }
    for (uint64_t e = 0; e < nnz; e++) EXPECT(seen[e] == 1, "entry %llu placed %u times", (unsigned long long)e, seen[e]);
    for (uint64_t r = 0; r < M; r++) {
        int64_t sum = 0;
        for (uint64_t e = a.rp[r]; e < a.rp[r + 1]; e++) sum += value_of(e) * (int64_t)(a.col[e] + 1);
        EXPECT(walked[r] == sum, "row %llu: the tiles sum value x (column + 1) to %lld, the CSR to %lld", (unsigned long long)r,
               (long long)walked[r], (long long)sum);
    }
    EXPECT(big_row && even_row, "the matrix lacks a > 32-entry row segment or an all-even one");
    hash_array("scalars", std::vector<uint64_t>{t.KC, t.nc, t.RSB, t.rpw_max, t.seg_cap, t.waves, t.maxr, t.lds_bytes});
    hash_array("seg_start", t.seg_start);
    hash_array("seg_row_off", t.seg_row_off);
    hash_array("tcol", t.tcol);
    hash_array("src", t.src);
}

static void refusal(const char *name, uint64_t tbr, uint64_t bwr, uint32_t N, uint32_t vbytes, size_t budget, bool dma,
                    const char *text) {
    g_case = name;
    const coo a = make_matrix(50, 500, 8);
    const blocks b = make_blocks(50, tbr, bwr);
    lds_tiles t;
    std::string why;
    const bool ok = build_lds_tiles(b.tb_rows, b.tb_bmw, b.bmw_rows, a.rp, a.col, 500, N, vbytes, budget, t, why, dma, 1);
    EXPECT(!ok && why == text, "%s, \"%s\"", ok ? "accepted" : "refused", why.c_str());
}

// a skewed column stream: a few heavy columns, many ties
static coo make_skewed(uint64_t M, uint64_t K) {
    coo a;
    a.M = M;
    a.K = K;
    for (uint64_t r = 0; r < M; r++) {
        std::vector<uint64_t> c;
        if (r % 5 != 3)
            for (uint32_t i = 0, n = 1 + rnd(12); i < n; i++) c.push_back(rnd(3) ? rnd((uint32_t)K) : rnd(9) * 7 % K);
        std::sort(c.begin(), c.end());
        c.erase(std::unique(c.begin(), c.end()), c.end());
        for (uint64_t x : c) {
            a.row.push_back(r);
            a.col.push_back(x);
        }
    }
    a.rp = csr_row_ptr(a.row, M);
    return a;
}

static void column_order_case(const char *name, const coo &a, uint64_t hot) {
    g_case = name;
    const uint64_t K = a.K;
    const column_ranks o = column_order(a.col, K, hot);
    std::vector<uint32_t> deg(K, 0), hit(K, 0);
    for (uint64_t c : a.col) deg[c]++;
    EXPECT(o.perm.size() == K && o.rank.size() == K, "sizes");
    for (uint32_t c : o.perm)
        if (c < K) hit[c]++;
    for (uint64_t c = 0; c < K; c++) EXPECT(hit[c] == 1 && o.perm[o.rank[c]] == c, "not a permutation and its inverse at %llu", (unsigned long long)c);
    auto before = [&](uint32_t x, uint32_t y) { return deg[x] != deg[y] ? deg[x] > deg[y] : x < y; };
    const uint64_t H = hot == 0 || hot >= K ? K : hot;
    for (uint64_t i = 1; i < H; i++) EXPECT(before(o.perm[i - 1], o.perm[i]), "rank %llu is not by degree, then column", (unsigned long long)i);
    for (uint64_t i = H; i < K; i++) {
        EXPECT(before(o.perm[H - 1], o.perm[i]), "column %u is denser than a hot one", o.perm[i]);
        if (i > H) EXPECT(o.perm[i - 1] < o.perm[i], "the rest is not in column order");
    }
    hash_array("perm", o.perm);
    hash_array("rank", o.rank);
}

static void col_parts_case(const char *name, const coo &a, uint32_t P, uint64_t hub) {
    g_case = name;
    const uint64_t K = a.K, nnz = a.col.size();
    const col_parts s = split_col_parts(a.row, a.col, K, P, hub);
    const column_ranks o = column_order(a.col, K, 0);
    const bool hubs = hub > 0 && hub < K;
    EXPECT(s.base.size() == P + 1 && s.gather.size() == K && s.parts.size() == P && s.base[0] == 0 && s.base[P] == K, "sizes");
    std::vector<uint64_t> own(P, 0);
    for (uint64_t r = 0; r < K; r++) own[hubs ? (r < hub ? 0 : 1) : r % P]++;
    std::vector<uint32_t> pos(K, 0);
    for (uint32_t x = 0; x < P; x++) EXPECT(s.base[x + 1] - s.base[x] == own[x], "partition %u holds %llu columns", x, (unsigned long long)(s.base[x + 1] - s.base[x]));
    for (uint64_t r = 0; r < K; r++) {
        const uint64_t q = hubs ? r : s.base[r % P] + r / P;
        EXPECT(q < K && s.gather[q] == o.perm[r], "rank %llu is not at position %llu", (unsigned long long)r, (unsigned long long)q);
        if (q < K) pos[o.perm[r]] = (uint32_t)q;
    }
    std::vector<uint32_t> seen(nnz, 0);
    for (uint32_t x = 0; x < P; x++) {
        const col_part &p = s.parts[x];
        EXPECT(p.rows.size() == p.cols.size() && p.rows.size() == p.src.size() && !p.rows.empty(), "partition %u sizes", x);
        for (size_t i = 0; i < p.src.size(); i++) {
            const uint32_t e = p.src[i];
            EXPECT(e < nnz, "source entry out of range");
            if (e >= nnz) continue;
            seen[e]++;
            EXPECT(p.rows[i] == a.row[e] && p.cols[i] == pos[a.col[e]], "entry %u: row or position", e);
            EXPECT(p.cols[i] >= s.base[x] && p.cols[i] < s.base[x + 1], "entry %u is in the wrong partition", e);
            if (i) EXPECT(p.src[i - 1] < e, "partition %u is not in the plan's entry order", x);
        }
        hash_array("rows", p.rows);
        hash_array("cols", p.cols);
        hash_array("src", p.src);
    }
    for (uint64_t e = 0; e < nnz; e++) EXPECT(seen[e] == 1, "entry %llu lands in %u partitions", (unsigned long long)e, seen[e]);
    hash_array("base", s.base);
    hash_array("gather", s.gather);
}

static void levels_case(const char *name, const coo &a, uint64_t ws) {
    g_case = name;
    std::vector<uint64_t> lr, ln, wr, wn;
    merge_path_levels(a.row, a.M, ws, lr, ln);
    // the path itself: a row's nonzeros, then the step that closes it; empty rows are not on it
    std::vector<uint64_t> crow;
    for (uint64_t r = 0; r < a.M; r++)
        if (a.rp[r + 1] > a.rp[r]) crow.push_back(r);
    EXPECT(crow.size() < a.M && !crow.empty(), "the CSR needs empty rows");
    uint64_t j = 0, z = 0;
    for (uint64_t p = 0; j < crow.size(); p++) {
        if (p % ws == 0) {
            wr.push_back(crow[j]);
            wn.push_back(z);
        }
        if (z < a.rp[crow[j] + 1]) z++;
        else j++;
    }
    wn.push_back(a.col.size());
    EXPECT(lr == wr && ln == wn, "levels differ from a walk of the path (%zu levels, walk %zu)", lr.size(), wr.size());
    hash_array("level rows", lr);
    hash_array("level nonzeros", ln);
}

static void bitmap_case(const char *name, const coo &a, uint64_t bmt, uint64_t row_base, uint64_t extra) {
    g_case = name;
    std::vector<uint64_t> fn;
    for (uint64_t z = 0; z < a.col.size(); z += bmt) fn.push_back(z);
    fn.push_back(a.col.size());
    const uint64_t M = row_base + a.M + extra;
    const std::vector<uint32_t> list = bitmap_finalize_rows(a.row, fn, a.rp, a.M, M, row_base, 0, M);
    std::vector<uint8_t> want(M, 0);
    for (uint64_t r = 0; r < M; r++) {
        const bool in = r >= row_base && r - row_base < a.M;
        if (!in || a.rp[r - row_base] == a.rp[r - row_base + 1]) want[r] = 1;
        else
            for (uint64_t z = a.rp[r - row_base] + 1; z < a.rp[r - row_base + 1]; z++) want[r] |= z % bmt == 0;
    }
    std::vector<uint32_t> ref;
    for (uint64_t r = 0; r < M; r++)
        if (want[r]) ref.push_back((uint32_t)r);
    EXPECT(list == ref, "finalize list of %zu rows, want %zu", list.size(), ref.size());
    hash_array("finalize rows", list);
    hash_array("row masks", gsk_host::row_start_masks(a.row, fn));
}

int main(int argc, char **argv) {
    g_print = argc > 1 && !std::strcmp(argv[1], "--print");
    try {
        lds_case("fp16 N=32 20x2", 70, 500, 20, 2, 32, 2, 8 * 1024, false, 1);
        lds_case("fp32 N=32 pair_banks 20x2", 90, 600, 20, 2, 32, 4, 16 * 1024, false, 1);
        lds_case("fp32 N=32 pair_banks 16x4", 43, 300, 16, 4, 32, 4, 12 * 1024, false, 1);
        // LDS-DMA keeps two buffers of >= 64 B rows of 128 B: no budget under 16 KB + entries fits
        lds_case("fp32 N=32 dma 20x4", 70, 500, 20, 4, 32, 4, 24 * 1024, true, 1);
        lds_case("fp32 N=32 rowslot 20x5", 70, 600, 20, 5, 32, 4, 24 * 1024, true, 1);
        lds_case("fp32 N=32 rowslot 24x6", 100, 700, 24, 6, 32, 4, 24 * 1024, true, 1);
        lds_case("fp32 N=32 rowslot 32x8", 81, 450, 32, 8, 32, 4, 24 * 1024, true, 1);
        lds_case("fp32 N=32 want=3", 90, 700, 20, 2, 32, 4, 16 * 1024, false, 3);
        lds_case("fp32 N=32 rowslot want=3", 50, 640, 16, 8, 32, 4, 24 * 1024, true, 3);

        refusal("refuse N x vbytes", 20, 2, 6, 2, 16 * 1024, false, "B rows are not whole 16-B units");
        refusal("refuse 17 BMWs", 17, 1, 32, 4, 16 * 1024, false, "more than 16 BMWs per BMTB");
        refusal("refuse 5-row BMWs", 20, 5, 32, 4, 16 * 1024, false, "more than 4 rows per BMW");
        refusal("refuse small chunks", 20, 2, 32, 4, 4 * 1024, false, "column chunks would be under 64 rows of B");

        const coo s = make_skewed(120, 200);
        column_order_case("column_order hot=0", s, 0);
        column_order_case("column_order hot=17", s, 17);
        column_order_case("column_order hot=K", s, 200);
        col_parts_case("col parts P=3", s, 3, 0);
        col_parts_case("col parts P=2 hub=10", s, 2, 10);
        col_parts_case("col parts P=2", s, 2, 0);

        const coo l = make_skewed(30, 64);
        levels_case("merge_path_levels ws=7", l, 7);
        levels_case("merge_path_levels ws=1", l, 1);
        levels_case("merge_path_levels ws=64", l, 64);
        bitmap_case("bitmap rows", s, 8, 0, 0);
        bitmap_case("bitmap rows, sub-matrix", l, 16, 5, 3);

        // the GPU edge pattern's size at the upload's budgets (160 KB; 80 KB with LDS-DMA), K split 1, 2 and
        // the upload's automatic one (256 / BMTBs, 512 / BMTBs with LDS-DMA): two chunks of 104 columns in one
        // K range, the same in two, and three of 72 (a fourth would make chunks of under 64).  No K split gives
        // one chunk here: a chunk is a multiple of 8 columns and build_lds_tiles passes over a chunk wider than
        // K, so K = 203 never goes as one chunk of 208.  tests/test_gpu_lds_variants.py pins the same table
        const coo e = make_edge();
        const struct { const char *name; uint64_t tbr, bwr; uint32_t N, vbytes; bool dma; } kEdge[] = {
            {"edge fp16 N=8 20x2", 20, 2, 8, 2, false},     {"edge fp32 N=32 pair_banks 20x2", 20, 2, 32, 4, false},
            {"edge fp32 N=32 dma 20x2", 20, 2, 32, 4, true}, {"edge fp32 N=32 rowslot 40x5", 40, 5, 32, 4, true},
            {"edge fp32 N=32 rowslot 64x8", 64, 8, 32, 4, true}};
        for (const auto &c : kEdge) {
            const uint64_t nbt = (e.M + c.tbr - 1) / c.tbr, wants[3] = {1, 2, (c.dma ? 512u : 256u) / nbt};
            const uint32_t pins[3][2] = {{104, 2}, {104, 2}, {72, 3}};
            for (int w = 0; w < 3; w++) {
                const std::string name = std::string(c.name) + (w == 0 ? " want=1" : w == 1 ? " want=2" : " want=auto");
                lds_case(name.c_str(), e.M, e.K, c.tbr, c.bwr, c.N, c.vbytes, (c.dma ? 80 : 160) * 1024, c.dma, wants[w], &e,
                         pins[w][0], pins[w][1]);
            }
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s: %s\n", g_case.c_str(), e.what());
        return 2;
    }
    if (!g_print) {
        g_case = "hashes";
        EXPECT(g_hash_at == sizeof(kExpect) / sizeof(kExpect[0]), "%zu arrays hashed, %zu expected", g_hash_at, sizeof(kExpect) / sizeof(kExpect[0]));
        std::printf("gather_layout_check: %zu arrays, %ld failures\n", g_hash_at, g_bad);
    }
    return g_bad ? 1 : 0;
}
