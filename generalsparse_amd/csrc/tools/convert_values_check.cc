// convert_values_check -- gs_convert_values (the upload's conversion of A's values) for the three
// plan dtypes against an arithmetic reference, as a stand-alone host program: no GPU, no Python.
// Built against the ASan/UBSan host objects by `make san_check` (Makefile), so the conversion
// runs instrumented; it also links against the plain library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "generalsparse.h"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// x rounded to nearest even in a binary format of E exponent and M mantissa bits, as its encoding:
// scaled to an integer significand and rounded by nearbyint (no bit tricks shared with the library)
static uint16_t ref_bits(float x, int E, int M) {
    const uint16_t sign = std::signbit(x) ? (uint16_t)(1u << (E + M)) : 0;
    const uint16_t inf = (uint16_t)(((1u << E) - 1u) << M);
    if (std::isinf(x)) return sign | inf;
    const double a = std::fabs((double)x);
    if (a == 0.0) return sign;
    const int bias = (1 << (E - 1)) - 1, emin = 1 - bias;
    int ex;
    std::frexp(a, &ex);
    int e = ex - 1 < emin ? emin : ex - 1;
    double q = std::nearbyint(std::ldexp(a, M - e));
    if (q == std::ldexp(1.0, M + 1)) {
        e++;
        q = std::ldexp(1.0, M);
    }
    if (e > bias) return sign | inf;
    if (q < std::ldexp(1.0, M)) return sign | (uint16_t)q;  // subnormal (or zero)
    return sign | (uint16_t)((unsigned)(e + bias) << M) | (uint16_t)(q - std::ldexp(1.0, M));
}

int main() {
    std::vector<float> x;
    // every tie and its neighbours on the bf16 grid, both signs, denormals included
    for (uint32_t k = 0; k < 0x7f80u; k++)
        for (uint32_t lo : {0x7fffu, 0x8000u, 0x8001u})
            for (uint32_t s : {0u, 0x80000000u}) x.push_back(from_bits(s | (k << 16) | lo));
    // ... and on the fp16 grid (13 dropped bits), through its exponent range and past it
    for (uint32_t k = 0x33000000u >> 13; k < (0x47800000u >> 13) + 64u; k += 3)
        for (uint32_t lo : {0x0fffu, 0x1000u, 0x1001u}) x.push_back(from_bits((k << 13) | lo));
    for (uint32_t b : {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x00000001u, 0x00007fffu, 0x00008000u, 0x00008001u,
                       0x007fffffu, 0x807fffffu, 0x7f7f0000u, 0x7f7f0001u, 0x7f7f7fffu, 0x7f7f8000u, 0x7f7fffffu, 0xff7f8000u,
                       0x477fe000u, 0x477ff000u, 0x33000000u, 0x33000001u, 0x32ffffffu})
        x.push_back(from_bits(b));
    uint64_t st = 0x9e3779b97f4a7c15ull;  // seeded values over 2^+-60
    for (int i = 0; i < 100000; i++) {
        st = st * 6364136223846793005ull + 1442695040888963407ull;
        const uint32_t man = (uint32_t)(st >> 41), ex = 127u - 60u + (uint32_t)((st >> 20) % 121u), sg = (uint32_t)(st >> 63);
        x.push_back(from_bits((sg << 31) | (ex << 23) | man));
    }
    const uint64_t n = x.size();
    long bad = 0;
    std::vector<uint16_t> h(n);
    std::vector<float> f(n);
    if (gs_convert_values(x.data(), n, GS_BF16, h.data())) return std::fprintf(stderr, "bf16: %s\n", gs_last_error()), 2;
    for (uint64_t i = 0; i < n; i++)
        if (h[i] != ref_bits(x[i], 8, 7) && ++bad < 10) std::fprintf(stderr, "bf16 %a: %04x, want %04x\n", x[i], h[i], ref_bits(x[i], 8, 7));
    if (gs_convert_values(x.data(), n, GS_F16, h.data())) return std::fprintf(stderr, "f16: %s\n", gs_last_error()), 2;
    for (uint64_t i = 0; i < n; i++)
        if (h[i] != ref_bits(x[i], 5, 10) && ++bad < 10) std::fprintf(stderr, "f16 %a: %04x, want %04x\n", x[i], h[i], ref_bits(x[i], 5, 10));
    if (gs_convert_values(x.data(), n, GS_F32, f.data())) return std::fprintf(stderr, "f32: %s\n", gs_last_error()), 2;
    if (std::memcmp(f.data(), x.data(), n * 4)) bad++, std::fprintf(stderr, "f32 is not the identity\n");
    // NaN stays a quiet NaN at both 16-bit types
    const float nans[4] = {from_bits(0x7fc00000u), from_bits(0xffc00000u), from_bits(0x7f800001u), from_bits(0xff80ffffu)};
    uint16_t nb[4];
    gs_convert_values(nans, 4, GS_BF16, nb);
    for (uint16_t v : nb) bad += !((v & 0x7f80u) == 0x7f80u && (v & 0x0040u));
    gs_convert_values(nans, 4, GS_F16, nb);
    for (uint16_t v : nb) bad += !((v & 0x7c00u) == 0x7c00u && (v & 0x0200u));
    // refusals: an unknown dtype, a null buffer; nothing is written
    uint16_t keep = 0xabcd;
    bad += gs_convert_values(x.data(), 1, 3, &keep) != GS_ERR || keep != 0xabcd;
    bad += gs_convert_values(nullptr, 1, GS_BF16, &keep) != GS_ERR || keep != 0xabcd;
    bad += gs_convert_values(nullptr, 0, GS_BF16, nullptr) != GS_OK;
    std::printf("convert_values_check: %llu values x 3 dtypes, %ld mismatches\n", (unsigned long long)n, bad);
    return bad ? 1 : 0;
}
