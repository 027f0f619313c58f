// hip_code/kernel_common.hpp -- what the kernel family headers share: the raw vector types,
// the fp32 load / store / atomic helpers, the read-once loads, xcd_block, epilogue_apply, fma_row, and the
// helpers of more than one matrix-core family (fragment types, b_piece, ks_slab_wait).
// A family header includes this one and nothing else of hip_code/.
#pragma once

#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "idx_formula.hpp"
#include "kernel_consts.hpp"

namespace gsk {

typedef _Float16 f16;
// bfloat16 (GS_BF16 plans): (float)bf16 is a 16-bit shift, (bf16)float one round-to-nearest-even
// conversion (v_cvt_pk_bf16_f32 on gfx950)
typedef __bf16 bf16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

template <int BYTES> struct raw_vec;
template <> struct raw_vec<2> { typedef uint16_t t; };
template <> struct raw_vec<4> { typedef uint32_t t; };
template <> struct raw_vec<8> { typedef uint2 t; };
template <> struct raw_vec<16> { typedef uint4 t; };
struct alignas(16) u32x8 { uint4 lo, hi; };
template <> struct raw_vec<32> { typedef u32x8 t; };

// CF contiguous values -> fp32 (one vector load)
template <class VT, int CF>
__device__ __forceinline__ void load_f32(const VT *__restrict__ p, float (&out)[CF]) {
    typedef typename raw_vec<CF * sizeof(VT)>::t R;
    R r = *reinterpret_cast<const R *>(p);
    VT tmp[CF];
    __builtin_memcpy(tmp, &r, sizeof(R));
#pragma unroll
    for (int k = 0; k < CF; k++) out[k] = (float)tmp[k];
}

template <class VT, int CF>
__device__ __forceinline__ void store_f32(VT *__restrict__ p, const float (&in)[CF]) {
    typedef typename raw_vec<CF * sizeof(VT)>::t R;
    VT tmp[CF];
#pragma unroll
    for (int k = 0; k < CF; k++) tmp[k] = (VT)in[k];
    R r;
    __builtin_memcpy(&r, tmp, sizeof(R));
    *reinterpret_cast<R *>(p) = r;
}

// Loads of the operand a launch reads exactly once (A's entries, groups, panels).  GS_A_NT=1
// (make A_NT=1): the non-temporal form (global_load ... nt), which the XCD's L2 holds at low
// retention, so the stream does not push out the rows of B that other workgroups re-read.
template <class T>
__device__ __forceinline__ T ld_once(const T *p) {
#if defined(GS_A_NT) && GS_A_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
// the same, chosen per instantiation (k_mfma_ks KS_NT, k_nm_mfma NM_NT): NT loads bypass the CU's
// L1 and stream through L2 (MI355X_MICROARCH.md: nt loads are L2-served)
template <bool NT, class T>
__device__ __forceinline__ T ld_once_if(const T *p) {
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return ld_once(p);
}
template <int BYTES> struct raw_ext;
template <> struct raw_ext<1> { typedef uint8_t t; };
template <> struct raw_ext<2> { typedef uint16_t t; };
template <> struct raw_ext<4> { typedef uint32_t t; };
template <> struct raw_ext<8> { typedef u32x2 t; };
template <> struct raw_ext<16> { typedef u32x4 t; };

// SCF contiguous sparse entries (cols or vals) in one load (read once: ld_once)
template <class T, int SCF>
__device__ __forceinline__ void load_raw(const T *__restrict__ p, T (&out)[SCF]) {
    if constexpr (SCF * sizeof(T) <= 16) {
        typedef typename raw_ext<SCF * sizeof(T)>::t R;
        R r = ld_once(reinterpret_cast<const R *>(p));
        __builtin_memcpy(out, &r, sizeof(R));
    } else {
        static_assert(SCF * sizeof(T) == 32, "8 to 32 bytes");
        u32x4 r[2] = {ld_once(reinterpret_cast<const u32x4 *>(p)), ld_once(reinterpret_cast<const u32x4 *>(p) + 1)};
        __builtin_memcpy(out, r, 32);
    }
}

template <int CF>
__device__ __forceinline__ void wave_reduce_slots(float (&acc)[CF], int X) {
    for (int off = X; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < CF; k++) acc[k] += __shfl_xor(acc[k], off, 64);
    }
}

template <class VT, int CF>
__device__ __forceinline__ void atomic_add_vals(VT *p, const float (&v)[CF]);

template <>
__device__ __forceinline__ void atomic_add_vals<float, 1>(float *p, const float (&v)[1]) {
    unsafeAtomicAdd(p, v[0]);
}
template <>
__device__ __forceinline__ void atomic_add_vals<float, 4>(float *p, const float (&v)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) unsafeAtomicAdd(p + k, v[k]);
}
template <>
__device__ __forceinline__ void atomic_add_vals<float, 8>(float *p, const float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k++) unsafeAtomicAdd(p + k, v[k]);
}
template <>
__device__ __forceinline__ void atomic_add_vals<f16, 8>(f16 *p, const float (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        __half2 h = __floats2half2_rn(v[k], v[k + 1]);
        unsafeAtomicAdd(reinterpret_cast<__half2 *>(p + k), h);
    }
}
template <>
__device__ __forceinline__ void atomic_add_vals<f16, 1>(f16 *p, const float (&v)[1]) {
    unsafeAtomicAdd(reinterpret_cast<__half *>(p), __float2half(v[0]));
}

// XCD-aware block numbering (cdna_hip_programming.md §5.5 T1): blocks b and b + 8 are
// observed to share an XCD (round-robin dispatch, MI355X_MICROARCH.md §Workgroup dispatch),
// so consecutive blockIdx read the neighbouring cache lines of A's streams from eight
// different L2s.  The bijective renumbering gives each XCD one contiguous range of
// logical block ids instead; a speed choice only, any placement stays correct.
__device__ __forceinline__ uint32_t xcd_block(uint32_t b, uint32_t n) {
#ifdef GS_NO_XCD_SWIZZLE  // A/B diagnostic builds only
    return b;
#endif
    const uint32_t q = n >> 3, r = n & 7u, x = b & 7u;
    return (x < r ? x * (q + 1u) : r * (q + 1u) + (x - r) * q) + (b >> 3);
}

// The epilogue of one element of C (gsk::epilogue, kernel_consts.hpp): acc = the fp32 value of
// (A * B)[row][col]; res = float(residual[row][col]), loaded by the caller when e.residual is set
// and ignored otherwise.  The stages in their fixed order, a stage that is not requested skipped
// (never an added zero: -0 and NaN pass as they are); the caller rounds the result once, to the
// plan dtype.  Called by k_mfma_ks's store_item (the fused path: acc is the kernel's fp32 sum)
// and by k_epilogue (the post-pass: acc is float(C) as the family wrote it), so the two agree.
__device__ __forceinline__ float epilogue_apply(const epilogue &e, float acc, size_t row, float res) {
    // (__fmul_rn / __fadd_rn: never contracted into an fma, so every stage rounds on its own in
    // both callers)
    float t = __fmul_rn(e.alpha, acc);
    if (e.bias) t = __fadd_rn(t, e.bias[row]);
    if (e.act == kEpiRelu) t = t < 0.f ? 0.f : t;  // NaN: the comparison is false, NaN stays
    if (e.residual) t = __fadd_rn(t, res);
    return t;
}

// one sparse entry times a CF-wide B segment
template <class VT, int CF>
__device__ __forceinline__ void fma_row(float (&acc)[CF], float v, const VT *__restrict__ brow) {
    float b[CF];
    load_f32<VT, CF>(brow, b);
#pragma unroll
    for (int k = 0; k < CF; k++) acc[k] = __builtin_fmaf(v, b[k], acc[k]);
}

// matrix-core operand and accumulator fragments (k_mfma_*, k_nm_mfma*; f4v also k_lds_rows*)
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s4v lds_s4v;
typedef _Float16 h16v __attribute__((ext_vector_type(16)));
// the bf16 MFMA's operands (v_mfma_f32_16x16x32_bf16): 8 x bf16 per lane, as h8v for fp16
typedef __bf16 b8v __attribute__((ext_vector_type(8)));
// a matrix-core element type's operand fragment and its 16x16x32 MFMA into fp32 (k_mfma_ks)
template <class ET> struct mfma_elem;
template <> struct mfma_elem<f16> {
    typedef h8v frag;
    static __device__ __forceinline__ f4v mfma_16x16x32(const frag &a, const frag &b, const f4v &c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
    }
};
template <> struct mfma_elem<bf16> {
    typedef b8v frag;
    static __device__ __forceinline__ f4v mfma_16x16x32(const frag &a, const frag &b, const f4v &c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
    }
};
// 8 bytes at a 2-byte-aligned address (k_mfma_kb / k_mfma_bm value windows)
typedef uint32_t u32x2_a2 __attribute__((ext_vector_type(2), aligned(2)));

// the place of 32-byte piece p of LDS B row k (a 16*CT-column tile): XOR-permuted so that the
// transposed fragment reads (ds_read_b64_tr_b16) are conflict-free
template <int CT>
__device__ __forceinline__ uint32_t b_piece(uint32_t k, uint32_t p) {
    uint32_t sw;
    if constexpr (CT == 1) sw = 0;
    else if constexpr (CT == 2) sw = (k >> 3) & 1u;
    else if constexpr (CT == 4) sw = ((k >> 1) & 1u) | (((k >> 3) & 1u) << 1);
    else sw = (k & 3u) | (((k >> 3) & 1u) << 2);
    return p ^ (sw & (uint32_t)(CT - 1));
}

// FP8 weights (k_mfma_ks_w8, k_mfma_ks_tm with VB = 8): a group's 8 OCP e4m3fn codes (byte e = entry e) as the 4
// registers of packed fp16 the 16-bit form loads (halfword e = entry e).  Exact: every finite e4m3 value
// is an fp16 value.  v_cvt_scalef32_pk_f16_fp8 with scale 1.0 converts two codes per instruction (the low
// or the high pair of a register: op_sel), 4 VALU per group.
// GS_KS_W8_ALU (0; 1 in a variant build for the A/B): the same values by integer operations and one
// packed multiply -- the two codes into the high byte of each half (v_perm_b32), sign | (exponent,
// mantissa) >> 1 as the fp16 bits of value / 256, times 256 (v_pk_mul_f16; fp16 denormals on)
#ifndef GS_KS_W8_ALU
#define GS_KS_W8_ALU 0
#endif
__device__ __forceinline__ u32x4 ks_decode8(const u32x2 &c) {
    u32x4 o;
#if GS_KS_W8_ALU
    typedef _Float16 h2v __attribute__((ext_vector_type(2)));
    const h2v k256 = {(_Float16)256.f, (_Float16)256.f};
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t w = __builtin_amdgcn_perm(0u, c[i >> 1], (i & 1) ? 0x030c020cu : 0x010c000cu);
        const uint32_t b = (w & 0x80008000u) | ((w & 0x7f007f00u) >> 1);
        h2v h;
        __builtin_memcpy(&h, &b, 4);
        h = h * k256;
        uint32_t r;
        __builtin_memcpy(&r, &h, 4);
        o[i] = r;
    }
#else
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const auto h = (i & 1) ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[i >> 1], 1.0f, true)
                               : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c[i >> 1], 1.0f, false);
        uint32_t r;
        __builtin_memcpy(&r, &h, 4);
        o[i] = r;
    }
#endif
    return o;
}
// a loaded group's 8 values as 16-bit words: the registers themselves (VB = 16), or the decoded codes
template <int VB>
__device__ __forceinline__ const u32x4 &ks_group_values(const u32x4 &v) {
    static_assert(VB == 16, "16-bit values are loaded as u32x4");
    return v;
}
template <int VB>
__device__ __forceinline__ u32x4 ks_group_values(const u32x2 &c) {
    static_assert(VB == 8, "e4m3 codes are loaded as u32x2");
    return ks_decode8(c);
}

// K-split combine: the last ticket holder's read of 4 words of another workgroup's slab
// (each word tagged in its low mantissa bit): agent-scope (sc1) loads until every tag reads
// `tag`.  The writer holds an earlier ticket, so it is resident and its stores are issued or
// about to be; the wait is bounded by wall time (s_memrealtime, 100 MHz: 0.2 s) all the same.
// Past the bound the words read as NaN and bit 0 of the plan replica's device error word
// (`err`, the word after the arrival counters) is set: gs_plan_device_status reports it as
// GS_ERR_DEVICE, so a lost slab is an error at the C ABI, not silent NaNs in C.  `force`
// (experiments build, KS_FORCE_TIMEOUT) takes the timeout path at once (the test of that chain).
__device__ __forceinline__ u32x4 ks_slab_wait(const uint32_t *src, uint32_t tag, uint32_t *err, bool force) {
    u32x4 w;
    auto load4 = [&]() {
#pragma unroll
        for (int i = 0; i < 4; i++) w[i] = __hip_atomic_load(src + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto stale = [&]() { return (((w[0] ^ tag) | (w[1] ^ tag) | (w[2] ^ tag) | (w[3] ^ tag)) & 1u) != 0u; };
    bool lost = force;
    if (!lost) {
        load4();
        if (stale()) {
            // the bound needs 0.2 s of wall time AND 1024 polls since the last gap: a gap of
            // over 1 ms between two polls means this wave was switched out (CWSR time slicing),
            // so the bound restarts rather than counting the time the writer could not run
            uint64_t t0 = __builtin_amdgcn_s_memrealtime(), prev = t0;
            uint32_t polls = 0;
            do {
                const uint64_t t = __builtin_amdgcn_s_memrealtime();
                if (t - prev > 100000ull) {
                    t0 = t;
                    polls = 0;
                }
                prev = t;
                if (t - t0 > 20000000ull && polls >= 1024u) {
                    lost = true;
                    break;
                }
                polls++;
                __builtin_amdgcn_s_sleep(2);
                load4();
            } while (stale());
        }
    }
    if (lost) {
        w = u32x4{0x7fc00000u | tag, 0x7fc00000u | tag, 0x7fc00000u | tag, 0x7fc00000u | tag};
        __hip_atomic_fetch_or(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    return w;
}
#ifdef GS_EXPERIMENTS
#define GS_KS_FORCE(prio) (((prio) & 16u) != 0u)
#else
#define GS_KS_FORCE(prio) false
#endif

}  // namespace gsk
