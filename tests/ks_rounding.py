"""Rounding rungs for the k_mfma_ks family (k_mfma_ks, k_mfma_ks_w8, k_mfma_ks_tm): operands whose
result is decided by the lowest fp32 bit of a K-range partial sum, and the model that predicts the
kernels' bits from the design.  No GPU is touched here: tests/test_ks_rounding_host.py checks on the
CPU that the rungs mean what they claim, tests/test_gpu_ks_rounding.py compares the kernels with them.

The idea: at a rounding tie the lowest fp32 bit decides the 16-bit result.  The fp32 sum 1 + 2^-11
rounds to the f16 value 1.0, 1 + 2^-11 + 2^-23 to 1 + 2^-10.  With more than one K range every fp32
partial sum loses that bit to the slab's validity tag (the K-split combine), so a plan with
three K ranges and the same plan with one differ at exactly such a sum -- and a reader that left the
tag in place, a truncating or round-half-away conversion or a second rounding each move some rung.

Operands.  A is ks_pattern(K) of tests/test_gpu_edges_mfma.py (131 x K, K = 1176 or 1184) with the
entries of nine *rung columns* replaced: three per K range of the KS_SPLIT = 3 layout (ranges of 416
columns), every one in a 32-column k-step of its own, column 0 and column K - 1 among them.  A row
that has no term at a rung column has no entry there.  X (tokens x K) is zero outside the rung
columns, so the pattern's other entries (the filler) contribute only +-0 and
Y[t, r] = sum_j X[t, c_j] * A[r, c_j]: at most one non-zero product per MFMA.  Each rung is one row of
A; its terms are written as products, A[r, c] = product / X[0, c].  Every A and X value is a normal
value of the dtype -- signed powers of two, and 2047 / 8 in X, which carries 32752's significand.
Tokens 0 .. 31 share one X row; tokens 32 .. 39 scale it by -1, 2^-1 and 2^3 (an entry that would
leave the dtype's normal range by that is zero instead: the f16 columns that hold 2^-14, at 2^-1).

FP8 weights (f16 activations): every A value of a row is an e4m3 value times the row's power-of-two
scale -- 1 where the row's values allow it -- and X is the same as for f16.

The rungs are the table of the host test (TABLE there); what differs from a plain reading of it:
- "odd partials in all three ranges" is (1 + 2^-23 | 1 + 2^-23 | 2^-10 + 2^-33) times 2^6, two products
  per range: no two normal f16 values multiply to 2^-33 (the least product is 2^-28), and the sum
  2 + 2^-10 sits on an f16 tie, so the result is 2 (here 128), not 2 + 2^-10, which is no f16 value.
  Its one-range sum is no fp32 value, so the rung exists only in operands built for three ranges;
- bf16 takes the same rungs with the tie at 2^-8 and the 257 / 259 pair of test_ks_rounding_ladder;
  the f16 overflow and subnormal rungs are dropped for it (bf16 shares fp32's exponent range: its
  overflow and subnormal edges are fp32's, which these operands never reach)."""
import functools
import itertools

import numpy as np
import torch

from test_gpu_edges import TORCH_DT
from test_gpu_edges_mfma import KS_M, ks_pattern, ks_ranges
from test_gpu_epilogue import epilogue_ref

KS = (1176, 1184)
CASES = [(1176, 1), (1176, 3), (1184, 1), (1184, 2)]  # (K, KS_SPLIT)
KINDS = ("f16", "bf16", "fp8")                       # fp8: f16 activations, e4m3 weight values
N_TOKENS = 40
TOKEN_SCALE = np.array([1.0] * 32 + [-1.0] * 3 + [0.5] * 3 + [8.0] * 2)
GRAD_ROWS = (1, 33, 129)  # filler rows the SparseLinear test's incoming gradient is non-zero in

# dtype: (significand bits, least normal exponent, largest finite value)
FORMAT = {"f16": (11, -14, 65504.0), "bf16": (8, -126, float.fromhex("0x1.fep127"))}


def dtype_of(kind):
    return "f16" if kind == "fp8" else kind


def range_width(K, split):
    """columns per K range at KS_SPLIT = split > 0 (device_layout.cc build_ks_tiles, as ks_ranges)"""
    S = max(1, min(split, (K + 31) // 32))
    return ((K + S - 1) // S + 31) // 32 * 32


def split_of(K, ksplit):
    """a KS_SPLIT that gives `ksplit` K ranges (plan.info()["ksplit"]); every such value gives one width"""
    found = [s for s in range(1, (K + 31) // 32 + 1) if ks_ranges(K, s) == ksplit]
    assert found and len({range_width(K, s) for s in found}) == 1, (K, ksplit, found)
    return found[0]


def range_slices(K, split):
    KR = range_width(K, split)
    return [slice(q * KR, min(K, (q + 1) * KR)) for q in range(ks_ranges(K, split))]


# ------------------------------------------------------------------ rung columns and X
SLOTS = ("a0", "a1", "a2", "b0", "b1", "b2", "c0", "c1", "c2")  # a / b / c: K range 0 / 1 / 2 at KS_SPLIT = 3


def rung_columns(K):
    """slot -> column: 32-column k-steps 0, 1, 3 | 13, 15, 17 | 26, 28 and the last one"""
    return dict(zip(SLOTS, (0, 40, 100, 421, 486, 546, 835, 900, K - 1)))


def x_base(dtype):
    """slot -> X[0, column]: powers of two, and 2047 / 8 at b2 for f16 (2^7 * 2047 / 8 = 32752)"""
    e = dict(zip(SLOTS, (8, -5, -13, 2, -14, 5, -2, -14, -13)))
    x = {s: 2.0 ** v for s, v in e.items()}
    if dtype == "f16":
        x["b2"] = 2047.0 / 8
    return x


# ------------------------------------------------------------------ the rungs
def rungs(dtype, three_ranges):
    """[(name, {slot: product})]: one weight row each.  u is half an ulp of 1.0 in the dtype"""
    u = 2.0 ** -11 if dtype == "f16" else 2.0 ** -8
    b = 2.0 ** -23
    R = [("tie to even, down", {"a0": 1, "a1": u}),
         ("tie to even, up", {"a0": 1, "a1": 2 * u, "b1": u}),
         ("above the tie, one range", {"a0": 1, "a1": u, "a2": b}),
         ("above the tie, across ranges", {"a0": 1, "a1": u, "b1": b}),
         ("tie in the last k-step", {"a0": 1, "c2": u}),
         ("above the tie, three ranges", {"a0": 1, "b1": u, "c2": b})]
    if dtype == "f16":
        R += [("2049", {"a0": 2048, "b0": 1}),
              ("2051", {"a0": 2048, "a1": 2, "b0": 1}),
              ("65520", {"a0": 32768, "b2": 32752}),
              ("just under 65520", {"a0": 32768, "b2": 32752, "b0": -2.0 ** -8}),
              ("subnormal tie", {"a2": 2.0 ** -24, "b1": 2.0 ** -25}),
              ("2^-25", {"a2": 2.0 ** -25}),
              ("just above 2^-25", {"a2": 2.0 ** -25, "b1": 2.0 ** -28}),
              ("1.25 subnormal ulps", {"a2": 2.0 ** -24, "b1": 2.0 ** -26}),
              ("epilogue, two ranges", {"a0": 1, "b1": 2.0 ** -12}),
              ("epilogue, one range", {"a0": 1, "a1": 2.0 ** -12})]
        mirrored = ("tie to even, down", "tie to even, up", "above the tie, one range", "above the tie, across ranges",
                    "above the tie, three ranges", "65520", "subnormal tie", "2^-25", "just above 2^-25")
    else:
        R += [("257", {"a0": 256, "b0": 1}),
              ("259", {"a0": 256, "a1": 2, "b0": 1})]
        mirrored = ("tie to even, down", "tie to even, up", "above the tie, one range", "above the tie, across ranges",
                    "above the tie, three ranges", "257")
    if three_ranges:
        R.append(("odd partials in all three ranges", {"a0": 64, "a2": 64 * b, "b0": 64, "b1": 64 * b, "c0": 128 * u, "c1": 128 * u * b}))
    terms = dict(R)
    R += [("negative: " + n, {s: -p for s, p in terms[n].items()}) for n in mirrored]
    return R


# rows for the rungs, block by block in turn (40-row blocks: 40, 40, 40 and 11 rows); none of GRAD_ROWS
_BLOCK_ROWS = ((3, 7, 12, 18, 22, 27, 31, 36), (41, 46, 52, 57, 63, 70, 76, 79), (80, 85, 91, 97, 104, 110, 115, 119),
               (120, 122, 124, 125, 127, 128))
_FIXED_ROWS = {"tie in the last k-step": 130, "above the tie, three ranges": 39}  # last rows of the 11- and a 40-row block


def rung_rows(names):
    """name -> row of A"""
    free = [list(b) for b in _BLOCK_ROWS]
    out, turn = {}, 0
    for n in names:
        if n in _FIXED_ROWS:
            out[n] = _FIXED_ROWS[n]
            continue
        while not free[turn % 4]:
            turn += 1
        out[n] = free[turn % 4].pop(0)
        turn += 1
    assert len(set(out.values())) == len(out) and not set(out.values()) & set(GRAD_ROWS)
    return out


class Operands:
    """one operand set: A as COO and dense, X, the rungs' rows; for fp8 the codes' values and the scales"""


@functools.lru_cache(maxsize=None)
def operands(kind, K, three_ranges=False):
    """the operand set of a dtype / weight kind at K; three_ranges: with the rung that needs three K ranges.
    Never written after it is made"""
    dtype = dtype_of(kind)
    cols, xb = rung_columns(K), x_base(dtype)
    R = rungs(dtype, three_ranges)
    rows = rung_rows([n for n, _ in R])
    prow, pcol, pval, _ = ks_pattern(K)
    keep = ~np.isin(pcol.astype(np.int64), list(cols.values()))
    r = [prow[keep].astype(np.int64)]
    c = [pcol[keep].astype(np.int64)]
    v = [pval[keep].astype(np.float64)]
    for name, terms in R:
        for slot, prod in terms.items():
            r.append(np.array([rows[name]]))
            c.append(np.array([cols[slot]]))
            v.append(np.array([prod / xb[slot]]))
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
    order = np.lexsort((c, r))
    o = Operands()
    o.kind, o.dtype, o.K, o.three_ranges = kind, dtype, K, three_ranges
    o.rungs, o.rows, o.cols = R, rows, cols
    o.row, o.col = r[order].astype(np.uint64), c[order].astype(np.uint64)
    o.val = v[order].astype(np.float32)
    assert (o.val.astype(np.float64) == v[order]).all()
    o.A = np.zeros((KS_M, K), np.float64)
    o.A[r, c] = v
    X = np.zeros((N_TOKENS, K), np.float64)
    _, emin, vmax = FORMAT[dtype]
    for slot, col in cols.items():
        x = TOKEN_SCALE * xb[slot]
        X[:, col] = np.where((np.abs(x) >= 2.0 ** emin) & (np.abs(x) <= vmax), x, 0.0)
    o.X = X
    o.X_t = torch.from_numpy(X).to(TORCH_DT[dtype])
    assert (o.X_t.double().numpy() == X).all()
    o.scale = o.codes_val = o.A_codes = None
    if kind == "fp8":
        o.scale = fp8_row_scales(o.row.astype(np.int64), o.val)
        o.codes_val = o.val / o.scale[o.row.astype(np.int64)]  # what the stored codes decode to
        o.A_codes = o.A / o.scale.astype(np.float64)[:, None]
    for a in (o.row, o.col, o.val, o.A, o.X):
        a.setflags(write=False)
    return o


def operands_for(kind, K, split):
    return operands(kind, K, ks_ranges(K, split) == 3)


def fp8_row_scales(row, val):
    """float32 powers of two, one per row: 2^e with e the value nearest 0 for which every value of the
    row over 2^e is a power of two in e4m3's range 2^-9 .. 2^8 (these rows hold nothing else)"""
    scale = np.ones(KS_M, np.float32)
    for r in range(KS_M):
        m, e = np.frexp(np.abs(val[row == r]).astype(np.float64))
        if len(e) == 0:
            continue
        assert (m == 0.5).all(), r  # |v| = m 2^e with m in [0.5, 1): powers of two only
        lo, hi = int(e.max()) - 1 - 8, int(e.min()) - 1 + 9
        assert lo <= hi, (r, lo, hi)
        scale[r] = 2.0 ** min(max(0, lo), hi)
    return scale


# ------------------------------------------------------------------ the model
def ks_model(A, X, K, split, *, scale=None, truncate=True, leak_tag=0):
    """the fp32 value store_item rounds: float32 (n, M).  A: (M, K) float64 (for FP8 the decoded codes,
    with scale the rows' float32 scales), X: (n, K) float64.  Per K range the float64 product, which
    must be an fp32 value; with more than one range bit 0 of its fp32 encoding cleared (leak_tag = 1:
    set instead; truncate = False: left as it is); the ranges added in q order in fp32 from +0; for
    FP8 the sum times scale[row] in fp32"""
    A, X = np.asarray(A, np.float64), np.asarray(X, np.float64)
    live = np.nonzero((X != 0).any(0))[0]  # (elsewhere A meets 0: +-0, which changes no sum that starts at +0)
    ranges = range_slices(K, split)
    acc = np.zeros((X.shape[0], A.shape[0]), np.float32)
    for sl in ranges:
        c = live[(live >= sl.start) & (live < sl.stop)]
        part64 = X[:, c] @ A[:, c].T
        part = part64.astype(np.float32)
        assert (part.astype(np.float64) == part64).all(), "a K range's partial sum is no fp32 value"
        if len(ranges) > 1:
            bits = part.view(np.uint32)
            if leak_tag:
                bits = bits | np.uint32(1)
            elif truncate:
                bits = bits & ~np.uint32(1)
            part = bits.view(np.float32)
        acc = acc + part
        assert acc.dtype == np.float32
    if scale is not None:
        acc = acc * np.asarray(scale, np.float32)[None, :]
    return acc


def round_to(v, dtype, mode="nearest_even"):
    """float64 values rounded to the dtype's values, as float64; mode: nearest_even, toward_zero, half_away"""
    v = np.asarray(v, np.float64)
    p, emin, vmax = FORMAT[dtype]
    a = np.abs(v)
    e = np.maximum(np.frexp(a)[1] - 1, emin)
    ulp = np.ldexp(1.0, e - (p - 1))
    q = a / ulp  # exact: a power of two
    f = np.floor(q)
    r = q - f
    if mode == "toward_zero":
        n = f
    elif mode == "half_away":
        n = f + (r >= 0.5)
    else:
        assert mode == "nearest_even", mode
        n = f + ((r > 0.5) | ((r == 0.5) & (f % 2 == 1)))
    out = n * ulp
    out = np.where(out > vmax, vmax if mode == "toward_zero" else np.inf, out)
    return np.copysign(out, v)


def on_tie(v, dtype):
    """where a float64 value lies exactly halfway between two neighbouring values of the dtype"""
    v = np.asarray(v, np.float64)
    p, emin, _ = FORMAT[dtype]
    a = np.abs(v)
    ulp = np.ldexp(1.0, np.maximum(np.frexp(a)[1] - 1, emin) - (p - 1))
    q = a / ulp
    return q - np.floor(q) == 0.5


def ks_expected(o, K, split, *, fused=True, rounding="nearest_even", truncate=True, leak_tag=0, X=None, **epi):
    """the bits a k_mfma_ks-family launch must give for operand set o: a torch tensor (n, M) of the
    plan dtype -- ks_model's fp32 value through epilogue_ref (the stages in fp32, one rounding by
    torch; fused = False: rounded to the dtype first).  epi as Plan.spmm takes it (residual M x n).
    rounding other than nearest_even (the host test's mutants): no epilogue, round_to"""
    A = o.A_codes if o.kind == "fp8" else o.A
    acc = ks_model(A, o.X if X is None else X, K, split, scale=o.scale, truncate=truncate, leak_tag=leak_tag)
    if rounding != "nearest_even":
        assert fused and not epi
        return torch.from_numpy(round_to(acc.astype(np.float64), o.dtype, rounding)).to(TORCH_DT[o.dtype])
    return epilogue_ref(acc.T.astype(np.float64), o.dtype, fused, **epi).t().contiguous()


def tie_counts(kind, K, split):
    """((token, row) results of a linear at 40 tokens, how many of their fp32 values sit on a tie)"""
    o = operands_for(kind, K, split)
    acc = ks_model(o.A_codes if kind == "fp8" else o.A, o.X, K, split, scale=o.scale).astype(np.float64)
    return acc.size, int(on_tie(acc, o.dtype).sum())


# ------------------------------------------------------------------ the epilogue rungs (f16)
def epilogue_cases(o, n):
    """[(name, epi)] for operand set o at n tokens, epi as Plan.spmm takes it: bias 2^-11 on the two
    epilogue rows (accumulator 1 + 2^-12: fused 1 + 2^-10, rounded twice 1), the same as a residual,
    and alpha = 0.5 (the subnormal rungs: 1.25 subnormal ulps halve to 2^-24 fused, to 0 rounded twice)"""
    rows = [o.rows["epilogue, two ranges"], o.rows["epilogue, one range"]]
    bias = torch.zeros(KS_M)
    bias[rows] = 2.0 ** -11
    res = torch.zeros((KS_M, n), dtype=TORCH_DT[o.dtype])
    res[rows] = 2.0 ** -11
    return [("bias", {"bias": bias}), ("residual", {"residual": res}), ("alpha", {"alpha": 0.5})]


# ------------------------------------------------------------------ the transposed product (SparseLinear's backward)
def grad_operands(o, n=32):
    """the incoming gradient (n, M) for x.grad = G @ A on plan_T: the tie's three products 1, 2^-11 and
    2^-22, times 2^10 so that every value stays a normal f16 one, carried by three filler rows of A
    (entries +-1, +-2), one per 32-row k-step of plan_T -- so x.grad[t, c] = 2^10 (+-a +- b 2^-11 +- c 2^-22)
    with a, b, c in {0, 1, 2}: ties at 2^10 (1 + 2^-11) and 2^10 (2 + 2^-10).  Tokens n - 8 .. n - 1 are
    scaled as X's tokens 32 .. 39"""
    G = np.zeros((n, KS_M), np.float64)
    s = np.concatenate([np.ones(n - 8), TOKEN_SCALE[32:]])
    for r, g in zip(GRAD_ROWS, (2.0 ** 10, 2.0 ** -1, 2.0 ** -12)):
        G[:, r] = s * g
    return G


def subsets(terms):
    """every non-empty subset of a short list"""
    return itertools.chain.from_iterable(itertools.combinations(terms, k) for k in range(1, len(terms) + 1))
