"""CPU checks that the rounding rungs of tests/ks_rounding.py mean what they claim: every partial sum
is exact in fp32 whatever the summation order, every MFMA holds at most one non-zero product, the
model gives the tabled results, and each way a kernel could be subtly wrong (no truncation, a leaked
tag, a truncating or round-half-away conversion, a second rounding) moves at least one result in the
first token tile and one in the second."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
import ks_rounding as kr  # noqa: E402
from test_gpu_edges import TORCH_DT  # noqa: E402
from test_gpu_edges_mfma import KS_M, ks_ranges  # noqa: E402

INF = float("inf")
# rung -> (result with one K range, result with three), token 0.  None: the rung needs three ranges
TABLE = {
    "f16": {
        "tie to even, down": (1.0, 1.0),
        "negative: tie to even, down": (-1.0, -1.0),
        "tie to even, up": (1 + 2.0 ** -9, 1 + 2.0 ** -9),
        "above the tie, one range": (1 + 2.0 ** -10, 1.0),  # three ranges: the bit is dropped
        "above the tie, across ranges": (1 + 2.0 ** -10, 1 + 2.0 ** -10),
        "2049": (2048.0, 2048.0),
        "2051": (2052.0, 2052.0),
        "65520": (INF, INF),
        "just under 65520": (65504.0, 65504.0),
        "subnormal tie": (2.0 ** -23, 2.0 ** -23),
        "2^-25": (0.0, 0.0),
        "just above 2^-25": (2.0 ** -24, 2.0 ** -24),
        # (1 + 2^-23 | 1 + 2^-23 | 2^-10 + 2^-33) x 2^6: truncated 2^6 (2 + 2^-10), a tie, to even
        "odd partials in all three ranges": (None, 128.0),
        # beyond the issue's table
        "negative: above the tie, one range": (-1 - 2.0 ** -10, -1.0),
        "negative: 65520": (-INF, -INF),
        "negative: 2^-25": (-0.0, -0.0),
        "tie in the last k-step": (1.0, 1.0),
        "above the tie, three ranges": (1 + 2.0 ** -10, 1 + 2.0 ** -10),
        "1.25 subnormal ulps": (2.0 ** -24, 2.0 ** -24),
        "epilogue, two ranges": (1.0, 1.0),
        "epilogue, one range": (1.0, 1.0),
    },
    "bf16": {
        "tie to even, down": (1.0, 1.0),
        "negative: tie to even, down": (-1.0, -1.0),
        "tie to even, up": (1 + 2.0 ** -6, 1 + 2.0 ** -6),
        "above the tie, one range": (1 + 2.0 ** -7, 1.0),
        "above the tie, across ranges": (1 + 2.0 ** -7, 1 + 2.0 ** -7),
        "257": (256.0, 256.0),
        "259": (260.0, 260.0),
        "odd partials in all three ranges": (None, 128.0),
        "tie in the last k-step": (1.0, 1.0),
        "above the tie, three ranges": (1 + 2.0 ** -7, 1 + 2.0 ** -7),
    },
}
MUTANTS = [{"truncate": False}, {"leak_tag": 1}, {"rounding": "toward_zero"}, {"rounding": "half_away"}]


def bits(t):
    return t.contiguous().view(torch.int16)


def all_operand_sets():
    return [kr.operands(kind, K, three) for kind in kr.KINDS for K in kr.KS for three in (False, True)]


def test_the_cases_are_the_k_ranges_they_say():
    assert [ks_ranges(K, s) for K, s in kr.CASES] == [1, 3, 1, 2]
    assert kr.range_width(1176, 3) == kr.range_width(1184, 3) == 416 and kr.range_width(1184, 2) == 608
    assert 1176 - 1 - 2 * 416 >= 32 * 10 and 1176 % 32 == 24  # column K - 1 lies in the 24-column last step
    assert kr.split_of(1176, 3) == 3 and kr.split_of(131, 5) == 5


def test_rung_columns_and_values():
    """every rung column in a k-step of its own (so in a different k-step of its range at every split:
    ranges are whole k-steps), two or three per range of the three-range layout, column 0 and K - 1
    among them; every A and X value a normal value of the dtype that round-trips through it"""
    for o in all_operand_sets():
        cols = sorted(o.cols.values())
        assert cols[0] == 0 and cols[-1] == o.K - 1
        assert len({c // 32 for c in cols}) == len(cols) == 9
        for K, split in kr.CASES:
            if K == o.K:
                assert kr.range_width(K, split) % 32 == 0
                for sl in kr.range_slices(K, split):
                    steps = [(c - sl.start) // 32 for c in cols if sl.start <= c < sl.stop]
                    assert len(set(steps)) == len(steps)
        per_range = [sum(sl.start <= c < sl.stop for c in cols) for sl in kr.range_slices(o.K, 3)]
        assert per_range == [3, 3, 3]
        _, emin, vmax = kr.FORMAT[o.dtype]
        td = TORCH_DT[o.dtype]
        for name, a in (("A", o.val.astype(np.float64)), ("X", o.X[o.X != 0])):
            assert (np.abs(a) >= 2.0 ** emin).all() and (np.abs(a) <= vmax).all(), (o.kind, o.K, name)
            assert (torch.from_numpy(a).to(td).double().numpy() == a).all(), (o.kind, o.K, name)
        # the rungs' entries replaced the pattern's at the rung columns: a row without a term has no entry
        at = np.isin(o.col.astype(np.int64), cols)
        assert int(at.sum()) == sum(len(t) for _, t in o.rungs)
        assert (o.X[:32] == o.X[0]).all() and (o.X[:, [c for c in range(o.K) if c not in cols]] == 0).all()
        assert {float(s) for s in kr.TOKEN_SCALE[32:]} == {-1.0, 0.5, 8.0}
        # rows of every 40-row block, the 11-row one included
        assert {r // 40 for r in o.rows.values()} == {0, 1, 2, 3} and 130 in o.rows.values()


def test_order_independence():
    """for every (token, row) and every K range at every split: every subset sum of the range's products
    is an fp32 value -- so the wave split, the LDS reduction and the MFMAs' order cannot matter"""
    for o in all_operand_sets():
        A = o.A_codes if o.kind == "fp8" else o.A
        tokens = [0] + list(range(32, 40))
        for K, split in kr.CASES:
            if K != o.K or (o.three_ranges and ks_ranges(K, split) != 3):
                continue
            for sl in kr.range_slices(K, split):
                cols = [c for c in o.cols.values() if sl.start <= c < sl.stop]
                for sub in kr.subsets(cols):
                    s64 = o.X[tokens][:, list(sub)] @ A[:, list(sub)].T
                    assert (s64.astype(np.float32).astype(np.float64) == s64).all(), (o.kind, K, split, sub)
                    # and the float64 sum itself is exact: the products span far fewer than 53 bits
                    terms = np.abs(o.X[tokens][:, list(sub), None] * A[:, list(sub)].T[None])
                    hi = terms.max(1)
                    lo = np.where(terms > 0, terms, np.inf).min(1)
                    assert (hi[hi > 0] / lo[hi > 0] < 2.0 ** 48).all()


def test_fp8_values_are_exact_codes():
    for K in kr.KS:
        for three in (False, True):
            o = kr.operands("fp8", K, three)
            codes, scale = gsa.fp8_quantize(o.val, o.row, KS_M, row_scale=o.scale)
            np.testing.assert_array_equal(scale, o.scale)
            assert (np.frexp(scale)[0] == 0.5).all()
            back = gsa.fp8_decode(codes) * scale[o.row.astype(np.int64)]
            np.testing.assert_array_equal(back, o.val)
            np.testing.assert_array_equal(gsa.fp8_decode(codes), o.codes_val.astype(np.float32))
            f16 = kr.operands("f16", K, three)
            np.testing.assert_array_equal(o.val, f16.val)  # the same weight, the same X
            assert (o.X == f16.X).all()
            assert int((scale == 1).sum()) > 100 and o.scale[o.rows["65520"]] > o.scale[o.rows["2^-25"]]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_the_table(dtype):
    """the model at token 0 against the table; FP8 weights give the f16 column"""
    for kind in ([dtype, "fp8"] if dtype == "f16" else [dtype]):
        for (K, split), column in (((1176, 1), 0), ((1184, 1), 0), ((1176, 3), 1)):
            o = kr.operands_for(kind, K, split)
            got = kr.ks_expected(o, K, split)[0]
            names = [n for n, _ in o.rungs]
            for name, want in TABLE[dtype].items():
                if want[column] is None:
                    assert name not in names
                    continue
                w = torch.tensor([want[column]], dtype=TORCH_DT[dtype])
                g = got[o.rows[name]].reshape(1)
                assert bits(g).item() == bits(w).item(), (kind, K, split, name, g.item(), want[column])
            # rows without a rung are +0
            rest = [r for r in range(KS_M) if r not in o.rows.values()]
            assert (bits(got[rest]) == 0).all()


def test_round_to_is_torchs_rounding():
    """the host-side conversion the mutants use, in its nearest-even mode, against torch's .to(dtype)"""
    for kind, (K, split) in [(k, c) for k in kr.KINDS for c in kr.CASES]:
        o = kr.operands_for(kind, K, split)
        A = o.A_codes if kind == "fp8" else o.A
        acc = kr.ks_model(A, o.X, K, split, scale=o.scale).astype(np.float64)
        mine = torch.from_numpy(kr.round_to(acc, o.dtype)).to(TORCH_DT[o.dtype])
        assert (bits(mine) == bits(kr.ks_expected(o, K, split))).all()
    v = np.array([65519.9, 65520.0, -65520.0, 2.0 ** -25, 2.0 ** -25 * 1.001, 3 * 2.0 ** -25, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11])
    for mode, want in (("nearest_even", [65504, INF, -INF, 0, 2.0 ** -24, 2.0 ** -23, 1, 1 + 2.0 ** -9]),
                       ("toward_zero", [65504, 65504, -65504, 0, 0, 2.0 ** -24, 1, 1 + 2.0 ** -10]),
                       ("half_away", [65504, INF, -INF, 2.0 ** -24, 2.0 ** -24, 2.0 ** -23, 1 + 2.0 ** -10, 1 + 2.0 ** -9])):
        np.testing.assert_array_equal(kr.round_to(v, "f16", mode), np.array(want, np.float64))


@pytest.mark.parametrize("kind", kr.KINDS)
def test_discrimination(kind):
    """each mutated model differs from the true one in the tokens-0..31 tile and in tokens 32..39;
    the two K-split mutants differ only where there is more than one K range"""
    for K, split in kr.CASES:
        o = kr.operands_for(kind, K, split)
        true = bits(kr.ks_expected(o, K, split))
        for m in MUTANTS:
            diff = bits(kr.ks_expected(o, K, split, **m)) != true
            if ("truncate" in m or "leak_tag" in m) and ks_ranges(K, split) == 1:
                assert not bool(diff.any()), (kind, K, split, m)
                continue
            assert bool(diff[:32].any()) and bool(diff[32:].any()), (kind, K, split, m)
            assert bool((diff[:32] == diff[0]).all())  # (tokens 0 .. 31 are one token)
    # a plan with three K ranges against the same plan with one: only at a tie of the truncated sum
    o = kr.operands_for(kind, 1176, 1)
    one, three = kr.ks_expected(o, 1176, 1), kr.ks_expected(o, 1176, 3)
    differ = (bits(one) != bits(three)).numpy()
    A = o.A_codes if kind == "fp8" else o.A
    tie = kr.on_tie(kr.ks_model(A, o.X, 1176, 3, scale=o.scale).astype(np.float64), o.dtype)
    assert differ.any() and (tie[differ]).all()
    assert differ[0, o.rows["above the tie, one range"]]


def test_epilogue_discrimination():
    """fused against rounded twice, f16: they differ on both epilogue rows under the bias and under the
    residual, and on the 1.25-subnormal-ulps row under alpha = 0.5"""
    for K, split in ((1176, 1), (1176, 3)):
        o = kr.operands_for("f16", K, split)
        for n in (32, 40):
            for name, epi in kr.epilogue_cases(o, n):
                X = o.X[:n]
                once = kr.ks_expected(o, K, split, fused=True, X=X, **epi)
                twice = kr.ks_expected(o, K, split, fused=False, X=X, **epi)
                rows = [o.rows["1.25 subnormal ulps"]] if name == "alpha" else [o.rows["epilogue, two ranges"], o.rows["epilogue, one range"]]
                for r in rows:
                    assert bits(once[0, r:r + 1]).item() != bits(twice[0, r:r + 1]).item(), (K, split, name, r)
                if name != "alpha":
                    assert (once[:32, rows] == 1 + 2.0 ** -10).all() and (twice[:32, rows] == 1.0).all()
                else:
                    assert (once[:32, rows] == 2.0 ** -24).all() and (bits(twice[:32, rows]) == 0).all()
                    r = o.rows["subnormal tie"]  # (2^-24 + 2^-25) / 2: 0.75 subnormal ulps, up
                    assert (once[:32, r] == 2.0 ** -24).all()


def test_grad_operands():
    """the transposed product of the SparseLinear test: G's rows lie in different k-steps of plan_T, its
    values are normal f16 values, the model finds ties, and a leaked tag would move one at every split"""
    o = kr.operands("f16", 1176)
    G = kr.grad_operands(o)
    assert len({r // 32 for r in kr.GRAD_ROWS}) == 3 and not set(kr.GRAD_ROWS) & set(o.rows.values())
    g = G[G != 0]
    assert (np.abs(g) >= 2.0 ** -14).all() and (torch.from_numpy(g).half().double().numpy() == g).all()
    for ksplit in (1, 2, 3, 5):
        s = kr.split_of(KS_M, ksplit)
        acc = kr.ks_model(o.A.T, G, KS_M, s).astype(np.float64)
        assert kr.on_tie(acc[0], "f16").sum() > 20 and kr.on_tie(acc[-1], "f16").sum() > 20
        true = torch.from_numpy(kr.round_to(acc, "f16")).half()
        if ksplit > 1:
            leak = kr.ks_model(o.A.T, G, KS_M, s, leak_tag=1).astype(np.float64)
            assert bool((bits(torch.from_numpy(kr.round_to(leak, "f16")).half()) != bits(true)).any())


def test_tie_counts():
    """the figures the pull request's summary quotes: results compared per plan and how many sit on a tie"""
    for kind in kr.KINDS:
        for K, split in kr.CASES:
            n, ties = kr.tie_counts(kind, K, split)
            print(f"{kind} K={K} ksplit={ks_ranges(K, split)}: {n} results, {ties} on a tie")
            assert n == 40 * KS_M and ties >= 40
