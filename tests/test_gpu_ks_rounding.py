"""GPU checks of the final rounding and of the K-split truncation in k_mfma_ks, k_mfma_ks_w8 and
k_mfma_ks_tm, on the rounding rungs of tests/ks_rounding.py: operands whose 16-bit result is decided
by the lowest fp32 bit of a K-range partial sum (a tie to even in either direction, just above a tie,
2049 / 2051, the overflow tie 65520, the subnormal ties), every partial sum exact in fp32 whatever the
summation order (tests/test_ks_rounding_host.py).  So every comparison is bit for bit against
ks_expected: the float64 product per K range, bit 0 of its fp32 encoding cleared where the plan has
more than one range (the slab's validity tag), the ranges added in order, one rounding.

A reader that left the tag in a partial, a tag that is set in one launch and clear in the next, a
truncating or half-away conversion, a scale applied after the rounding or a second rounding each move
a rung (the host test's mutants).  Plans are built as ks_plan / fp8_plan build them, operands are
guarded (tests/guarded.py), every launch is repeated into the NaN-refilled output -- consecutive
launches of a plan alternate the tag -- and followed by plan.device_status()."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
import ks_rounding as kr  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C  # noqa: E402
from test_gpu_edges import DEV, TORCH_DT, build  # noqa: E402
from test_gpu_edges_mfma import KS_M, ks_ranges, mfma_everywhere  # noqa: E402,F401  (fixture)
from test_gpu_epilogue import config  # noqa: E402
from test_gpu_fp8 import fp8_plan  # noqa: E402

pytestmark = pytest.mark.gpu


def rung_plan(o, K, split):
    """the plan of operand set o at KS_SPLIT = split, N = 32, 40-row blocks; checked to be what the rungs assume"""
    if o.kind == "fp8":
        plan = fp8_plan(KS_M, K, o.row, o.col, o.val, 32, split, row_scale=o.scale)
    else:
        plan = build(KS_M, K, o.row, o.col, o.val, "block_total", 40, 1, 32, o.dtype, over={"KS_SPLIT": split})
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split), info
    assert info["weights"] == (1 if o.kind == "fp8" else 0), info
    for n in (32, 40):
        assert plan.linear_fused(n) == 1, (n, info)
    assert plan.epilogue_fused(32) == 1
    return plan


def twice(plan, launch, out, h_out, h_in, ref, what):
    """a launch and a relaunch into the NaN-refilled output (the other tag value where the plan has K
    ranges): the model's bits both times, the guard bands intact, a clean device status; returns the bits"""
    ref = ref.to(DEV)
    got = None
    for again in ("", " relaunch"):
        launch()
        torch.cuda.synchronize()
        plan.device_status()
        assert_bits(out, ref, what + again)
        assert_guards_intact(h_out, what + again + " out")
        for h in h_in:
            assert_guards_intact(h, what + again + " in")
        got = out.cpu().clone()
        h_out.refill()
    return got


def run_linear(plan, o, n, ref, what, **epi):
    """Plan.linear on tokens 0 .. n - 1, twice; epi as Plan.spmm takes it (residual M x n)"""
    td = TORCH_DT[o.dtype]
    X, hx = guarded_B(o.X_t[:n].contiguous(), DEV)
    Y, hy = guarded_C(n, KS_M, td, DEV)
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in epi.items()}
    holders = [hx]
    if "residual" in epi:
        kw["residual"], hr = guarded_B(epi["residual"].t().contiguous(), DEV)
        holders.append(hr)
    return twice(plan, lambda: plan.linear(X, out=Y, **kw), Y, hy, holders, ref, what)


def run_spmm(plan, o, ref, what, **epi):
    """Plan.spmm at N = 32 with B = X[:32].T, twice; ref as linear's (n, M)"""
    B, hb = guarded_B(o.X_t[:32].t().contiguous(), DEV)
    C, hc = guarded_C(KS_M, 32, TORCH_DT[o.dtype], DEV)
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in epi.items()}
    return twice(plan, lambda: plan.spmm(B, C=C, **kw), C, hc, [hb], ref.t().contiguous(), what)


# ------------------------------------------------------------------ 1: the rungs, per plan
@pytest.mark.parametrize("K,split", kr.CASES)
@pytest.mark.parametrize("kind", kr.KINDS)
def test_rungs(kind, K, split, mfma_everywhere):
    """linear at 32 tokens, spmm at N = 32 (the same bits, transposed), linear at 40 tokens (two token
    tiles, the second partial and with the scaled tokens), each twice in a row, on one replica"""
    o = kr.operands_for(kind, K, split)
    plan = rung_plan(o, K, split)
    what = f"{kind} K={K} KS_SPLIT={split}"
    want = kr.ks_expected(o, K, split)
    y = run_linear(plan, o, 32, want[:32].contiguous(), what + " linear n=32")
    c = run_spmm(plan, o, want[:32].contiguous(), what + " spmm N=32")
    assert_bits(c.t().contiguous(), y, what + ": spmm(x.T).T against linear(x)")
    run_linear(plan, o, 40, want, what + " linear n=40")
    plan.free()


# ------------------------------------------------------------------ 2: one rounding under an epilogue
@pytest.mark.parametrize("split", [1, 3])
def test_epilogue_rungs(split, mfma_everywhere):
    """f16, K = 1176: accumulator 1 + 2^-12 with bias 2^-11 (and with the same as a residual) is
    1 + 2^-10 rounded once and 1 rounded twice; alpha = 0.5 on the subnormal rungs.  Fused at 32 and 40
    tokens and in spmm; under LINEAR_FUSE = 0 (three launches: the SpMM rounds, k_tm_out rounds again)
    at 32 tokens against the reference rounded twice"""
    K = 1176
    o = kr.operands_for("f16", K, split)
    plan = rung_plan(o, K, split)
    for n in (32, 40):
        for name, epi in kr.epilogue_cases(o, n):
            what = f"K={K} KS_SPLIT={split} n={n} {name}"
            once = kr.ks_expected(o, K, split, fused=True, X=o.X[:n], **epi)
            y = run_linear(plan, o, n, once, what + " fused", **epi)
            rows = [o.rows["epilogue, two ranges"], o.rows["epilogue, one range"]]
            if name != "alpha":
                assert bool((y[:32, rows] == 1 + 2.0 ** -10).all()), y[:32, rows]
            if n == 32:
                run_spmm(plan, o, once, what + " fused spmm", **epi)
                with config(LINEAR_FUSE=0):
                    assert plan.linear_fused(n) == 0
                    ref = kr.ks_expected(o, K, split, fused=False, X=o.X[:n], **epi)
                    t = run_linear(plan, o, n, ref, what + " three launches", **epi)
                if name != "alpha":
                    assert bool((t[:, rows] == 1.0).all()), t[:, rows]
                assert plan.linear_fused(n) == 1
    plan.free()


# ------------------------------------------------------------------ 3: the module, forward and grad_x
def test_sparse_linear_rungs(mfma_everywhere):
    """SparseLinear.from_dense on the f16 rung weight (the K ranges its own: KS_SPLIT as configured):
    forward at 40 tokens is the model at the plan's ksplit; with grad="input", x.grad for the gradient
    of ks_rounding.grad_operands is the model of plan_T -- A.T at plan_T's own ksplit"""
    K, n = 1176, 32
    o = kr.operands("f16", K)
    layer = gsa.SparseLinear.from_dense(torch.tensor(o.A, dtype=torch.float32), tokens=32, dtype="f16", grad="input")
    info = layer.plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["nnz"] == len(o.row) and layer.plan.linear_fused(40) == 1, info
    split = kr.split_of(K, info["ksplit"])
    with torch.no_grad():
        y = layer(o.X_t.to(DEV))
    torch.cuda.synchronize()
    layer.plan.device_status()
    assert_bits(y.cpu(), kr.ks_expected(o, K, split), f"SparseLinear forward, {info['ksplit']} K ranges")
    layer.prepare_backward()
    ti = layer.plan_T.info()
    if ti["device_kernel"] != "k_mfma_ks":
        layer.plan.free(), layer.plan_T.free()
        pytest.skip(f"plan_T of this weight runs {ti['device_kernel']}, not k_mfma_ks: the model does not describe it")
    G = kr.grad_operands(o, n)
    acc = kr.ks_model(o.A.T, G, KS_M, kr.split_of(KS_M, ti["ksplit"]))
    want = torch.from_numpy(kr.round_to(acc.astype(np.float64), "f16")).to(torch.float16)
    assert bool((want == torch.from_numpy(acc.astype(np.float64)).to(torch.float16)).all())
    x = o.X_t[:n].to(DEV).requires_grad_()
    out = layer(x)
    out.backward(torch.from_numpy(G).to(torch.float16).to(DEV))
    torch.cuda.synchronize()
    layer.plan.device_status()
    layer.plan_T.device_status()
    assert_bits(out.detach().cpu(), kr.ks_expected(o, K, split)[:n].contiguous(), "SparseLinear forward under grad")
    assert_bits(x.grad.cpu(), want, f"x.grad on plan_T, {ti['ksplit']} K ranges")
    layer.plan.free(), layer.plan_T.free()
