"""GPU checks of the token-major linear (Plan.linear / gs_linear: Y = epilogue(X A^T), X: n x K,
Y: n x M): the single launch k_mfma_ks_tm on k_mfma_ks plans of 17 .. 32 tokens, and the
three-launch path (k_tm_in, the plan's SpMM, k_tm_out) behind every other plan, width and alignment.

The operands are the integer ones of tests/test_gpu_edges.py and tests/test_gpu_epilogue.py (A in
{-2, -1, 1, 2}, X in {-2 .. 2}, integer bias and residual, alpha in {1, 0.5, -2}): every stage is
exact in fp32, so Y must equal epilogue_ref(prod, ...).T bit for bit -- from the exact product where
linear_fused(n) is 1 (one rounding), from the product rounded to the plan dtype where it is 0 (the
family rounds, k_tm_out rounds again).  X, Y and the residual are guarded (tests/guarded.py): NaN
bands around X and the residual, so a read outside them poisons Y; a fixed pattern around Y.  Every
launch is repeated into the NaN-refilled Y, and plan.device_status() must be clean."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C, int_values  # noqa: E402
from test_gpu_edges import (DEV, EDGE_K, PIPE_PARAMS, TORCH_DT, build, dense_f64, edge_dense, edge_matrix,  # noqa: E402
                            int_B_cpu)
from test_gpu_edges_mfma import KS_M, ks_pattern, ks_ranges, mfma_everywhere  # noqa: E402,F401  (fixture)
from test_gpu_epilogue import config, epilogue_ref, stage_sets  # noqa: E402

pytestmark = pytest.mark.gpu

# (KS_SPLIT, K).  K = 40: two k-steps, the second with one 16-byte unit below K, six of the eight
# waves without a step; K = 1176: 37 steps, a 24-column tail, waves with 5 and 4 steps (around
# 2 * depth), three K ranges; K = 1184: no tail
FUSED_CASES = [(1, 40), (2, 40), (3, 1176), (1, 1184), (2, 1184)]


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def ks_operands(K, n, dtype, M=KS_M):
    """(X: n x K on the CPU, the exact product A X^T: M x n); M < 131 takes the pattern's first rows"""
    B = int_B_cpu(K, n, dtype, seed=1)
    prod = ks_pattern(K)[3][:M] @ B.double().numpy()
    assert np.abs(prod).max() <= 1024
    return B.t().contiguous(), prod


def ks_plan(K, n, dtype, split, M=KS_M, **over):
    row, col, val, _ = ks_pattern(K)
    keep = row < M
    return build(M, K, row[keep], col[keep], val[keep], "block_total", 40, 1, n, dtype, over=dict(over, KS_SPLIT=split))


def run_linear(plan, X_cpu, prod, dtype, epi, what, fused, replica=0):
    """one guarded Plan.linear and a relaunch into the NaN-refilled Y: bit-exact against
    epilogue_ref(...).T, every guard band intact; returns Y's bits (a CPU copy).  epi: the epilogue as
    spmm takes it (residual M x n); linear gets the residual transposed"""
    M, n = prod.shape
    ref = epilogue_ref(prod, dtype, fused, **epi).t().contiguous().to(DEV)
    X, hx = guarded_B(X_cpu, DEV)
    Y, hy = guarded_C(n, M, TORCH_DT[dtype], DEV)
    kw = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in epi.items()}
    hr = None
    if "residual" in epi:
        kw["residual"], hr = guarded_B(epi["residual"].t().contiguous(), DEV)
    out = None
    for again in ("", " relaunch"):
        got = plan.linear(X, out=Y, replica=replica, **kw)
        assert got is Y
        torch.cuda.synchronize()
        plan.device_status()
        assert_bits(Y, ref, what + again)
        assert_guards_intact(hy, what + again + " Y")
        assert_guards_intact(hx, what + again + " X")
        if hr is not None:
            assert_guards_intact(hr, what + again + " residual")
        out = Y.cpu().clone()
        hy.refill()
    return out


# ------------------------------------------------------------------ 1: fused, exact
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("split,K", FUSED_CASES)
def test_fused_exact(split, K, dtype, mfma_everywhere):
    """k_mfma_ks_tm on the uploaded k_mfma_ks plan: n = 32 (a full tile: the fast iterations) with
    KS_NT 0 and 1, n = 24 (a partial tile: the general form, 8 tokens never stored), every stage set;
    M = 131: odd tokens' rows of Y are not 8-byte aligned (2-byte stores), the last block has 11 rows"""
    for n, nt in ((32, 0), (32, 1), (24, 0)):
        X, prod = ks_operands(K, n, dtype)
        plan = ks_plan(K, n, dtype, split, KS_NT=nt)
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split), info
        assert info["ks_nt"] == nt and plan.linear_fused(n) == 1, info
        for name, epi in stage_sets(KS_M, n, dtype):
            run_linear(plan, X, prod, dtype, epi, f"k_mfma_ks_tm {dtype} K={K} n={n} KS_SPLIT={split} KS_NT={nt} {name}", True)
        plan.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fused_exact_aligned_rows(dtype, mfma_everywhere):
    """M = 120 (the pattern's rows below 120): every row block is full and every store address is
    8-byte aligned, so every store is the 8-byte one"""
    split, K, n, M = 3, 1176, 32, 120
    X, prod = ks_operands(K, n, dtype, M)
    plan = ks_plan(K, n, dtype, split, M)
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == 3 and info["rows"] == M and plan.linear_fused(n) == 1, info
    for name, epi in stage_sets(M, n, dtype):
        run_linear(plan, X, prod, dtype, epi, f"k_mfma_ks_tm {dtype} M=120 {name}", True)
    plan.free()


# ------------------------------------------------------------------ 2: the same bits as spmm
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("split,K", [(3, 1176), (1, 1184)])
def test_same_bits_as_spmm(split, K, dtype, mfma_everywhere):
    """random normal values in A and X: the two kernels run the same MFMAs in the same order and
    combine in the same order, so linear(x) is spmm(x.T).T bit for bit; a difference is a bug in the
    fragment or store mapping"""
    n = 32
    row, col, _, _ = ks_pattern(K)
    rng = np.random.default_rng(7 + K)
    val = rng.standard_normal(len(row)).astype(np.float32)
    plan = build(KS_M, K, row, col, val, "block_total", 40, 1, n, dtype, over={"KS_SPLIT": split})
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split) and plan.linear_fused(n) == 1, info
    x = torch.from_numpy(rng.standard_normal((n, K)).astype(np.float32)).to(TORCH_DT[dtype]).to(DEV)
    y = plan.linear(x)
    c = plan.spmm(x.t().contiguous())
    torch.cuda.synchronize()
    plan.device_status()
    assert tuple(y.shape) == (n, KS_M) and not bool(torch.isnan(y).any())
    assert_bits(y, c.t().contiguous(), f"linear against spmm {dtype} K={K} KS_SPLIT={split}")
    plan.free()


# ------------------------------------------------------------------ 3: containment
def test_a_nan_token_stays_in_its_row(mfma_everywhere):
    """row j of X all NaN: row j of Y is NaN, every other row the reference's bits -- a token's unit
    never reaches another token's fragment; with the NaN band behind X's last element this also
    catches a read past K in the tail step (K = 1176: 24 columns)"""
    split, K, n, dtype = 3, 1176, 32, "f16"
    X_cpu, prod = ks_operands(K, n, dtype)
    plan = ks_plan(K, n, dtype, split)
    assert plan.info()["device_kernel"] == "k_mfma_ks" and plan.linear_fused(n) == 1, plan.info()
    ref = epilogue_ref(prod, dtype, True).t().contiguous().to(DEV)
    for j in (0, 17, 31):
        Xj = X_cpu.clone()
        Xj[j] = float("nan")
        X, hx = guarded_B(Xj, DEV)
        Y, hy = guarded_C(n, KS_M, TORCH_DT[dtype], DEV)
        plan.linear(X, out=Y)
        torch.cuda.synchronize()
        plan.device_status()
        keep = [i for i in range(n) if i != j]
        assert bool(torch.isnan(Y[j]).all()), j
        assert_bits(Y[keep].contiguous(), ref[keep].contiguous(), f"NaN token {j}: the other rows")
        assert_guards_intact(hy, f"NaN token {j} Y")
        assert_guards_intact(hx, f"NaN token {j} X")
    plan.free()


# ------------------------------------------------------------------ 4: the three-launch path
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("pipeline", gsa.PIPELINES)
def test_every_family_takes_the_three_launches(pipeline, dtype):
    """each pipeline of gsa.PIPELINES on the 131 x 203 edge pattern (gather side), the full
    epilogue, n = 5 and n = 32 (K = 203: every tile of both transposes is partial somewhere)"""
    p0, p1 = PIPE_PARAMS[pipeline]
    M, K, row, col, val, long_rows = edge_matrix(pipeline)
    for n in (5, 32):
        B = int_B_cpu(EDGE_K, n, dtype)
        prod = (edge_dense(long_rows) @ B.double().numpy())[:M]
        plan = build(M, K, row, col, val, pipeline, p0, p1, n, dtype, over={"MFMA_TILES": 0})
        try:
            assert plan.linear_fused(n) == 0, plan.info()
            epi = dict(stage_sets(M, n, dtype))["all"]
            run_linear(plan, B.t().contiguous(), prod, dtype, epi,
                       f"{pipeline}({p0},{p1}) {dtype} n={n} {plan.info()['device_kernel']}", False)
        finally:
            plan.free()


def full_epilogue(M, n, dtype):
    return dict(stage_sets(M, n, dtype))["all"]


def test_ks_plans_the_kernel_does_not_cover_take_the_three_launches(mfma_everywhere):
    """k_mfma_ks plans outside k_mfma_ks_tm's conditions report 0 and are correct: K % 8 != 0, a
    token count other than the plan's width (72: the gather side), window positions (KS_WPOS)"""
    dtype = "f16"
    K = 33
    plan = ks_plan(K, 32, dtype, 1)
    assert plan.info()["device_kernel"] == "k_mfma_ks", plan.info()
    for n in (32, 72):
        X, prod = ks_operands(K, n, dtype)
        assert plan.linear_fused(n) == 0
        run_linear(plan, X, prod, dtype, full_epilogue(KS_M, n, dtype), f"K=33 n={n}", False)
    plan.free()
    K, n = 1184, 32
    X, prod = ks_operands(K, n, dtype)
    plan = ks_plan(K, n, dtype, 2, KS_WPOS=1)
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ks_wpos"] == 1 and plan.linear_fused(n) == 0, info
    run_linear(plan, X, prod, dtype, full_epilogue(KS_M, n, dtype), "KS_WPOS", False)
    plan.free()


def test_mfma_rows_takes_the_three_launches(mfma_everywhere):
    K, n, dtype = 640, 64, "f16"
    row, col, val, dense = ks_pattern(K)
    B = int_B_cpu(K, n, dtype, seed=1)
    prod = dense @ B.double().numpy()
    plan = build(KS_M, K, row, col, val, "block_total", 20, 1, n, dtype)
    assert plan.info()["device_kernel"] == "k_mfma_rows" and plan.linear_fused(n) == 0, plan.info()
    run_linear(plan, B.t().contiguous(), prod, dtype, full_epilogue(KS_M, n, dtype), "k_mfma_rows", False)
    plan.free()


def test_divided_plan_takes_the_three_launches():
    """a row-divided plan (two sub-matrix kernels) between the two transposes"""
    K, n, dtype = 640, 32, "f16"
    row, col, val, dense = ks_pattern(K)
    B = int_B_cpu(K, n, dtype, seed=1)
    prod = dense @ B.double().numpy()
    plan = gsa.Plan.from_coo(KS_M, K, row, col, val)
    with config(MFMA_TILES=0):
        for i, s in enumerate(plan.divide_rows(80)):
            plan.run_pipeline("merge_path" if i % 2 else "tblock_warp_total", n, 64 if i % 2 else 16, 1 if i % 2 else 2, sub=s)
        plan.compile().upload(dtype, 0)
    assert plan.info()["n_kernels"] == 2 and plan.linear_fused(n) == 0, plan.info()
    run_linear(plan, B.t().contiguous(), prod, dtype, full_epilogue(KS_M, n, dtype), "divided plan", False)
    plan.free()


# ------------------------------------------------------------------ 5: fused == three launches when nothing rounds twice
@pytest.mark.parametrize("split,K", FUSED_CASES)
def test_fused_equals_three_launches_on_exact_products(split, K, mfma_everywhere):
    """fp16 with |A X^T| <= 2048 (integers fp16 holds exactly): LINEAR_FUSE 1 and 0 give one Y"""
    n, dtype = 32, "f16"
    X, prod = ks_operands(K, n, dtype)
    assert np.abs(prod).max() <= 2048
    plan = ks_plan(K, n, dtype, split)
    assert plan.info()["device_kernel"] == "k_mfma_ks" and plan.info()["ksplit"] == ks_ranges(K, split), plan.info()
    for name, epi in stage_sets(KS_M, n, dtype):
        what = f"K={K} KS_SPLIT={split} {name}"
        assert plan.linear_fused(n) == 1
        a = run_linear(plan, X, prod, dtype, epi, what + " fused", True)
        with config(LINEAR_FUSE=0):
            assert plan.linear_fused(n) == 0
            b = run_linear(plan, X, prod, dtype, epi, what + " three launches", False)
        assert_bits(a, b, what + ": fused against three launches")
    plan.free()


# ------------------------------------------------------------------ 6: one rounding when fused
@pytest.mark.parametrize("split", [1, 2])
def test_fused_rounds_once(split, mfma_everywhere):
    """tests/test_gpu_epilogue.py's construction: output feature 5 sums to 2049 exactly; with bias
    -2048 the fused store writes fp16(2049 - 2048) = 1, the three launches fp16(fp16(2049) - 2048) = 0"""
    M, K, n, R = 48, 544, 32, 5
    rng = np.random.default_rng(3)
    mask = rng.random((M, K)) < 0.05
    mask[R] = False
    mask[R, :513] = True
    r, c = np.nonzero(mask)
    row, col = r.astype(np.uint64), c.astype(np.uint64)
    val = int_values(len(row), 5)
    val[r == R] = 2.0
    val[(r == R) & (c == 512)] = 1.0
    B = int_B_cpu(K, n, "f16", seed=3).clone()
    B[:512] = 2
    B[512] = 1
    prod = dense_f64(M, K, row, col, val) @ B.double().numpy()
    assert (prod[R] == 2049).all() and np.abs(prod).max() == 2049
    bias = torch.zeros(M)
    bias[R] = -2048.0
    plan = build(M, K, row, col, val, "block_total", 48, 1, n, "f16", over={"KS_SPLIT": split})
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == split and plan.linear_fused(n) == 1, info
    X = B.t().contiguous()
    once = run_linear(plan, X, prod, "f16", {"bias": bias}, f"fused, {split} K ranges", True)
    assert (once[:, R] == 1.0).all(), once[:, R]
    with config(LINEAR_FUSE=0):
        assert plan.linear_fused(n) == 0
        twice = run_linear(plan, X, prod, "f16", {"bias": bias}, f"three launches, {split} K ranges", False)
    assert (twice[:, R] == 0.0).all(), twice[:, R]
    assert plan.linear_fused(n) == 1
    plan.free()


# ------------------------------------------------------------------ 7: refusals
@pytest.mark.parametrize("fuse", [1, 0])
def test_refusals_leave_out_untouched(fuse, mfma_everywhere):
    K, n, dtype = 40, 32, "f16"
    X_cpu, _ = ks_operands(K, n, dtype)
    plan = ks_plan(K, n, dtype, 2)
    x = X_cpu.to(DEV)
    big = torch.full((n + 1, KS_M), 7.0, dtype=torch.float16, device=DEV)
    out = big[:n]
    bias = torch.zeros(KS_M, device=DEV)
    res = torch.zeros((n, KS_M), dtype=torch.float16, device=DEV)
    wide = torch.zeros((n, 2 * K), dtype=torch.float16, device=DEV)
    bad = [
        ("x is (K, n)", ValueError, dict(x=x.t().contiguous())),
        ("x non-contiguous", ValueError, dict(x=wide[:, :K])),
        ("x dtype", TypeError, dict(x=x.float())),
        ("out is (M, n)", ValueError, dict(out=torch.full((KS_M, n), 7.0, dtype=torch.float16, device=DEV))),
        ("residual is (M, n)", ValueError, dict(residual=res.t().contiguous())),
        ("residual is out", ValueError, dict(residual=out)),
        ("residual overlaps out", ValueError, dict(residual=big[1:])),
        ("bias with n entries", ValueError, dict(bias=torch.zeros(n, device=DEV))),
        ("activation", ValueError, dict(activation="gelu")),
        ("alpha", ValueError, dict(alpha=float("nan"))),
    ]
    with config(LINEAR_FUSE=fuse):
        assert plan.linear_fused(n) == fuse
        for what, exc, kw in bad:
            args = dict(x=x, out=out)
            args.update(kw)
            xx = args.pop("x")
            with pytest.raises(exc):
                plan.linear(xx, **args)
            torch.cuda.synchronize()
            assert bool((big == 7.0).all()) and bool((args["out"] == 7.0).all()), what
        with pytest.raises(gsa.GsError):  # the C ABI's own check: the replica, before any launch
            plan.linear(x, out=out, replica=3)
        torch.cuda.synchronize()
        assert bool((big == 7.0).all())
        # and the accepted call still works on the same operands
        plan.linear(x, out=out, bias=bias, residual=res)
        torch.cuda.synchronize()
        assert not bool((out == 7.0).all(1).any()) and bool((big[n] == 7.0).all())  # every row of out written
    plan.free()


# ------------------------------------------------------------------ 8: the module
def test_sparse_linear_module(mfma_everywhere):
    """from_dense on a pruned 131 x 1184 weight with bias and relu; forward on (2, 16, 1184) is
    Plan.linear on the flattened input, bit for bit"""
    K, dtype = 1184, "f16"
    row, col, val, dense = ks_pattern(K)
    weight = torch.from_numpy(dense).float()
    bias = torch.arange(KS_M, dtype=torch.float32) - 60.0
    layer = gsa.SparseLinear.from_dense(weight, bias, tokens=32, dtype=dtype, activation="relu")
    assert isinstance(layer, torch.nn.Module)
    info = layer.plan.info()
    assert (info["rows"], info["cols"], info["nnz"]) == (KS_M, K, len(row)) and info["device_kernel"] == "k_mfma_ks", info
    assert "k_mfma_ks" in repr(layer) and "linear_fused(32)=1" in repr(layer), repr(layer)
    x = int_B_cpu(K, 32, dtype, seed=1).t().contiguous().reshape(2, 16, K).to(DEV)
    y = layer(x)
    flat = layer.plan.linear(x.reshape(32, K), bias=bias.to(DEV), activation="relu")
    torch.cuda.synchronize()
    layer.plan.device_status()
    assert tuple(y.shape) == (2, 16, KS_M) and y.dtype == torch.float16
    assert_bits(y.reshape(32, KS_M), flat, "SparseLinear.forward against Plan.linear")
    prod = dense @ x.reshape(32, K).t().cpu().double().numpy()
    assert_bits(flat.cpu(), epilogue_ref(prod, dtype, True, bias=bias, activation="relu").t().contiguous(), "against the reference")
    with pytest.raises(RuntimeError, match="inference"):
        layer(x.clone().requires_grad_())
    with torch.no_grad():
        layer(x.clone().requires_grad_())
    layer.plan.free()
