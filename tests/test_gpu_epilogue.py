"""GPU checks of the SpMM epilogue (Plan.spmm's alpha / bias / activation / residual, gs_spmm_ex):
fused into k_mfma_ks's store, and as the post-pass k_epilogue behind every other family.

The exact tests use the integer operands and the guarded buffers of tests/test_gpu_edges.py
(A in {-2, -1, 1, 2}, B in {-2 .. 2}), alpha in {1, 0.5, -2}, integer bias in [-8, 8] and integer
residual in [-4, 4]: every stage is exact in fp32, the only rounding is the final one, so C must
equal the reference bit for bit -- after a relaunch into the NaN-refilled payload too, with both
guard bands intact.  The reference (epilogue_ref) is torch on the CPU, in fp32, in the order the
interface states: times alpha, plus bias[row], relu as (t < 0 ? 0 : t), plus residual, one rounding.
It starts from the exact product where plan.epilogue_fused(N) is 1 and from the product rounded to
the plan dtype where it is 0 (the family rounds, then the pass rounds again).  A zero accumulator
is +0, as every family's zero-initialised fp32 accumulators give."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
import tolerance  # noqa: E402
from generalsparse_amd import _lib  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C, int_values  # noqa: E402
from test_gpu_edges import (DEV, EDGE_K, PIPE_PARAMS, TORCH_DT, build, dense_f64, edge_dense, edge_matrix,  # noqa: E402
                            int_B_cpu)
from test_gpu_edges_mfma import KS_M, ks_pattern, mfma_everywhere  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ operands and the reference
@functools.lru_cache(maxsize=None)
def int_bias(M, seed=0):
    g = torch.Generator()
    g.manual_seed(31 * M + seed)
    return torch.randint(-8, 9, (M,), generator=g).float()


@functools.lru_cache(maxsize=None)
def int_residual(M, N, dtype, seed=0):
    g = torch.Generator()
    g.manual_seed(17 * M + N + seed)
    return torch.randint(-4, 5, (M, N), generator=g).to(TORCH_DT[dtype])


def epilogue_ref(prod, dtype, fused, alpha=1.0, bias=None, activation=None, residual=None):
    """the stages in fp32 on the CPU from the exact float64 product `prod` (numpy): from the exact
    value when the plan fuses, from the value rounded to the plan dtype when it does not"""
    acc = torch.from_numpy(np.asarray(prod, np.float64) + 0.0)  # a zero accumulator is +0
    if not fused:
        acc = acc.to(TORCH_DT[dtype])
    t = acc.to(torch.float32)
    assert bool((t.double() == acc.double()).all())  # the fp32 start value is exact
    t = t * torch.tensor(alpha, dtype=torch.float32)
    if bias is not None:
        t = t + bias.cpu()[:, None]
    if activation == "relu":
        t = torch.where(t < 0, torch.zeros_like(t), t)
    if residual is not None:
        t = t + residual.cpu().float()
    assert t.dtype == torch.float32
    return t.to(TORCH_DT[dtype])


def stage_sets(M, N, dtype):
    """every stage alone (alpha at each of its values) and all together"""
    bias, res = int_bias(M), int_residual(M, N, dtype)
    return [("alpha=1", {"alpha": 1.0}), ("alpha=0.5", {"alpha": 0.5}), ("alpha=-2", {"alpha": -2.0}),
            ("bias", {"bias": bias}), ("relu", {"activation": "relu"}), ("residual", {"residual": res}),
            ("all", {"alpha": -2.0, "bias": bias, "activation": "relu", "residual": res})]


def on_dev(epi):
    return {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in epi.items()}


def run_guarded_epilogue(plan, B_cpu, prod, dtype, epi, what, fused=None, replica=0):
    """one guarded launch with the epilogue and a relaunch into the NaN-refilled C: bit-exact, guard
    bands intact both times; returns C's bits (a CPU copy)"""
    M, N = prod.shape
    fused = plan.epilogue_fused(N) if fused is None else fused
    ref = epilogue_ref(prod, dtype, fused, **epi).to(DEV)
    B, hb = guarded_B(B_cpu, DEV)
    C, hc = guarded_C(M, N, TORCH_DT[dtype], DEV)
    dev_epi = on_dev(epi)
    for again in ("", " relaunch"):
        plan.spmm(B, C=C, replica=replica, **dev_epi)
        torch.cuda.synchronize()
        plan.device_status()
        assert_bits(C, ref, what + again)
        assert_guards_intact(hc, what + again + " C")
        assert_guards_intact(hb, what + again + " B")
        out = C.cpu().clone()
        hc.refill()
    return out


class config:
    """a config key set for a block"""

    def __init__(self, **over):
        self.over = over

    def __enter__(self):
        self.old = {k: gsa.get_config(k) for k in self.over}
        for k, v in self.over.items():
            gsa.set_config(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            gsa.set_config(k, v)


# ------------------------------------------------------------------ 1: every family, post-pass
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("pipeline", gsa.PIPELINES)
def test_every_family_takes_the_post_pass(pipeline, dtype):
    """each pipeline of gsa.PIPELINES on the 131 x 203 edge pattern (tests/test_gpu_edges.py's
    parameters and gather-side setting; the long-row variant for the col-direction pipelines), the
    full epilogue, N = 5 (scalar accesses) and N = 32 (16-byte accesses)"""
    p0, p1 = PIPE_PARAMS[pipeline]
    M, K, row, col, val, long_rows = edge_matrix(pipeline)
    for N in (5, 32):
        B = int_B_cpu(EDGE_K, N, dtype)
        prod = (edge_dense(long_rows) @ B.double().numpy())[:M]
        plan = build(M, K, row, col, val, pipeline, p0, p1, N, dtype, over={"MFMA_TILES": 0})
        try:
            assert plan.epilogue_fused(N) == 0, plan.info()
            epi = dict(stage_sets(M, N, dtype))["all"]
            run_guarded_epilogue(plan, B, prod, dtype, epi, f"{pipeline}({p0},{p1}) {dtype} N={N} {plan.info()['device_kernel']}")
        finally:
            plan.free()


def test_mfma_rows_takes_the_post_pass(mfma_everywhere):
    """k_mfma_rows is not fused: only k_mfma_ks is"""
    K, N, dtype = 640, 64, "f16"
    row, col, val, dense = ks_pattern(K)
    B = int_B_cpu(K, N, dtype, seed=1)
    prod = dense @ B.double().numpy()
    plan = build(KS_M, K, row, col, val, "block_total", 20, 1, N, dtype)
    assert plan.info()["device_kernel"] == "k_mfma_rows" and plan.epilogue_fused(N) == 0, plan.info()
    run_guarded_epilogue(plan, B, prod, dtype, dict(stage_sets(KS_M, N, dtype))["all"], "k_mfma_rows")
    plan.free()


def test_divided_plan_takes_the_post_pass():
    """a row-divided plan (two sub-matrix kernels): the pass runs once, after the last kernel"""
    K, N, dtype = 640, 32, "f16"
    row, col, val, dense = ks_pattern(K)
    B = int_B_cpu(K, N, dtype, seed=1)
    prod = dense @ B.double().numpy()
    plan = gsa.Plan.from_coo(KS_M, K, row, col, val)
    with config(MFMA_TILES=0):
        for i, s in enumerate(plan.divide_rows(80)):
            plan.run_pipeline("merge_path" if i % 2 else "tblock_warp_total", N, 64 if i % 2 else 16, 1 if i % 2 else 2, sub=s)
        plan.compile().upload(dtype, 0)
    assert plan.info()["n_kernels"] == 2 and plan.epilogue_fused(N) == 0, plan.info()
    run_guarded_epilogue(plan, B, prod, dtype, dict(stage_sets(KS_M, N, dtype))["all"], "divided plan")
    plan.free()


# ------------------------------------------------------------------ 2: fused k_mfma_ks
# (KS_SPLIT, K, K ranges).  K = 33 is two k-steps: KS_SPLIT = 1 is the S == 1 store; KS_SPLIT = 0 (auto)
# splits these four row blocks as far as it can, one range per k-step, so it combines too.
# K = 1183 at KS_SPLIT = 3: the combine path over three ranges, the last row block of 11 rows
KS_CASES = [(1, 33, 1), (0, 33, 2), (3, 1183, 3)]


def ks_plan(K, N, dtype, split):
    row, col, val, _ = ks_pattern(K)
    plan = build(KS_M, K, row, col, val, "block_total", 40, 1, N, dtype, over={"KS_SPLIT": split})
    return plan


@functools.lru_cache(maxsize=None)
def ks_product(K, N, dtype):
    B = int_B_cpu(K, N, dtype, seed=1)
    prod = ks_pattern(K)[3] @ B.double().numpy()
    assert np.abs(prod).max() <= 1024
    return B, prod


@pytest.mark.parametrize("N", [32, 72])
@pytest.mark.parametrize("split,K,ranges", KS_CASES)
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_ks_fused(dtype, split, K, ranges, N, mfma_everywhere):
    """every stage alone and all together in k_mfma_ks's store: N = 72 is two column tiles, the last
    partial; K = 1183 at KS_SPLIT = 3 ends in the last-ticket combine"""
    B, prod = ks_product(K, N, dtype)
    plan = ks_plan(K, N, dtype, split)
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ranges and plan.epilogue_fused(N) == 1, info
    for name, epi in stage_sets(KS_M, N, dtype):
        run_guarded_epilogue(plan, B, prod, dtype, epi, f"k_mfma_ks {dtype} K={K} N={N} KS_SPLIT={split} {name}")
    plan.free()


# ------------------------------------------------------------------ 3: one rounding when fused
@pytest.mark.parametrize("split", [1, 2])
def test_fused_rounds_once(split, mfma_everywhere):
    """row 5 sums to 2049 exactly (512 x 2*2 + 1*1); with bias -2048 the fused store writes
    fp16(2049 - 2048) = 1, the post-pass fp16(fp16(2049) - 2048) = fp16(2048 - 2048) = 0"""
    M, K, N, R = 48, 544, 32, 5
    rng = np.random.default_rng(3)
    mask = rng.random((M, K)) < 0.05
    mask[R] = False
    mask[R, :513] = True
    r, c = np.nonzero(mask)
    row, col = r.astype(np.uint64), c.astype(np.uint64)
    val = int_values(len(row), 5)
    val[r == R] = 2.0
    val[(r == R) & (c == 512)] = 1.0
    B = int_B_cpu(K, N, "f16", seed=3).clone()
    B[:512] = 2
    B[512] = 1
    prod = dense_f64(M, K, row, col, val) @ B.double().numpy()
    assert (prod[R] == 2049).all() and np.abs(prod).max() == 2049
    bias = torch.zeros(M)
    bias[R] = -2048.0
    plan = build(M, K, row, col, val, "block_total", 48, 1, N, "f16", over={"KS_SPLIT": split})
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == split and plan.epilogue_fused(N) == 1, info
    fused = run_guarded_epilogue(plan, B, prod, "f16", {"bias": bias}, f"fused, {split} K ranges")
    assert (fused[R] == 1.0).all(), fused[R]
    with config(EPILOGUE_FUSE=0):
        assert plan.epilogue_fused(N) == 0
        twice = run_guarded_epilogue(plan, B, prod, "f16", {"bias": bias}, f"post-pass, {split} K ranges")
    assert (twice[R] == 0.0).all(), twice[R]
    assert plan.epilogue_fused(N) == 1
    plan.free()


# ------------------------------------------------------------------ 4: fused == post-pass when nothing rounds twice
@pytest.mark.parametrize("N", [32, 72])
@pytest.mark.parametrize("split,K,ranges", KS_CASES)
def test_fused_equals_post_pass_on_exact_products(split, K, ranges, N, mfma_everywhere):
    """fp16 with |A * B| <= 2048 (integers fp16 holds exactly): EPILOGUE_FUSE 1 and 0 give one C"""
    B, prod = ks_product(K, N, "f16")
    assert np.abs(prod).max() <= 2048
    plan = ks_plan(K, N, "f16", split)
    assert plan.info()["device_kernel"] == "k_mfma_ks" and plan.info()["ksplit"] == ranges, plan.info()
    for name, epi in stage_sets(KS_M, N, "f16"):
        what = f"K={K} N={N} KS_SPLIT={split} {name}"
        assert plan.epilogue_fused(N) == 1
        a = run_guarded_epilogue(plan, B, prod, "f16", epi, what + " fused")
        with config(EPILOGUE_FUSE=0):
            assert plan.epilogue_fused(N) == 0
            b = run_guarded_epilogue(plan, B, prod, "f16", epi, what + " post-pass")
        assert_bits(a, b, what + ": fused against post-pass")
    plan.free()


# ------------------------------------------------------------------ 5: the grouped launch
@pytest.mark.parametrize("fuse", [1, 0])
def test_grouped_launch_with_epilogues(fuse, mfma_everywhere):
    """three replicas of a KS_SPLIT = 3 plan as ONE k_mfma_ks_group launch, as without epilogues:
    entry 0 plain, entry 1 bias + relu, entry 2 alpha + residual; each C is its single spmm's bits
    (EPILOGUE_FUSE = 0: the same launch, then the pass over the entries that have an epilogue)"""
    K, N, dtype = 1183, 32, "f16"
    B_cpu, prod = ks_product(K, N, dtype)
    plan = ks_plan(K, N, dtype, 3)
    assert plan.info()["device_kernel"] == "k_mfma_ks" and plan.info()["ksplit"] == 3, plan.info()
    plan.add_replica()
    plan.add_replica()
    eps = [None, {"bias": int_bias(KS_M), "activation": "relu"}, {"alpha": 0.5, "residual": int_residual(KS_M, N, dtype)}]
    B, hb = guarded_B(B_cpu, DEV)
    outs = [guarded_C(KS_M, N, torch.float16, DEV) for _ in eps]
    entries = [(plan, i, B, C) for i, (C, _) in enumerate(outs)]
    assert gsa.Batch(entries, N).launches() == [3]
    with config(EPILOGUE_FUSE=fuse):
        assert plan.epilogue_fused(N) == fuse
        bat = gsa.Batch(entries, N, epilogues=[None if e is None else on_dev(e) for e in eps])
        assert bat.launches() == [3], bat.launches()
        singles = [run_guarded_epilogue(plan, B_cpu, prod, dtype, e or {}, f"single entry {i}", replica=i)
                   for i, e in enumerate(eps)]
        for again in ("", " relaunch"):
            bat.run(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            plan.device_status()
            for i, (C, hc) in enumerate(outs):
                assert_bits(C.cpu(), singles[i], f"grouped entry {i}{again}")
                assert_guards_intact(hc, f"grouped entry {i}{again} C")
                hc.refill()
            assert_guards_intact(hb, f"grouped{again} B")
    plan.free()


# ------------------------------------------------------------------ 6: the identity
def test_identity_epilogue_is_the_plain_spmm(mfma_everywhere):
    K, N = 1183, 32
    B_cpu, _ = ks_product(K, N, "f16")
    row, col, val, _ = ks_pattern(K)
    fused = ks_plan(K, N, "f16", 3)
    post = build(KS_M, K, row, col, val, "warp_total", 0, 1, N, "f16", over={"MFMA_TILES": 0})
    assert fused.epilogue_fused(N) == 1 and post.epilogue_fused(N) == 0
    B = B_cpu.to(DEV)
    for plan in (fused, post):
        a = plan.spmm(B)
        b = plan.spmm(B, alpha=1.0)
        # the C ABI's identity: gs_spmm_ex with alpha 1 and nothing else, and with a NULL epilogue
        c, d = torch.empty_like(a), torch.empty_like(a)
        one = _lib.GsEpilogue(1.0, 0, None, None)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        _lib.check(plan._L.gs_spmm_ex(plan._h, 0, ctypes.c_void_p(B.data_ptr()), ctypes.c_void_p(c.data_ptr()), N,
                                      ctypes.byref(one), s))
        _lib.check(plan._L.gs_spmm_ex(plan._h, 0, ctypes.c_void_p(B.data_ptr()), ctypes.c_void_p(d.data_ptr()), N, None, s))
        torch.cuda.synchronize()
        for other, what in ((b, "alpha=1.0"), (c, "gs_spmm_ex identity"), (d, "gs_spmm_ex NULL")):
            assert_bits(other, a, plan.info()["device_kernel"] + " " + what)
        plan.free()


# ------------------------------------------------------------------ 7: refusals
def test_refusals_leave_C_untouched(mfma_everywhere):
    K, N = 33, 32
    B_cpu, _ = ks_product(K, N, "f16")
    plan = ks_plan(K, N, "f16", 0)
    B = B_cpu.to(DEV)
    big = torch.full((KS_M + 1, N), 7.0, dtype=torch.float16, device=DEV)
    C = big[:KS_M]
    good_bias = int_bias(KS_M).to(DEV)
    good_res = int_residual(KS_M, N, "f16").to(DEV)
    bad = [
        ("bias length", ValueError, {"bias": torch.zeros(KS_M - 1, device=DEV)}),
        ("bias dtype", TypeError, {"bias": good_bias.half()}),
        ("bias device", ValueError, {"bias": good_bias.cpu()}),
        ("residual shape", ValueError, {"residual": torch.zeros((KS_M, N + 8), dtype=torch.float16, device=DEV)}),
        ("residual dtype", TypeError, {"residual": good_res.float()}),
        ("residual is C", ValueError, {"residual": C}),
        ("residual overlaps C", ValueError, {"residual": big[1:]}),
        ("activation", ValueError, {"activation": "gelu"}),
        ("alpha", ValueError, {"alpha": float("inf")}),
    ]
    for what, exc, kw in bad:
        with pytest.raises(exc):
            plan.spmm(B, C=C, **kw)
        torch.cuda.synchronize()
        assert bool((big == 7.0).all()), what
    # the C ABI refuses with code -1 before any launch: unknown activation, non-finite alpha, residual == C
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for what, epi in (("activation", _lib.GsEpilogue(1.0, 2, None, None)),
                      ("alpha", _lib.GsEpilogue(float("nan"), 0, None, None)),
                      ("residual", _lib.GsEpilogue(1.0, 0, None, C.data_ptr()))):
        rc = plan._L.gs_spmm_ex(plan._h, 0, ctypes.c_void_p(B.data_ptr()), ctypes.c_void_p(C.data_ptr()), N, ctypes.byref(epi), s)
        assert rc == -1, (what, rc)
        ptr = (ctypes.POINTER(_lib.GsEpilogue) * 1)(ctypes.pointer(epi))
        args = ((ctypes.c_void_p * 1)(plan._h), (ctypes.c_int * 1)(0), (ctypes.c_void_p * 1)(B.data_ptr()),
                (ctypes.c_void_p * 1)(C.data_ptr()))
        rc = plan._L.gs_spmm_batch_ex(*args, ptr, 1, N, s)
        assert rc == -1, (what, rc)
        torch.cuda.synchronize()
        assert bool((big == 7.0).all()), what
    # a Batch checks its epilogues when it is built
    with pytest.raises(ValueError):
        gsa.Batch([(plan, 0, B, C)], N, epilogues=[{"activation": "gelu"}])
    with pytest.raises(ValueError):
        gsa.Batch([(plan, 0, B, C)], N, epilogues=[{"residual": C}])
    # and the accepted call still works on the same operands
    plan.spmm(B, C=C, bias=good_bias, residual=good_res)
    torch.cuda.synchronize()
    assert not bool((C == 7.0).all())
    plan.free()


# ------------------------------------------------------------------ 8: one non-integer case per path
@pytest.mark.parametrize("path", ["fused", "post-pass"])
def test_uniform_operands_within_tolerance(path, mfma_everywhere):
    """uniform operands, an fp64 reference from the dtype-rounded operands, held to
    tolerance.bound(dtype, kernel) relative to max(1, |ref|).
    The 16-bit post-pass rounds the product to fp16 before the stages: c = fp16(acc) differs from
    acc by at most half an ulp, |c - acc| <= 2^-11 |acc| (fp16 holds 11 significant bits), and the
    stages carry that to the result times |alpha| (the bias and residual adds and relu have
    Lipschitz constant 1).  So the post-pass is allowed |alpha| * 2^-11 * |acc| more, an absolute
    term from the reference's own acc -- not a wider relative bound."""
    M, K, N, dtype, alpha = KS_M, 640, 32, "f16", -0.75
    rng = np.random.default_rng(11)
    row, col, _, _ = ks_pattern(K)
    val = rng.uniform(-1, 1, len(row)).astype(np.float32)
    B16 = rng.uniform(-1, 1, (K, N)).astype(np.float16)
    bias = rng.uniform(-2, 2, M).astype(np.float32)
    res16 = rng.uniform(-1, 1, (M, N)).astype(np.float16)
    if path == "fused":
        plan = build(M, K, row, col, val, "block_total", 40, 1, N, dtype, over={"KS_SPLIT": 2})
    else:
        plan = build(M, K, row, col, val, "warp_total", 0, 1, N, dtype, over={"MFMA_TILES": 0})
    kernel = plan.info()["device_kernel"]
    assert plan.epilogue_fused(N) == (1 if path == "fused" else 0) and (kernel == "k_mfma_ks") == (path == "fused"), kernel
    acc = dense_f64(M, K, row, col, val.astype(np.float16).astype(np.float64)) @ B16.astype(np.float64)
    ref = alpha * acc + bias[:, None].astype(np.float64)
    ref = np.where(ref < 0, 0.0, ref) + res16.astype(np.float64)
    C = plan.spmm(torch.from_numpy(B16).to(DEV), alpha=alpha, bias=torch.from_numpy(bias).to(DEV), activation="relu",
                  residual=torch.from_numpy(res16).to(DEV))
    torch.cuda.synchronize()
    err = np.abs(C.float().cpu().numpy().astype(np.float64) - ref)
    allowed = tolerance.bound(dtype, kernel) * np.maximum(1.0, np.abs(ref))
    if path == "post-pass":
        allowed = allowed + abs(alpha) * 2.0 ** -11 * np.abs(acc)
    worst = float((err / allowed).max())
    print(f"{path} {kernel}: max err / allowed = {worst:.3f}, max rel err {tolerance.rel_err(C.float().cpu().numpy(), ref):.3e}")
    assert worst <= 1.0, (path, kernel, worst)
    plan.free()
