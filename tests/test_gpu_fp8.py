"""GPU checks of FP8 (OCP e4m3fn) weight values on k_mfma_ks plans: Plan.upload(weights="fp8") stores one
code per value and one float32 scale per row; k_mfma_ks_w8 (spmm at the plan's width) and k_mfma_ks_tm's
8-bit form (linear at any token count) decode the codes to fp16, run the f16 kernels' MFMAs and scale the
fp32 sum of a row before the epilogue and the one rounding.

Every finite e4m3 value is an fp16 value and a power-of-two scale multiplies exactly, so all but one of
the comparisons here are bit for bit: against the CPU decode table, against epilogue_ref on integer
operands, and against the f16 plan of the dequantised weights.  Shapes and operands are those of
tests/test_gpu_linear.py (M = 131: 40-row blocks, the last with 11 rows, odd tokens' rows unaligned);
X / B, Y / C and the residual are guarded (tests/guarded.py), every launch is repeated into the
NaN-refilled output and plan.device_status() must be clean."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C  # noqa: E402
from test_gpu_edges import DEV, TORCH_DT, build  # noqa: E402
from test_gpu_edges_mfma import KS_M, ks_pattern, ks_ranges, mfma_everywhere  # noqa: E402,F401  (fixture)
from test_gpu_epilogue import config, epilogue_ref, run_guarded_epilogue, stage_sets  # noqa: E402
from test_gpu_linear import FUSED_CASES, full_epilogue, ks_operands, run_linear  # noqa: E402
from test_gpu_linear_tokens import misaligned_B  # noqa: E402
from tolerance import TIGHT_F16, bound, rel_err  # noqa: E402

pytestmark = pytest.mark.gpu

FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)


def fp8_plan(M, K, row, col, val, n, split, row_scale=None, dtype="f16", pipeline=("block_total", 40, 1), **over):
    """compile at N = n with KS_SPLIT = split and upload with FP8 weights"""
    with config(**dict(over, KS_SPLIT=split)):
        plan = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline(pipeline[0], n, pipeline[1], pipeline[2]).compile()
        return plan.upload(dtype, 0, weights="fp8", row_scale=row_scale)


def check_fp8(plan, K, split, n=None):
    info = plan.info()
    assert info["weights"] == 1 and info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split), info
    assert plan.epilogue_fused(info["lds_n"]) == 1
    if n is not None:
        assert plan.linear_fused(n) == 1, (n, info)
    return info


def run_pair(fn, Y, hy, holders, ref, what):
    """a launch and a relaunch into the refilled output: bits and guard bands both times"""
    for again in ("", " relaunch"):
        fn()
        torch.cuda.synchronize()
        assert_bits(Y, ref, what + again)
        assert_guards_intact(hy, what + again + " out")
        for h in holders:
            assert_guards_intact(h, what + again + " in")
        out = Y.cpu().clone()
        hy.refill()
    return out


# ------------------------------------------------------------------ 1: the decode on the device
@pytest.mark.parametrize("split", [1, 2])
def test_every_code_decodes_on_the_device(split, mfma_everywhere):
    """K = 40, M = 131, values cycling through the 254 finite codes at row_scale = 1, X one-hot (token t
    selects column t; n = 40: a full tile and a partial one): Y[t, r] is the decoded A[r, t] -- the CPU
    decode table at every stored position (subnormal codes, both zeros, +-448), 0 elsewhere"""
    K, n = 40, 40
    row, col, _, _ = ks_pattern(K)
    assert len(row) >= 4 * 254
    code = FINITE[np.arange(len(row)) % 254]
    val = gsa.fp8_decode(code)
    ones = np.ones(KS_M, np.float32)
    got_codes, _ = gsa.fp8_quantize(val, row, KS_M, row_scale=ones)
    np.testing.assert_array_equal(got_codes & 0x7F, code & 0x7F)  # (the quantiser is the identity on code values)
    plan = fp8_plan(KS_M, K, row, col, val, 32, split, row_scale=ones)
    check_fp8(plan, K, split, n)
    dense = np.zeros((KS_M, K), np.float32)
    dense[row.astype(np.int64), col.astype(np.int64)] = val
    want = torch.from_numpy(dense.T.copy()).to(torch.float16)
    assert bool((want.float() == torch.from_numpy(dense.T.copy())).all())  # fp16 holds every code's value
    X, hx = guarded_B(torch.eye(n, K, dtype=torch.float16), DEV)
    Y, hy = guarded_C(n, KS_M, torch.float16, DEV)
    for again in ("", " relaunch"):
        plan.linear(X, out=Y)
        torch.cuda.synchronize()
        plan.device_status()
        got = Y.cpu()
        bad = (got.float() != want.float()).nonzero()
        assert len(bad) == 0, f"{len(bad)} values differ{again}, first at token {bad[0].tolist()}: " \
                              f"{got[tuple(bad[0])].item()} vs {want[tuple(bad[0])].item()}"
        assert_guards_intact(hy, "decode Y" + again)
        assert_guards_intact(hx, "decode X" + again)
        hy.refill()
    plan.free()


# ------------------------------------------------------------------ 2: exact, integer operands
@pytest.mark.parametrize("split,K", FUSED_CASES)
def test_exact_on_integer_operands(split, K, mfma_everywhere):
    """A in {+-1, +-2} (default scales 2^-7 / 2^-8: the codes are exact), X in {-2 .. 2}: linear at
    n = 32 with KS_NT 0 and 1 and at n = 24, spmm at N = 32 and 24, every stage set, against
    epilogue_ref from the exact product with one rounding"""
    dtype = "f16"
    row, col, val, _ = ks_pattern(K)
    for n, nt in ((32, 0), (32, 1), (24, 0)):
        X, prod = ks_operands(K, n, dtype)
        plan = fp8_plan(KS_M, K, row, col, val, n, split, KS_NT=nt)
        info = check_fp8(plan, K, split, n)
        assert info["ks_nt"] == nt and info["lds_n"] == n, info
        for name, epi in stage_sets(KS_M, n, dtype):
            what = f"FP8 K={K} n={n} KS_SPLIT={split} KS_NT={nt} {name}"
            run_linear(plan, X, prod, dtype, epi, "k_mfma_ks_tm VB=8 " + what, True)
            if nt == 0 or name == "all":
                run_guarded_epilogue(plan, X.t().contiguous(), prod, dtype, epi, "k_mfma_ks_w8 " + what, True)
        plan.free()


# ------------------------------------------------------------------ 3: the same bits as the f16 twin
def normal_weights(K, seed):
    """random normal values (magnitudes floored at 2^-6) times a per-row power of two in 2^-3 .. 2^3"""
    row, col, _, _ = ks_pattern(K)
    rng = np.random.default_rng(seed)
    z = rng.standard_normal(len(row))
    z = np.copysign(np.maximum(np.abs(z), 2.0 ** -6), z)
    pw = np.exp2(rng.integers(-3, 4, KS_M))
    return row, col, (z * pw[row.astype(np.int64)]).astype(np.float32), rng


@pytest.mark.parametrize("split,K", [(3, 1176), (1, 1184)])
def test_same_bits_as_the_f16_plan_of_the_dequantised_weights(split, K, mfma_everywhere):
    """the FP8 plan of the raw values against the f16 plan of fp8_decode(codes) * scale[row]: the same
    MFMAs on the same numbers up to the rows' powers of two, so identical bits -- linear at n = 32, 8
    and 100 (four tiles: the T > 1 K-split state), spmm at N = 32; and linear(x) == spmm(x.T).T"""
    row, col, val, rng = normal_weights(K, 21 + K)
    r = row.astype(np.int64)
    codes, scale = gsa.fp8_quantize(val, row, KS_M)
    deq = gsa.fp8_decode(codes) * scale[r]
    assert (codes & 0x7F != 0).all(), "no entry quantises to zero"
    assert (np.abs(deq) >= 2.0 ** -14).all() and (deq.astype(np.float16).astype(np.float32) == deq).all()  # normal fp16, exact
    assert (np.frexp(scale)[0] == 0.5).all()
    p8 = fp8_plan(KS_M, K, row, col, val, 32, split)
    p16 = build(KS_M, K, row, col, deq, "block_total", 40, 1, 32, "f16", over={"KS_SPLIT": split})
    check_fp8(p8, K, split, 100)
    i16 = p16.info()
    assert i16["weights"] == 0 and i16["device_kernel"] == "k_mfma_ks" and i16["ksplit"] == ks_ranges(K, split), i16
    x_cpu = torch.from_numpy(rng.standard_normal((100, K)).astype(np.float32)).to(torch.float16)
    for n in (32, 8, 100):
        X, hx = guarded_B(x_cpu[:n].contiguous(), DEV)
        want = p16.linear(X)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(want).any())
        Y, hy = guarded_C(n, KS_M, torch.float16, DEV)
        y = run_pair(lambda: p8.linear(X, out=Y), Y, hy, [hx], want, f"linear n={n} K={K} KS_SPLIT={split}: FP8 against f16 plan")
        p8.device_status()
        if n == 32:
            B, hb = guarded_B(x_cpu[:32].t().contiguous(), DEV)
            want_c = p16.spmm(B)
            C, hc = guarded_C(KS_M, 32, torch.float16, DEV)
            c = run_pair(lambda: p8.spmm(B, C=C), C, hc, [hb], want_c, f"spmm N=32 K={K} KS_SPLIT={split}: FP8 against f16 plan")
            assert_bits(y, c.t().contiguous(), "FP8 plan: linear(x) against spmm(x.T).T")
    p8.device_status()
    p16.device_status()
    p8.free()
    p16.free()


# ------------------------------------------------------------------ 4: token invariance
def test_a_tokens_row_does_not_depend_on_the_token_count(mfma_everywhere):
    split, K = 3, 1176
    row, col, val, rng = normal_weights(K, 5)
    plan = fp8_plan(KS_M, K, row, col, val, 32, split)
    check_fp8(plan, K, split, 100)
    X, hx = guarded_B(torch.from_numpy(rng.standard_normal((100, K)).astype(np.float32)).to(torch.float16), DEV)
    y100 = plan.linear(X)
    y40 = plan.linear(X[:40])
    y8 = plan.linear(X[:8])
    torch.cuda.synchronize()
    plan.device_status()
    assert not bool(torch.isnan(y100).any())
    assert_bits(y40, y100[:40].contiguous(), "rows 0..39: n = 40 against n = 100")
    assert_bits(y8, y100[:8].contiguous(), "rows 0..7: n = 8 against n = 100")
    assert_guards_intact(hx, "token invariance X")
    plan.free()


# ------------------------------------------------------------------ 5: scales that are no powers of two
@pytest.mark.parametrize("split,K", [(3, 1176), (1, 1184)])
def test_caller_scales_within_the_tight_f16_bound(split, K, mfma_everywhere):
    """row_scale = amax / 448: the scale multiply rounds (once, in fp32), so this one is held to
    tests/tolerance.py's tight f16 bound against the float64 product of the dequantised weights"""
    row, col, val, rng = normal_weights(K, 9 + K)
    r = row.astype(np.int64)
    amax = np.zeros(KS_M, np.float32)
    np.maximum.at(amax, r, np.abs(val))
    scale_in = (amax / np.float32(448.0)).astype(np.float32)
    assert (np.frexp(scale_in)[0] != 0.5).any()
    codes, scale = gsa.fp8_quantize(val, row, KS_M, row_scale=scale_in)
    np.testing.assert_array_equal(scale, scale_in)
    deq = np.zeros((KS_M, K), np.float64)
    deq[r, col.astype(np.int64)] = gsa.fp8_decode(codes).astype(np.float64) * scale.astype(np.float64)[r]
    plan = fp8_plan(KS_M, K, row, col, val, 32, split, row_scale=scale_in)
    check_fp8(plan, K, split, 100)
    x_cpu = torch.from_numpy(rng.standard_normal((100, K)).astype(np.float32)).to(torch.float16)
    ref = x_cpu.double().numpy() @ deq.T
    assert bound("f16", "k_mfma_ks") == TIGHT_F16
    for n in (32, 100):
        X, hx = guarded_B(x_cpu[:n].contiguous(), DEV)
        Y, hy = guarded_C(n, KS_M, torch.float16, DEV)
        plan.linear(X, out=Y)
        torch.cuda.synchronize()
        plan.device_status()
        err = rel_err(Y.float().cpu().numpy(), ref[:n])
        print(f"caller scales K={K} KS_SPLIT={split} linear n={n}: max rel err {err:.3g} (bound {TIGHT_F16:.3g})")
        assert err <= TIGHT_F16, (n, err)
        assert_guards_intact(hy, "caller scales Y")
        assert_guards_intact(hx, "caller scales X")
    B, hb = guarded_B(x_cpu[:32].t().contiguous(), DEV)
    C, hc = guarded_C(KS_M, 32, torch.float16, DEV)
    plan.spmm(B, C=C)
    torch.cuda.synchronize()
    plan.device_status()
    err = rel_err(C.float().cpu().numpy(), ref[:32].T)
    print(f"caller scales K={K} KS_SPLIT={split} spmm N=32: max rel err {err:.3g} (bound {TIGHT_F16:.3g})")
    assert err <= TIGHT_F16, err
    assert_guards_intact(hc, "caller scales C")
    assert_guards_intact(hb, "caller scales B")
    plan.free()


# ------------------------------------------------------------------ 6: replicas and batches
def test_replica_and_batch(mfma_everywhere):
    """replica 1 (add_replica copies the codes and the scales) gives replica 0's bits; a Batch of two
    FP8 plans runs as single launches (no grouped FP8 kernel) with the single calls' bits"""
    split, K, N = 3, 1176, 32
    rowa, cola, vala, rng = normal_weights(K, 31)
    rowb, colb, valb, _ = normal_weights(K, 32)
    pa = fp8_plan(KS_M, K, rowa, cola, vala, N, split)
    pb = fp8_plan(KS_M, K, rowb, colb, valb, N, split)
    check_fp8(pa, K, split, N)
    check_fp8(pb, K, split, N)
    pa.add_replica()
    assert pa.info()["replicas"] == 2
    x_cpu = torch.from_numpy(rng.standard_normal((N, K)).astype(np.float32)).to(torch.float16)
    X, hx = guarded_B(x_cpu, DEV)
    B, hb = guarded_B(x_cpu.t().contiguous(), DEV)
    y0, c0, cb = pa.linear(X, replica=0), pa.spmm(B, replica=0), pb.spmm(B)
    torch.cuda.synchronize()
    Y, hy = guarded_C(N, KS_M, torch.float16, DEV)
    run_pair(lambda: pa.linear(X, out=Y, replica=1), Y, hy, [hx], y0, "replica 1 against replica 0: linear")
    C, hc = guarded_C(KS_M, N, torch.float16, DEV)
    run_pair(lambda: pa.spmm(B, C=C, replica=1), C, hc, [hb], c0, "replica 1 against replica 0: spmm")
    outs = [guarded_C(KS_M, N, torch.float16, DEV) for _ in range(2)]
    bat = gsa.Batch([(pa, 1, B, outs[0][0]), (pb, 0, B, outs[1][0])], N)
    assert bat.launches() == [1, 1], bat.launches()
    for again in ("", " relaunch"):
        bat.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for (Cx, hcx), want, name in zip(outs, (c0, cb), "ab"):
            assert_bits(Cx, want, f"batch entry {name}{again}")
            assert_guards_intact(hcx, f"batch entry {name}{again} C")
            hcx.refill()
        assert_guards_intact(hb, "batch B" + again)
    pa.device_status()
    pb.device_status()
    pa.free()
    pb.free()


# ------------------------------------------------------------------ 7: refusals
def compiled(M, K, row, col, val, pipeline, N, p0, p1, **over):
    with config(**over):
        return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline(pipeline, N, p0, p1).compile()


def test_refused_uploads_leave_no_plan_on_the_device(mfma_everywhere):
    K = 1184
    row, col, val, _ = ks_pattern(K)
    B = torch.zeros((K, 32), dtype=torch.float16, device=DEV)
    C = torch.full((KS_M, 32), 7.0, dtype=torch.float16, device=DEV)

    def refused(plan, match, dtype="f16", over=None, **kw):
        with config(**(over or {})):  # (the upload chooses the layout under the config of the moment)
            with pytest.raises(gsa.GsError, match=match):
                plan.upload(dtype, 0, weights="fp8", **kw)
        with pytest.raises(gsa.GsError, match="not on the device"):  # nothing half-uploaded
            plan.spmm_raw(B.data_ptr(), C.data_ptr(), 32)
        torch.cuda.synchronize()
        assert bool((C == 7.0).all())

    refused(compiled(KS_M, K, row, col, val, "thread_total", 32, 4, 1), "k_mfma_ks plans only")  # a gather family
    refused(compiled(KS_M, K, row, col, val, "block_total", 64, 40, 1), "17 .. 32")  # built for N = 64
    refused(compiled(KS_M, K, row, col, val, "block_total", 16, 40, 1), "17 .. 32")  # ... for N = 16
    ok = compiled(KS_M, K, row, col, val, "block_total", 32, 40, 1)
    refused(ok, "fp16 activations", dtype="bf16")
    refused(ok, "fp16 activations", dtype="f32")
    refused(ok, "row_scale", row_scale=np.zeros(KS_M, np.float32))
    refused(ok, "row_scale", row_scale=np.ones(KS_M + 1, np.float32))
    refused(ok, "16-bit entry positions", over={"KS_WPOS": 1})
    r1180, c1180, v1180, _ = ks_pattern(1180)
    refused(compiled(KS_M, 1180, r1180, c1180, v1180, "block_total", 32, 40, 1), "multiple of 8")
    bad = val.copy()
    bad[11] = np.nan
    refused(compiled(KS_M, K, row, col, bad, "block_total", 32, 40, 1), "non-finite")
    # a divided plan
    plan = gsa.Plan.from_coo(KS_M, K, row, col, val)
    for s in plan.divide_rows(80):
        plan.run_pipeline("block_total", 32, 40, 1, sub=s)
    plan.compile()
    with pytest.raises(gsa.GsError, match="undivided"):
        plan.upload("f16", 0, weights="fp8")
    # and the plan every refusal above was measured against uploads
    ok.upload("f16", 0, weights="fp8")
    assert ok.info()["weights"] == 1
    ok.upload("f16", 0)  # ... and goes back to native values
    assert ok.info()["weights"] == 0
    ok.free()


def test_refused_launches_leave_the_output_untouched(mfma_everywhere):
    split, K, W = 2, 1184, 32
    row, col, val, _ = ks_pattern(K)
    plan = fp8_plan(KS_M, K, row, col, val, W, split)
    check_fp8(plan, K, split, W)
    # spmm at a width other than the plan's (no CSR copy of A behind an FP8 plan)
    for N in (24, 64):
        B, hb = guarded_B(torch.ones((K, N), dtype=torch.float16), DEV)
        C, hc = guarded_C(KS_M, N, torch.float16, DEV)
        C.fill_(7.0)
        with pytest.raises(gsa.GsError, match="width it was built for"):
            plan.spmm(B, C=C)
        with pytest.raises(gsa.GsError, match="width it was built for"):
            plan.spmm(B, C=C, alpha=2.0)
        torch.cuda.synchronize()
        assert bool((C == 7.0).all()), N
        assert_guards_intact(hc, f"refused spmm N={N}")
    # linear with a misaligned x: three launches, so only at the plan's width
    for n in (8, 72):
        X_cpu, _ = ks_operands(K, n, "f16")
        x, _ = misaligned_B(X_cpu, DEV)
        Y, hy = guarded_C(n, KS_M, torch.float16, DEV)
        Y.fill_(7.0)
        assert plan.linear_launches(n, x) == []
        with pytest.raises(gsa.GsError, match="three-launch"):
            plan.linear(x, out=Y)
        torch.cuda.synchronize()
        assert bool((Y == 7.0).all()), n
        assert_guards_intact(hy, f"refused linear n={n}")
    with config(LINEAR_FUSE=0):
        X = ks_operands(K, 8, "f16")[0].to(DEV)
        Y = torch.full((8, KS_M), 7.0, dtype=torch.float16, device=DEV)
        with pytest.raises(gsa.GsError, match="three-launch"):
            plan.linear(X, out=Y)
        torch.cuda.synchronize()
        assert bool((Y == 7.0).all())
    # the positive case: a misaligned x at n = lds_n runs the three launches (two roundings)
    X_cpu, prod = ks_operands(K, W, "f16")
    epi = full_epilogue(KS_M, W, "f16")
    x, flat = misaligned_B(X_cpu, DEV)
    ref = epilogue_ref(prod, "f16", False, **epi).t().contiguous().to(DEV)
    Y, hy = guarded_C(W, KS_M, torch.float16, DEV)
    res = epi["residual"].t().contiguous().to(DEV)
    run_pair(lambda: plan.linear(x, out=Y, alpha=epi["alpha"], bias=epi["bias"].to(DEV), activation=epi["activation"], residual=res),
             Y, hy, [], ref, "misaligned x at the plan's width: three launches")
    with config(LINEAR_FUSE=0):
        run_linear(plan, X_cpu, prod, "f16", epi, "LINEAR_FUSE=0 at the plan's width", False)
    plan.device_status()
    plan.free()


# ------------------------------------------------------------------ 8: the module
def test_sparse_linear_with_fp8_weights(mfma_everywhere):
    K = 1184
    row, col, val, rng = normal_weights(K, 41)
    dense = np.zeros((KS_M, K), np.float32)
    dense[row.astype(np.int64), col.astype(np.int64)] = val
    bias = torch.arange(KS_M, dtype=torch.float32) / 8 - 8.0
    layer = gsa.SparseLinear.from_dense(torch.from_numpy(dense), bias, tokens=32, activation="relu", weights="fp8")
    info = layer.plan.info()
    assert info["weights"] == 1 and info["device_kernel"] == "k_mfma_ks" and info["nnz"] == len(row), info
    assert "weights=fp8_e4m3" in repr(layer) and "linear_fused(32)=1" in repr(layer), repr(layer)
    plain = gsa.SparseLinear.from_dense(torch.from_numpy(dense), bias, tokens=32, activation="relu")
    assert "fp8" not in repr(plain), repr(plain)
    x = torch.from_numpy(rng.standard_normal((3, 15, K)).astype(np.float32)).to(torch.float16).to(DEV)
    y = layer(x)
    flat = layer.plan.linear(x.reshape(45, K), bias=bias.to(DEV), activation="relu")
    torch.cuda.synchronize()
    layer.plan.device_status()
    assert tuple(y.shape) == (3, 15, KS_M) and y.dtype == torch.float16 and not bool(torch.isnan(y).any())
    assert_bits(y.reshape(45, KS_M), flat, "SparseLinear.forward against Plan.linear")
    with pytest.raises(gsa.GsError, match="fp16 activations"):
        gsa.SparseLinear.from_dense(torch.from_numpy(dense), bias, tokens=32, dtype="bf16", weights="fp8")
    layer.plan.free()
    plain.plan.free()


# ------------------------------------------------------------------ 9: bytes
@pytest.mark.parametrize("head", [0, 1])
def test_tile_bytes_drop_by_eight_per_entry_group(head, mfma_everywhere):
    """tile_bytes = BMTB rows + positions (16 B per group) + values + step records: the f16 plan holds
    16 B of values per entry group, the FP8 plan 8, everything else is the same -- so the difference is
    exactly 8 x groups, the group count being the layout's (len(codes) / 8, the spare group included);
    device_bytes_A drops by that less the 4 x M bytes of scales"""
    split, K = 3, 1176
    row, col, val, _ = ks_pattern(K)
    p8 = fp8_plan(KS_M, K, row, col, val, 32, split, KS_HEAD=head)
    p16 = build(KS_M, K, row, col, val, "block_total", 40, 1, 32, "f16", over={"KS_SPLIT": split, "KS_HEAD": head})
    with config(KS_SPLIT=split, KS_HEAD=head):
        codes, scale = p8.fp8_layout()
    groups = len(codes) // 8
    i8, i16 = p8.info(), p16.info()
    assert (i8["ks_head_groups"] > 0) == (i16["ks_head_groups"] > 0)
    assert groups * 8 == len(codes) and groups > len(row) // 8
    assert i16["tile_bytes"] - i8["tile_bytes"] == 8 * groups, (i16["tile_bytes"], i8["tile_bytes"], groups)
    assert i16["device_bytes_A"] - i8["device_bytes_A"] == 8 * groups - 4 * KS_M
    p8.free()
    p16.free()
