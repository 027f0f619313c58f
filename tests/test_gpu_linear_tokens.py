"""GPU checks of the token-major linear at token counts other than the plan's own width: a k_mfma_ks
plan built for 32 tokens runs k_mfma_ks_tm on ceil(n / 32) token tiles at any n >= 1 (one launch, or
several where the tiles' K-split state would pass LINEAR_WS_KB).

Plans are ks_plan(K, 32, dtype, split) of tests/test_gpu_linear.py on the 131-row pattern (40-row
blocks: 4 row blocks of 3 row tiles).  The operands are its integer ones, so every comparison is bit
for bit and needs no tolerance; X, Y and the residual are guarded (tests/guarded.py), every launch is
repeated into the NaN-refilled Y, and plan.device_status() must be clean (run_linear)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guard_elems, guarded_B, guarded_C  # noqa: E402
from test_gpu_edges import DEV, TORCH_DT, build, int_B_cpu  # noqa: E402
from test_gpu_edges_mfma import KS_M, ks_case, ks_pattern, ks_ranges, mfma_everywhere  # noqa: E402,F401  (fixture)
from test_gpu_epilogue import config, epilogue_ref, stage_sets  # noqa: E402
from test_gpu_linear import full_epilogue, ks_operands, ks_plan, run_linear  # noqa: E402

pytestmark = pytest.mark.gpu

W = 32  # the width every plan here is built for
NB, RT = 4, 3  # the pattern's 40-row blocks: 40, 40, 40, 11 rows; 3 row tiles of 16


def tiles(n):
    return (n + 31) // 32


def check_plan(plan, K, split):
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split), info


# ------------------------------------------------------------------ 1: exact at every tile shape
# n = 1, 7, 16: one partial tile, the second 16-token MFMA tile all clamped at 1 .. 16; 17, 31: partial
# in the second one; 33: a full tile and one token; 64: two full tiles; 72, 100: a partial last tile
TOKENS = [1, 7, 16, 17, 31, 33, 64, 72, 100]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("split,K", [(1, 40), (2, 40), (3, 1176), (2, 1184)])
def test_exact_at_every_tile_shape(split, K, dtype, mfma_everywhere):
    plan = ks_plan(K, W, dtype, split)
    check_plan(plan, K, split)
    for n in TOKENS:
        X, prod = ks_operands(K, n, dtype)
        assert plan.linear_fused(n) == 1, n
        assert plan.linear_launches(n) == [tiles(n)], n
        sets = stage_sets(KS_M, n, dtype)
        for name, epi in sets if n in (7, 72) else [s for s in sets if s[0] == "all"]:
            run_linear(plan, X, prod, dtype, epi, f"k_mfma_ks_tm {dtype} K={K} KS_SPLIT={split} n={n} {name}", True)
    plan.free()


# ------------------------------------------------------------------ 2: token invariance
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("split,K", [(3, 1176), (1, 1184)])
def test_a_tokens_row_does_not_depend_on_the_call(split, K, dtype, mfma_everywhere):
    """random normal A and X (test_same_bits_as_spmm's): the MFMAs and every sum keep their order at
    any n, so linear(x[:100]) is the four 32-token calls -- the path of before, the last slice
    zero-padded and cut -- one after another, and linear(x[:7]) rows 0 .. 6 of linear(x[:32])"""
    row, col, _, _ = ks_pattern(K)
    rng = np.random.default_rng(7 + K)
    val = rng.standard_normal(len(row)).astype(np.float32)
    plan = build(KS_M, K, row, col, val, "block_total", 40, 1, W, dtype, over={"KS_SPLIT": split})
    check_plan(plan, K, split)
    x = torch.from_numpy(rng.standard_normal((100, K)).astype(np.float32)).to(TORCH_DT[dtype]).to(DEV)
    pad = torch.zeros((128, K), dtype=x.dtype, device=DEV)
    pad[:100] = x
    parts = [plan.linear(pad[i:i + 32]).clone() for i in range(0, 128, 32)]  # 32 tokens: one tile, the plan's width
    want = torch.cat(parts)[:100].contiguous()
    assert plan.linear_launches(100) == [4]
    y = plan.linear(x)
    y7 = plan.linear(x[:7])
    torch.cuda.synchronize()
    plan.device_status()
    assert tuple(y.shape) == (100, KS_M) and not bool(torch.isnan(y).any())
    assert_bits(y, want, f"100 tokens against four 32-token calls {dtype} K={K} KS_SPLIT={split}")
    assert_bits(y7, parts[0][:7].contiguous(), f"7 tokens against rows 0..6 of 32 {dtype} K={K} KS_SPLIT={split}")
    plan.free()


# ------------------------------------------------------------------ 3: geometry changes on one replica
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_tile_counts_in_turn_on_one_replica(dtype, mfma_everywhere):
    """three K ranges: the arrival counters' epochs and the slabs' tags are laid out by the tile count,
    so each change of it must start from cleared state; one tile (33 -> 32, 72 -> 32) runs on the
    upload's state, which the plan's SpMM at N = 32 shares"""
    split, K = 3, 1176
    plan = ks_plan(K, W, dtype, split)
    check_plan(plan, K, split)
    B32, ref32 = ks_case(K, 32, dtype)
    for step, n in enumerate((100, 40, 100, 33, 32, 72, 32)):
        X, prod = ks_operands(K, n, dtype)
        assert plan.linear_launches(n) == [tiles(n)]
        run_linear(plan, X, prod, dtype, full_epilogue(KS_M, n, dtype), f"step {step}: n={n} {dtype}", True, replica=0)
        if step in (0, 3, 5):
            c = plan.spmm(B32.to(DEV))
            torch.cuda.synchronize()
            plan.device_status()
            assert_bits(c, ref32.to(DEV), f"spmm at N=32 after step {step}")
    plan.free()


# ------------------------------------------------------------------ 4: the budget splits a call
def ws_kb_for(tile_bytes, cap):
    """a LINEAR_WS_KB that holds `cap` tiles' state and not cap + 1"""
    kb = (cap * tile_bytes + 1023) // 1024
    assert kb * 1024 // tile_bytes == cap
    return kb


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_the_budget_splits_a_call(dtype, mfma_everywhere):
    split, K, n = 3, 1176, 100
    X, prod = ks_operands(K, n, dtype)
    epi = full_epilogue(KS_M, n, dtype)  # alpha, bias, relu and the residual: each launch offsets Y and the residual
    plan = ks_plan(K, W, dtype, split)
    check_plan(plan, K, split)
    tile_bytes = NB * 3 * RT * 2048 + NB * 4
    old = gsa.get_config("LINEAR_WS_KB")
    for cap, want in ((1, [1, 1, 1, 1]), (2, [2, 2])):
        with config(LINEAR_WS_KB=ws_kb_for(tile_bytes, cap)):
            assert plan.linear_launches(n) == want
            run_linear(plan, X, prod, dtype, epi, f"{dtype} n={n} launches {want}", True)
    assert gsa.get_config("LINEAR_WS_KB") == old
    assert plan.linear_launches(n) == [4]
    run_linear(plan, X, prod, dtype, epi, f"{dtype} n={n} one launch again", True)
    plan.free()
    # one K range keeps no state: nothing to bound
    K = 1184
    X, prod = ks_operands(K, n, dtype)
    plan = ks_plan(K, W, dtype, 1)
    check_plan(plan, K, 1)
    for kb in (0, 1, 100):
        with config(LINEAR_WS_KB=kb):
            assert plan.linear_launches(n) == [4]
            run_linear(plan, X, prod, dtype, epi, f"{dtype} one K range, LINEAR_WS_KB={kb}", True)
    plan.free()


# ------------------------------------------------------------------ 5: containment
def test_a_nan_token_stays_in_its_row_of_a_partial_tile(mfma_everywhere):
    """n = 72 (the last tile holds 8 tokens), token 40 all NaN: row 40 of Y is NaN, every other row the
    reference's bits; the NaN bands around X and the residual catch a read past token n - 1 that
    reaches a stored row"""
    split, K, n, dtype = 3, 1176, 72, "f16"
    X_cpu, prod = ks_operands(K, n, dtype)
    plan = ks_plan(K, W, dtype, split)
    check_plan(plan, K, split)
    epi = full_epilogue(KS_M, n, dtype)
    ref = epilogue_ref(prod, dtype, True, **epi).t().contiguous().to(DEV)
    j = 40
    Xj = X_cpu.clone()
    Xj[j] = float("nan")
    X, hx = guarded_B(Xj, DEV)
    R, hr = guarded_B(epi["residual"].t().contiguous(), DEV)
    Y, hy = guarded_C(n, KS_M, TORCH_DT[dtype], DEV)
    for again in ("", " relaunch"):
        plan.linear(X, out=Y, alpha=epi["alpha"], bias=epi["bias"].to(DEV), activation=epi["activation"], residual=R)
        torch.cuda.synchronize()
        plan.device_status()
        keep = [i for i in range(n) if i != j]
        assert bool(torch.isnan(Y[j]).all()), again
        assert_bits(Y[keep].contiguous(), ref[keep].contiguous(), "NaN token 40: the other rows" + again)
        for h, what in ((hy, "Y"), (hx, "X"), (hr, "residual")):
            assert_guards_intact(h, f"NaN token 40 {what}{again}")
        hy.refill()
    plan.free()


# ------------------------------------------------------------------ 6: the fallbacks are unchanged
def misaligned_B(B_cpu, device):
    """guarded_B with the payload 8 bytes past a 16-byte boundary: (X, the whole allocation)"""
    n, K = B_cpu.shape
    G = guard_elems(K)
    flat = torch.full((G + n * K + G + 4,), float("nan"), dtype=B_cpu.dtype, device=device)
    flat[G + 4:G + 4 + n * K].copy_(B_cpu.reshape(-1))
    x = flat[G + 4:G + 4 + n * K].view(n, K)
    assert x.data_ptr() % 16 == 8 and x.is_contiguous()
    return x, flat


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fallbacks_unchanged(dtype, mfma_everywhere):
    """what k_mfma_ks_tm does not run still takes the three launches at another token count, and is
    exact against the reference that rounds twice (at bf16 the two references differ)"""
    n = 72
    # X 8 bytes off a 16-byte boundary
    K = 1184
    X_cpu, prod = ks_operands(K, n, dtype)
    plan = ks_plan(K, W, dtype, 2)
    check_plan(plan, K, 2)
    epi = full_epilogue(KS_M, n, dtype)
    x, flat = misaligned_B(X_cpu, DEV)
    assert plan.linear_fused(n) == 1 and plan.linear_launches(n) == [3] and plan.linear_launches(n, x) == []
    ref = epilogue_ref(prod, dtype, False, **epi).t().contiguous().to(DEV)
    Y, hy = guarded_C(n, KS_M, TORCH_DT[dtype], DEV)
    for again in ("", " relaunch"):
        plan.linear(x, out=Y, alpha=epi["alpha"], bias=epi["bias"].to(DEV), activation=epi["activation"],
                    residual=epi["residual"].t().contiguous().to(DEV))
        torch.cuda.synchronize()
        plan.device_status()
        assert_bits(Y, ref, f"misaligned X {dtype}" + again)
        assert_guards_intact(hy, "misaligned X: Y" + again)
        hy.refill()
    G = guard_elems(K)
    assert bool(torch.isnan(flat[:G + 4]).all()) and bool(torch.isnan(flat[G + 4 + n * K:]).all())
    # LINEAR_FUSE = 0 on the same plan
    with config(LINEAR_FUSE=0):
        assert plan.linear_fused(n) == 0 and plan.linear_launches(n) == []
        run_linear(plan, X_cpu, prod, dtype, epi, f"LINEAR_FUSE=0 {dtype} n={n}", False)
    assert plan.linear_launches(n) == [3]
    plan.free()
    # K % 8 != 0
    K = 33
    X_cpu, prod = ks_operands(K, n, dtype)
    plan = ks_plan(K, W, dtype, 1)
    assert plan.info()["device_kernel"] == "k_mfma_ks", plan.info()
    assert plan.linear_fused(n) == 0 and plan.linear_launches(n) == []
    run_linear(plan, X_cpu, prod, dtype, full_epilogue(KS_M, n, dtype), f"K=33 {dtype} n={n}", False)
    plan.free()
    # window positions (fp16 plans only)
    if dtype == "f16":
        K = 1184
        X_cpu, prod = ks_operands(K, n, dtype)
        plan = ks_plan(K, W, dtype, 2, KS_WPOS=1)
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and info["ks_wpos"] == 1, info
        assert plan.linear_fused(n) == 0 and plan.linear_launches(n) == []
        run_linear(plan, X_cpu, prod, dtype, full_epilogue(KS_M, n, dtype), f"KS_WPOS n={n}", False)
        plan.free()


# ------------------------------------------------------------------ 7: the module
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_sparse_linear_at_another_token_count(dtype, mfma_everywhere):
    """a layer built with tokens=32 on (3, 25, K): 75 tokens, three tiles in one launch, bit for bit
    Plan.linear on the flattened input and the reference"""
    K = 1184
    row, col, val, dense = ks_pattern(K)
    bias = torch.arange(KS_M, dtype=torch.float32) - 60.0
    layer = gsa.SparseLinear.from_dense(torch.from_numpy(dense).float(), bias, tokens=W, dtype=dtype, activation="relu")
    assert layer.plan.info()["device_kernel"] == "k_mfma_ks", layer.plan.info()
    assert layer.plan.linear_fused(75) == 1 and layer.plan.linear_launches(75) == [3]
    x = int_B_cpu(K, 75, dtype, seed=1).t().contiguous().reshape(3, 25, K).to(DEV)
    y = layer(x)
    flat = layer.plan.linear(x.reshape(75, K), bias=bias.to(DEV), activation="relu")
    torch.cuda.synchronize()
    layer.plan.device_status()
    assert tuple(y.shape) == (3, 25, KS_M) and y.dtype == TORCH_DT[dtype]
    assert_bits(y.reshape(75, KS_M), flat, "SparseLinear.forward against Plan.linear")
    prod = dense @ x.reshape(75, K).t().cpu().double().numpy()
    assert np.abs(prod).max() <= 1024
    assert_bits(flat.cpu(), epilogue_ref(prod, dtype, True, bias=bias, activation="relu").t().contiguous(), "against the reference")
    layer.plan.free()
