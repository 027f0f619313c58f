"""GPU checks of the sampled product (Plan.sddmm / gs_sddmm, k_sddmm_tm):
out[e] = sum_t G[t][row_e] * X[t][col_e] over the plan's pattern in canonical order.

Integer operands in the style of tests/test_gpu_edges.py: G and X in {-2 .. 2}, n <= 100, so every sum
is an integer of magnitude <= 400 and exact in fp32 -- out must equal the numpy integer reference bit for
bit.  G and X sit between NaN bands (guarded_B: a read outside them poisons out), out between pattern
bands (guarded_C: a store outside it is seen, an entry never written stays NaN).  Every launch is
repeated into the NaN-refilled out.  The shapes stand where the kernel's boundaries are
(gs_sddmm_geometry): the row block, the column strip, the token chunk."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
import tolerance  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C, int_values  # noqa: E402
from test_gpu_edges import DEV, TORCH_DT, build  # noqa: E402
from test_gpu_edges_mfma import ks_pattern, mfma_everywhere  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu

RB, CS, TC = gsa.sddmm_geometry()
MS = (131, 120)              # an odd row stride (2-byte loads) and a last row block of 3 rows; 16-byte loads
KS = (40, CS + 72, CS + 75)  # one strip; two strips, the second with a partial 16-column tile; the same, odd stride
NS = (1, 24, 32, 33, 100)    # one token, a partial chunk, a full one, a full one + 1, three full + a partial
FULL_ROW, EMPTY_ROW = 7, 5


@functools.lru_cache(maxsize=None)
def pattern(M, K):
    """(row, col, val) in canonical order: 30% random, row 5 empty, row 7 full (with its duplicate: more
    than 64 entries inside strip 0 when K >= CS), (0, 0) and (M - 1, K - 1), columns CS - 1 and CS in a row
    of the first and of the last row block, the coordinate (7, 3) stored twice"""
    assert RB < M and CS - 1 < CS + 72 and TC == 32  # the cases are placed for these
    rng = np.random.default_rng(17 * M + K)
    mask = rng.random((M, K)) < 0.3
    mask[EMPTY_ROW] = False
    mask[FULL_ROW] = True
    mask[0, 0] = mask[M - 1, K - 1] = True
    if K > CS:
        mask[[1, M - 1], CS - 1] = mask[[1, M - 1], CS] = True
    r, c = np.nonzero(mask)
    at = int(np.flatnonzero((r == FULL_ROW) & (c == 3))[0])
    r, c = np.insert(r, at, FULL_ROW), np.insert(c, at, 3)
    return r.astype(np.uint64), c.astype(np.uint64), int_values(len(r), M + K)


@functools.lru_cache(maxsize=None)
def operands(M, K, n, dtype):
    """(G: n x M, X: n x K on the CPU, the exact out as float32 (nnz, 1)); never written"""
    g = torch.Generator()
    g.manual_seed(1000 * M + 10 * K + n)
    G = torch.randint(-2, 3, (n, M), generator=g)
    X = torch.randint(-2, 3, (n, K), generator=g)
    row, col, _ = pattern(M, K)
    full = G.numpy().T.astype(np.int64) @ X.numpy().astype(np.int64)
    ref = full[row.astype(np.int64), col.astype(np.int64)]
    assert np.abs(ref).max() <= 400
    return G.to(TORCH_DT[dtype]), X.to(TORCH_DT[dtype]), torch.from_numpy(ref.astype(np.float32)).reshape(-1, 1)


def make_plan(M, K, dtype, pipe=("block_total", 40, 1)):
    row, col, val = pattern(M, K)
    plan = build(M, K, row, col, val, pipe[0], pipe[1], pipe[2], 32, dtype)
    r, c = plan.pattern()
    assert np.array_equal(r, row) and np.array_equal(c, col)
    return plan


def run_sddmm(plan, G_cpu, X_cpu, ref_cpu, what):
    """one guarded Plan.sddmm and a relaunch into the NaN-refilled out: bit-exact, every band intact;
    returns out's bits (a CPU copy)"""
    G, hg = guarded_B(G_cpu, DEV)
    X, hx = guarded_B(X_cpu, DEV)
    out, ho = guarded_C(ref_cpu.shape[0], 1, torch.float32, DEV)
    ref = ref_cpu.to(DEV)
    bits = None
    for again in ("", " relaunch"):
        got = plan.sddmm(G, X, out=out)
        assert got is out
        torch.cuda.synchronize()
        assert_bits(out, ref, what + again)
        for h, name in ((ho, "out"), (hg, "G"), (hx, "X")):
            assert_guards_intact(h, what + again + " " + name)
        bits = out.cpu().clone()
        ho.refill()
    plan.device_status()
    return bits


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("M", MS)
def test_exact_on_the_boundaries(M, K, dtype):
    plan = make_plan(M, K, dtype)
    assert plan.info()["nnz"] == len(pattern(M, K)[0])
    for n in NS:
        G, X, ref = operands(M, K, n, dtype)
        run_sddmm(plan, G, X, ref, f"k_sddmm_tm {dtype} M={M} K={K} n={n}")
    plan.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_prepare_then_the_same_bits(dtype):
    """sddmm_prepare uploads the pattern ahead of the first call; out allocated by the call"""
    M, K, n = 131, CS + 75, 33
    plan = make_plan(M, K, dtype).sddmm_prepare()
    G, X, ref = operands(M, K, n, dtype)
    out = plan.sddmm(G.to(DEV), X.to(DEV))
    assert out.dtype == torch.float32 and tuple(out.shape) == (ref.shape[0],)
    assert_bits(out.reshape(-1, 1), ref.to(DEV), "allocated out")
    plan.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("which", ["X", "G"])
def test_one_nan_stays_in_its_column_or_row(which, dtype):
    """one NaN at X[t][j]: exactly the entries of column j are NaN, every other entry keeps its bits (a
    zero of the other image times the NaN would spread it); the same for G[t][i] and row i"""
    M, K, n = 131, CS + 72, 33
    plan = make_plan(M, K, dtype)
    row, col, _ = pattern(M, K)
    G, X, ref = operands(M, K, n, dtype)
    G, X = G.clone(), X.clone()
    if which == "X":
        j = CS + 70  # in the partial tile of the second strip
        X[n - 1, j] = float("nan")
        hit = col == j
    else:
        i = M - 2    # in the 3-row last block
        G[0, i] = float("nan")
        hit = row == i
    assert 0 < hit.sum() < len(row)
    out = plan.sddmm(G.to(DEV), X.to(DEV)).cpu()
    nan = torch.isnan(out).numpy()
    assert np.array_equal(nan, hit), (int(nan.sum()), int(hit.sum()))
    keep = torch.from_numpy(~hit)
    assert torch.equal(out[keep].view(torch.int32), ref.reshape(-1)[keep].view(torch.int32))
    plan.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_misaligned_x_and_g(dtype):
    """x (then g) 2 bytes into its allocation: not 16-byte aligned, the 2-byte loads; the same bits"""
    M, K, n = 120, CS + 72, 33
    plan = make_plan(M, K, dtype)
    G, X, ref = operands(M, K, n, dtype)

    def shifted(t):
        flat = torch.full((t.numel() + 8,), float("nan"), dtype=t.dtype, device=DEV)
        v = flat[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 2 and v.is_contiguous()
        return v

    for g, x, what in ((G.to(DEV), shifted(X), "x"), (shifted(G), X.to(DEV), "g")):
        out = plan.sddmm(g, x)
        assert_bits(out.reshape(-1, 1), ref.to(DEV), f"misaligned {what}")
    plan.free()


def test_gaussian_on_the_fp32_contract_line():
    """f16 Gaussian operands against float64: fp32 sums of exact products, held to the fp32 line"""
    M, K, n = 131, CS + 72, 100
    plan = make_plan(M, K, "f16")
    row, col, _ = pattern(M, K)
    g = torch.Generator()
    g.manual_seed(5)
    G = torch.randn(n, M, generator=g).half()
    X = torch.randn(n, K, generator=g).half()
    ref = (G.double().numpy().T @ X.double().numpy())[row.astype(np.int64), col.astype(np.int64)]
    out = plan.sddmm(G.to(DEV), X.to(DEV)).cpu().numpy()
    err = tolerance.rel_err(out.astype(np.float64), ref)
    print(f"k_sddmm_tm f16 Gaussian n={n}: max rel err {err:.3g} (bound {tolerance.TOL['f32']})")
    assert err <= tolerance.TOL["f32"], err
    plan.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_the_plan_family_does_not_matter(dtype):
    """the same call on a gather-family plan of the same matrix: the kernel reads only the pattern"""
    M, K, n = 131, CS + 75, 100
    G, X, ref = operands(M, K, n, dtype)
    bits = []
    for pipe in (("block_total", 40, 1), ("warp_total", 0, 1)):
        plan = make_plan(M, K, dtype, pipe)
        bits.append((plan.info()["device_kernel"] or plan.info()["kernel_name"],
                     run_sddmm(plan, G, X, ref, f"k_sddmm_tm on a {pipe[0]} plan")))
        plan.free()
    assert bits[0][0] != bits[1][0], bits[0][0]
    assert torch.equal(bits[0][1].view(torch.int32), bits[1][1].view(torch.int32))


def test_an_fp8_weight_plan_is_an_f16_plan_here(mfma_everywhere):
    """the weights' storage does not matter to G and X: the FP8-weight plan of a pattern gives the f16 plan's bits"""
    K, n, M = 1176, 33, 131
    row, col, val, _ = ks_pattern(K)
    g = torch.Generator()
    g.manual_seed(3)
    G, X = torch.randint(-2, 3, (n, M), generator=g).half().to(DEV), torch.randint(-2, 3, (n, K), generator=g).half().to(DEV)
    ref = (G.double().t() @ X.double())[torch.from_numpy(row.astype(np.int64)).to(DEV), torch.from_numpy(col.astype(np.int64)).to(DEV)]
    for weights in (None, "fp8"):
        plan = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", 32, 40, 1).compile().upload("f16", 0, weights=weights)
        assert plan.info()["weights"] == (1 if weights else 0) and plan.info()["device_kernel"] == "k_mfma_ks"
        out = plan.sddmm(G, X)
        assert_bits(out.reshape(-1, 1), ref.float().reshape(-1, 1), f"sddmm on a plan with weights={weights}")
        plan.free()


def test_refusals_leave_out_untouched():
    M, K, n = 120, 40, 24
    G, X, ref = operands(M, K, n, "f16")
    row, col, val = pattern(M, K)
    nnz = len(row)
    plan = make_plan(M, K, "f16")
    g, x = G.to(DEV), X.to(DEV)
    out = torch.full((nnz,), 7.0, device=DEV)
    with pytest.raises(TypeError):
        plan.sddmm(g.bfloat16(), x.bfloat16(), out)  # not the plan's dtype
    with pytest.raises(ValueError, match="device"):
        plan.sddmm(G, X, out)                        # CPU tensors
    for bad in (torch.zeros(nnz + 1, device=DEV), torch.zeros(nnz, device=DEV, dtype=torch.float16),
                torch.zeros(nnz), torch.zeros(2 * nnz, device=DEV)[::2]):
        with pytest.raises(ValueError, match="out"):
            plan.sddmm(g, x, bad)
    plan.free()
    # an f32 plan has no sampled product: refused by the library with a message, before any launch
    p32 = build(M, K, row, col, val, "block_total", 40, 1, 32, "f32")
    with pytest.raises(TypeError):
        p32.sddmm(g.float(), x.float(), out)
    rc = p32._L.gs_sddmm(p32._h, ctypes.c_void_p(g.data_ptr()), ctypes.c_void_p(x.data_ptr()), n,
                         ctypes.c_void_p(out.data_ptr()), None)
    assert rc == -1 and "f16 and bf16" in p32._L.gs_last_error().decode()
    with pytest.raises(gsa.GsError, match="f16 and bf16"):
        p32.sddmm_prepare()
    torch.cuda.synchronize()
    assert (out == 7).all()
    p32.free()
