"""Every (RT, MAXG) instantiation pair of the k_mfma_ks family through every launcher that dispatches on it:
the launch files turn a plan's row tiles per block (RT, 2 .. 8) and entry groups per lane per k-step (MAXG,
1 .. 4) into template arguments, and a transposed or shifted argument there shows only on a plan of that pair.

One small matrix per pair: two row blocks of block_total(rows, 1), rows = 16 RT - 3, the second one ragged
(rows // 2 + 1 rows), K = 136 (three full k-steps and a short one; a multiple of 8 for the token-major
form), its density chosen for MAXG: a k-step of a full block holds about rows * 32 * density / 8 entry groups
over 64 lanes.  The pairs the upload layout cannot produce at these sizes, and which are therefore not run:
(2, 3), (2, 4) and (3, 4) -- a full 29-row block holds at most 116 groups per k-step (MAXG 2), a 45-row one
at most 180 (MAXG 3).  test_the_patterns_produce_the_pinned_pairs holds the inputs to exactly CASES on the
CPU, from the instantiation the emitted program names (as tests/test_ks_layout.py reads it).

Each case runs spmm at N = 32 in fp16 and bf16 (k_mfma_ks), a two-entry Batch in both (k_mfma_ks_group),
linear at 40 tokens -- two token tiles, the second partial -- in both (k_mfma_ks_tm), and spmm and linear on
FP8 weights (k_mfma_ks_w8, k_mfma_ks_tm with VB = 8).  Half of the cases run with KS_NT = 1, the RT = 5 ones
with KS_SPLIT = 2.  Values as in tests/test_gpu_exact.py: A in {+-1, +-2} (exact e4m3 codes under the default
power-of-two scales), B and X in {-2 .. 2}; every partial sum is an integer below 2^24, so each result is the
float64 product rounded once to the plan's dtype, bit for bit.  plan.device_status() after each case."""
import contextlib
import functools
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402

DEV = "cuda:0"
K, N, TOKENS = 136, 32, 40
TORCH_DT = {"f16": torch.float16, "bf16": torch.bfloat16}
UNREACHABLE = {(2, 3), (2, 4), (3, 4)}
CASES = [(rt, g) for rt in range(2, 9) for g in range(1, 5) if (rt, g) not in UNREACHABLE]


def rows_of(rt):
    return 16 * rt - 3


def overrides(rt, maxg):
    """the fill limit and the k_mfma_ks row threshold lowered so that these small patterns take the kernel"""
    return {"HALF": 1, "MFMA_MAX_FILL": 1 << 30, "KS_MIN_ROWS": 17, "KS_NT": (rt + maxg) % 2, "KS_SPLIT": 2 if rt == 5 else 1}


@contextlib.contextmanager
def config(**over):
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        yield
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


@functools.lru_cache(maxsize=None)
def pattern(rt, maxg):
    """(M, row, col, val, dense float64 A): the corners of both blocks stored, values in {+-1, +-2}"""
    rows = rows_of(rt)
    M = rows + rows // 2 + 1
    rng = np.random.default_rng(1000 * rt + maxg)
    mask = rng.random((M, K)) < (maxg - 0.5) * 16.0 / rows
    for r in (0, rows - 1, rows, M - 1):
        mask[r, 0] = mask[r, K - 1] = True
    r, c = np.nonzero(mask)
    val = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), len(r))
    A = np.zeros((M, K), np.float64)
    A[r, c] = val
    return M, r.astype(np.uint64), c.astype(np.uint64), val, A


def compiled(rt, maxg):
    M, row, col, val, _ = pattern(rt, maxg)
    return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", N, rows_of(rt), 1).compile()


@pytest.mark.parametrize("rt,maxg", CASES)
def test_the_patterns_produce_the_pinned_pairs(tmp_path, rt, maxg):
    with config(**overrides(rt, maxg)):
        d = compiled(rt, maxg).generate_program(str(tmp_path), repeat=1)
    src = open(os.path.join(d, "kernel_file.hip")).read()
    m = re.search(r"gsk::k_mfma_ks<(\d+), (\d+), (\d+), (\d+), (\d+)", src)
    assert m, src[:400]
    CT, RT, W, D, MAXG = map(int, m.groups())
    assert (CT, RT, W, MAXG) == (2, rt, 8, maxg), (rt, maxg, m.group(0))


def test_the_case_list_is_every_reachable_pair():
    assert len(CASES) == 25 and set(CASES) | UNREACHABLE == {(rt, g) for rt in range(2, 9) for g in range(1, 5)}
    # a k-step of a full block holds at most rows * 32 / 8 entry groups over 64 lanes
    assert UNREACHABLE == {(rt, g) for rt in range(2, 9) for g in range(1, 5) if 64 * (g - 1) >= rows_of(rt) * 4}


@functools.lru_cache(maxsize=None)
def operands(rt, maxg):
    """B0, B1 (K x N) and X (TOKENS x K), integers in {-2 .. 2} as float64, and the exact products"""
    _, _, _, _, A = pattern(rt, maxg)
    rng = np.random.default_rng(7 * rt + maxg)
    B0, B1 = (rng.integers(-2, 3, (K, N)).astype(np.float64) for _ in range(2))
    X = rng.integers(-2, 3, (TOKENS, K)).astype(np.float64)
    return B0, B1, X, A @ B0, A @ B1, X @ A.T


def assert_bits(got, exact, dt, what):
    want = torch.from_numpy(exact).to(dt)  # integers below 2^24: one rounding, the kernel's
    bad = (got.cpu().view(torch.int16) != want.view(torch.int16)).nonzero()
    assert len(bad) == 0, f"{what}: {len(bad)} elements differ, first at {bad[0].tolist()}: " \
                          f"{got[tuple(bad[0])].item()} vs {want[tuple(bad[0])].item()}"


def check_plan(plan, rt, maxg, dtype, what, grouped):
    M = pattern(rt, maxg)[0]
    B0, B1, X, C0, C1, Y = operands(rt, maxg)
    dt = TORCH_DT[dtype]
    over = overrides(rt, maxg)
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ks_nt"] == over["KS_NT"] and info["ksplit"] == over["KS_SPLIT"], info
    assert plan.linear_fused(TOKENS) == 1, info
    nan = lambda r, c: torch.full((r, c), float("nan"), device=DEV, dtype=dt)  # noqa: E731
    b0, b1, x = (torch.from_numpy(t).to(dt).to(DEV) for t in (B0, B1, X))
    c = nan(M, N)
    plan.spmm(b0, C=c)
    y = nan(TOKENS, M)
    plan.linear(x, out=y)
    torch.cuda.synchronize()
    assert_bits(c, C0, dt, what + " spmm N=32")
    assert_bits(y, Y, dt, what + f" linear n={TOKENS}")
    if grouped:
        plan.add_replica()
        g0, g1 = nan(M, N), nan(M, N)
        bat = gsa.Batch([(plan, 0, b0, g0), (plan, 1, b1, g1)], N)
        assert bat.launches() == [2], bat.launches()
        bat.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert_bits(g0, C0, dt, what + " batch entry 0")
        assert_bits(g1, C1, dt, what + " batch entry 1")
    plan.device_status()
    plan.free()


@pytest.mark.gpu
@pytest.mark.parametrize("rt,maxg", CASES)
def test_every_launcher_on_every_pair(rt, maxg):
    what = f"RT={rt} MAXG={maxg}"
    with config(**overrides(rt, maxg)):
        for dtype in ("f16", "bf16"):
            check_plan(compiled(rt, maxg).upload(dtype, 0), rt, maxg, dtype, f"{what} {dtype}", True)
        p8 = compiled(rt, maxg).upload("f16", 0, weights="fp8")
        assert p8.info()["weights"] == 1
        check_plan(p8, rt, maxg, "f16", what + " FP8 weights", False)
