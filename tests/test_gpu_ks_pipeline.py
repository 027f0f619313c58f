"""k_mfma_ks's load pipeline at its edges, bit for bit (integer known answers as tests/test_gpu_exact.py:
A in {+-1, +-2}, B in {-2..2}, every partial sum an exact fp32 integer, so C == fp16(exact) whatever the
order of loads, K ranges and slab combine).

The step loop runs on D = kKsDepth = 2 register slots per wave, primed by a prologue (by the head-step
layout or by step records) and reloaded two steps ahead; its iterations are fast ones (whole k-steps)
and general ones (the last K range of a K that is no multiple of 32).  What can go wrong is how many
steps a wave owns relative to D, the head-step slots and the hand-over from the fast to the general
iterations, so the cases are:

- M = 80 as two 40-row blocks under block_total(40,1) (KS_MIN_ROWS = 40: k_mfma_ks, asserted), 8 waves;
- NS k-steps per K range in {1, 8, 9, 16, 17, 24, 25, 40}: waves holding 0, 1, 2 = D, 3, 4 and 5 steps,
  16 = W * D being exactly the head steps of a unit;
- K = 32 * NS * S (every step whole) and 32 * NS * S - 13 (a short last step), KS_SPLIT S in {1, 2}
  (build_ks_tiles: K range = ceil(K / S) rounded up to 32 columns, so either K gives NS steps per range);
- density 0.3 (48 groups per step: one group load per lane, 5 loads per slot) and 0.9 (144 groups:
  MAXG = 3, 9 loads per slot), the same entry count in every whole (row block, k-step) tile so that the
  head-step layout pads nothing and is taken whenever KS_HEAD is on;
- N in {32, 8}, KS_NT in {0, 1}, KS_HEAD on and off;
- one bf16 plan, and one grouped launch (gs_spmm_batch) of three entries with NS = 1, 17 and 40.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, M = 40, 80
NS_CASES = (1, 8, 9, 16, 17, 24, 25, 40)


@functools.lru_cache(maxsize=None)
def pattern(K, density):
    """COO of an M x K matrix with round(density * 40 * w) entries in every 40-row x w-column tile
    (w = 32, or what is left of K), values in {+-1, +-2}"""
    rng = np.random.default_rng(1000 * K + int(100 * density))
    rows, cols = [], []
    for b in range(M // ROWS):
        for c0 in range(0, K, 32):
            w = min(32, K - c0)
            cell = rng.choice(ROWS * w, int(round(density * ROWS * w)), replace=False)
            rows.append(b * ROWS + cell // w)
            cols.append(c0 + cell % w)
    row, col = np.concatenate(rows), np.concatenate(cols)
    order = np.lexsort((col, row))
    row, col = row[order].astype(np.uint64), col[order].astype(np.uint64)
    val = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), len(row))
    return row, col, val


@functools.lru_cache(maxsize=None)
def known_answer(K, density, N, tdt):
    """B in {-2..2} and tdt(A @ B) from the exact integer product (float64 on the GPU), once per case"""
    row, col, val = pattern(K, density)
    g = torch.Generator(device=DEV)
    g.manual_seed(7 * K + N)
    B = torch.randint(-2, 3, (K, N), device=DEV, generator=g).to(tdt)
    A = torch.zeros((M, K), dtype=torch.float64, device=DEV)
    A[torch.from_numpy(row.astype(np.int64)).to(DEV), torch.from_numpy(col.astype(np.int64)).to(DEV)] = \
        torch.from_numpy(val.astype(np.float64)).to(DEV)
    exact = A @ B.double()
    assert exact.abs().max().item() < 2 ** 15  # exact in fp32, finite in fp16 / bf16: one rounding
    return B, exact.to(tdt)


def build(K, density, N, dtype="f16", **over):
    row, col, val = pattern(K, density)
    over["KS_MIN_ROWS"] = ROWS
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", N, ROWS, 1).compile().upload(dtype, 0)
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def assert_bits(C, ref, what):
    assert C.dtype == ref.dtype and C.shape == ref.shape, what
    bad = C.view(torch.int16) != ref.view(torch.int16)
    n_bad = int(bad.sum().item())
    if n_bad:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n_bad} elements differ, first at {i}: {C[i[0], i[1]].item()} vs "
                             f"{ref[i[0], i[1]].item()}")


def check_plan(plan, S, nt, head, whole, what):
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == S and info["lds_waves"] == 8, (what, info)
    assert info["ks_nt"] == nt, (what, info)
    # equal tiles pad no head step, so the layout is taken when it is on (a short last step holds
    # fewer entries: there the upload decides, and either form must be right)
    if not head:
        assert info["ks_head_groups"] == 0, (what, info)
    elif whole:
        assert info["ks_head_groups"] > 0, (what, info)


@pytest.mark.parametrize("density", [0.3, 0.9])
@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("NS", NS_CASES)
def test_steps_per_wave_against_depth(NS, S, density):
    for short in (0, 13):
        K = 32 * NS * S - short
        for N in (32, 8):
            B, ref = known_answer(K, density, N, torch.float16)
            for nt in (0, 1):
                for head in (1, 0):
                    what = f"NS={NS} S={S} K={K} density={density} N={N} KS_NT={nt} KS_HEAD={head}"
                    plan = build(K, density, N, KS_SPLIT=S, KS_NT=nt, KS_HEAD=head)
                    # (non-temporal loads are built for 32- and 128-column tiles: N = 8 keeps plain loads)
                    check_plan(plan, S, nt if N == 32 else 0, head, short == 0, what)
                    C = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float16)
                    plan.spmm(B, C=C)
                    torch.cuda.synchronize()
                    assert_bits(C, ref, what)
                    plan.device_status()
                    plan.free()


def test_bf16_twin():
    NS, S, density, N = 17, 2, 0.3, 32
    K = 32 * NS * S - 13
    B, ref = known_answer(K, density, N, torch.bfloat16)
    plan = build(K, density, N, dtype="bf16", KS_SPLIT=S, KS_NT=1)
    check_plan(plan, S, 1, 1, False, "bf16")
    assert plan.info()["dtype"] == 2
    C = torch.full((M, N), float("nan"), device=DEV, dtype=torch.bfloat16)
    plan.spmm(B, C=C)
    torch.cuda.synchronize()
    assert_bits(C, ref, "bf16")
    plan.device_status()
    plan.free()


def test_grouped_launch_of_three_step_counts():
    """gs_spmm_batch: one k_mfma_ks_group launch whose entries hold 1, 17 and 40 steps per K range"""
    N, density = 32, 0.3
    shapes = ((1, 1, 0), (17, 2, 13), (40, 1, 0))  # NS, S, columns short of 32 * NS * S
    plans, entries, refs = [], [], []
    for NS, S, short in shapes:
        K = 32 * NS * S - short
        B, ref = known_answer(K, density, N, torch.float16)
        plan = build(K, density, N, KS_SPLIT=S)
        check_plan(plan, S, 0, 1, short == 0, f"group NS={NS}")
        plans.append(plan)
        entries.append((plan, 0, B, torch.full((M, N), float("nan"), device=DEV, dtype=torch.float16)))
        refs.append(ref)
    bat = gsa.Batch(entries, N)
    assert bat.launches() == [3], bat.launches()
    bat.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for (NS, S, short), e, ref in zip(shapes, entries, refs):
        assert_bits(e[3], ref, f"group entry NS={NS} S={S}")
    for plan in plans:
        plan.device_status()
        plan.free()
