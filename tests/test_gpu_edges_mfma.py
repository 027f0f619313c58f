"""Edge sweeps of the matrix-core kernels on guarded operands (tests/guarded.py), with the integer
operands, the float64 reference and the three checks per launch of tests/test_gpu_edges.py.

C2 k_mfma_ks with more than one column tile and a partial last one.
C3 k_mfma_ks K edges: the last k-step short, per-wave step counts around 2 * depth.
C4 k_mfma_rows and k_nm_mfma once each.

plan.info() names the kernel and the K ranges, not the column tiles, the waves or the pipeline
depth of a launch.  ks_column_tiles below is a copy of the upload's rule (device_layout.hpp
ks_ct_rt; a 128-column plan that would spill is built on 64-column tiles instead, which the
assertions allow for by N % 64 != 0): nothing ties it to the tile width the launch used.  The
per-wave step counts of the K edges likewise assume the kernel's defaults, 8 waves and depth 2
(kKsWaves, kKsDepth)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from generalsparse_amd import datasets as ds  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C, int_values  # noqa: E402
from test_gpu_edges import DEV, build, dense_f64, exact_ref, int_B_cpu, run_guarded  # noqa: E402

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ k_mfma_ks
@pytest.fixture
def mfma_everywhere():
    """the fill limit raised so that these small patterns take the matrix-core kernels"""
    old = gsa.get_config("MFMA_MAX_FILL")
    gsa.set_config("MFMA_MAX_FILL", 1 << 30)
    yield
    gsa.set_config("MFMA_MAX_FILL", old)


KS_M = 131  # 40-row blocks: 40, 40, 40, 11; 80-row blocks: 80, 51


@functools.lru_cache(maxsize=None)
def ks_pattern(K, seed=0):
    """131 x K, 30% dense but at most 200 nonzeros per row, integer values; an entry at column
    K - 1 in the last row of every 40- and 80-row block (rows 39, 79, 119, 130) and at column 0"""
    rng = np.random.default_rng(100 + K + seed)
    mask = rng.random((KS_M, K)) < min(0.3, 200.0 / K)
    mask[[39, 79, 119, 130], K - 1] = True
    mask[[0, 39, 130], 0] = True
    assert mask.sum(1).max() <= 256
    r, c = np.nonzero(mask)
    row, col = r.astype(np.uint64), c.astype(np.uint64)
    val = int_values(len(row), K)
    return row, col, val, dense_f64(KS_M, K, row, col, val)


@functools.lru_cache(maxsize=None)
def ks_case(K, N, dtype):
    B = int_B_cpu(K, N, dtype, seed=1)
    return B, exact_ref(ks_pattern(K)[3], B, dtype)


def ks_ranges(K, split):
    """K ranges of a k_mfma_ks plan at KS_SPLIT = split > 0 (device_layout.cc build_ks_tiles): at most
    one per 32-row k-step, ranges of whole k-steps, none empty"""
    S = max(1, min(split, (K + 31) // 32))
    KR = ((K + S - 1) // S + 31) // 32 * 32
    return (K + KR - 1) // KR


def ks_column_tiles(N, rows):
    """(column tiles, columns per tile) of a k_mfma_ks launch: 16-column tiles, 1 / 2 / 4 per
    workgroup at N <= 16 / <= 32 / above, 8 at N >= 128 for row blocks of at most 48 rows"""
    rt = max(2, (rows + 15) // 16)
    ct = 8 if (N >= 128 and rt <= 3) else (1 if N <= 16 else (2 if N <= 32 else 4))
    return (N + 16 * ct - 1) // (16 * ct), 16 * ct


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("rows", [40, 80])
def test_ks_column_tiles(rows, split, dtype, mfma_everywhere):
    """C2: gridDim.y > 1 with nv < 16 * CT in the last tile, where the arrival, slab and error-word
    indexing by gridDim.y meets the partial tile"""
    K = 640
    row, col, val, _ = ks_pattern(K)
    ran = []
    for N in (40, 72, 136, 200):
        B, ref = ks_case(K, N, dtype)
        plan = build(KS_M, K, row, col, val, "block_total", rows, 1, N, dtype, over={"KS_SPLIT": split})
        info = plan.info()
        tiles, width = ks_column_tiles(N, rows)
        if info["device_kernel"] == "k_mfma_ks":
            assert info["ksplit"] == ks_ranges(K, split), info
            ran.append(N)
            if N in (72, 136):
                # (a 128-column plan that would spill is built on 64-column tiles: more tiles, the last still partial)
                assert tiles > 1 and N % width != 0 and N % 64 != 0, (N, tiles, width)
        run_guarded(plan, B, ref, f"block_total({rows}) {dtype} N={N} KS_SPLIT={split} {info['device_kernel']}")
        plan.free()
    assert 72 in ran and 136 in ran, ran


KS_EDGE_K = [20, 33, 100, 257, 901, 1057, 1183]


def test_ks_edge_steps_are_what_the_cases_say():
    """full 32-row k-steps and the short last step's rows, and the full steps per wave (8 waves
    take the steps round-robin) around 2 * depth = 4"""
    want = {20: (0, 20), 33: (1, 1), 100: (3, 4), 257: (8, 1), 901: (28, 5), 1057: (33, 1), 1183: (36, 31)}
    for K, (full, tail) in want.items():
        assert (K // 32, K % 32) == (full, tail)
    per_wave = {K: [len(range(w, K // 32, 8)) for w in range(8)] for K in (901, 1057, 1183)}
    assert per_wave == {901: [4, 4, 4, 4, 3, 3, 3, 3], 1057: [5, 4, 4, 4, 4, 4, 4, 4], 1183: [5, 5, 5, 5, 4, 4, 4, 4]}
    assert ks_ranges(100, 3) == 2 and ks_ranges(20, 3) == 1 and ks_ranges(1183, 3) == 3


@pytest.mark.parametrize("split", [1, 3])
@pytest.mark.parametrize("rows", [40, 80])
@pytest.mark.parametrize("K", KS_EDGE_K)
def test_ks_k_edges(K, rows, split, mfma_everywhere):
    """C3: the NaN band starts right after row K - 1 of B, so a short k-step run in the fast form
    (B rows stored without the zero selects) turns its row block NaN; N = 32 is a full tile (fast
    form eligible), 24 a partial one (general form), 72 both in one launch"""
    row, col, val, _ = ks_pattern(K)
    assert (col == K - 1).any() and set(row[col == K - 1].astype(int)) >= {39, 79, 119, 130}
    for N, nt in ((32, 0), (32, 1), (24, 0), (72, 0)):
        B, ref = ks_case(K, N, "f16")
        plan = build(KS_M, K, row, col, val, "block_total", rows, 1, N, "f16", over={"KS_SPLIT": split, "KS_NT": nt})
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split), info
        if N == 32:
            assert info["ks_nt"] == nt, info
        run_guarded(plan, B, ref, f"K={K} block_total({rows}) N={N} KS_SPLIT={split} KS_NT={nt}")
        plan.free()


@pytest.mark.parametrize("K", [901, 1183])
def test_ks_k_edges_grouped(K, mfma_everywhere):
    """the same edges through k_mfma_ks_group: one gsa.Batch of two replicas, both outputs guarded"""
    N = 32
    row, col, val, _ = ks_pattern(K)
    B_cpu, ref_cpu = ks_case(K, N, "f16")
    plan = build(KS_M, K, row, col, val, "block_total", 40, 1, N, "f16", over={"KS_SPLIT": 3})
    assert plan.info()["device_kernel"] == "k_mfma_ks" and plan.info()["ksplit"] == 3, plan.info()
    plan.add_replica()
    B, hb = guarded_B(B_cpu, DEV)
    outs = [guarded_C(KS_M, N, torch.float16, DEV) for _ in range(2)]
    bat = gsa.Batch([(plan, i, B, C) for i, (C, _) in enumerate(outs)], N)
    assert bat.launches() == [2], bat.launches()
    ref = ref_cpu.to(DEV)
    for again in ("", " relaunch"):
        bat.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        plan.device_status()
        for i, (C, hc) in enumerate(outs):
            assert_bits(C, ref, f"K={K} grouped entry {i}{again}")
            assert_guards_intact(hc, f"K={K} grouped entry {i}{again} C")
            hc.refill()
        assert_guards_intact(hb, f"K={K} grouped{again} B")
    plan.free()


# ------------------------------------------------------------------ C4: the other matrix-core paths
@pytest.mark.parametrize("N", [8, 64])
@pytest.mark.parametrize("rows", [20, 33])
def test_mfma_rows_guarded(rows, N, mfma_everywhere):
    K = 640
    row, col, val, _ = ks_pattern(K)
    B, ref = ks_case(K, N, "f16")
    plan = build(KS_M, K, row, col, val, "block_total", rows, 1, N, "f16")
    kernel = plan.info()["device_kernel"]
    assert kernel == "k_mfma_rows", plan.info()
    run_guarded(plan, B, ref, f"block_total({rows}) N={N} {kernel}")
    plan.free()


@pytest.mark.parametrize("N", [8, 128])
def test_nm_mfma_guarded(N):
    M, K = 333, 772
    row, col, _ = ds.two_four(M, K, 3)
    val = int_values(len(row), 9)
    B = int_B_cpu(K, N, "f16", seed=2)
    ref = exact_ref(dense_f64(M, K, row, col, val), B, "f16")
    plan = build(M, K, row, col, val, "col_direction_nm", 32, 1, N, "f16")
    assert plan.info()["device_kernel"] == "k_nm_mfma", plan.info()
    run_guarded(plan, B, ref, f"k_nm_mfma N={N}")
    plan.free()
