"""bfloat16 plans on the GPU (GS_BF16): the K-split matrix-core kernel k_mfma_ks and every gather
family, through the Python surface.

Tolerance.  Every kernel accumulates in fp32 and rounds once, to nearest even, when it stores C,
so against a reference computed from the already-rounded operands the expected error is one bf16
half-ulp: at most 2^-8 relative (8 significant bits), 2^-9 at the top of a binade.  The bound is
TIGHT_BF16 = 2^-7 relative to max(1, |ref|), set after the project's rule for fp16
(tests/tolerance.py: 2^-9 for a 2^-11 half-ulp); the measured maxima are 0.0039.  References are
oracle_ffi.spmm_ref(..., "f64") on A's values and B rounded to bf16 first; the integer cases use
a float64 dense product on the GPU (exact), as tests/test_gpu_exact.py does."""
import functools

import numpy as np
import pytest

import oracle_ffi as ofi

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from generalsparse_amd import datasets as ds  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIGHT_BF16 = 2.0 ** -7
BF = torch.bfloat16


def round_bf16(x):
    """float32 array rounded to bf16 and back (numpy has no bfloat16)"""
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(BF).float().numpy()


def build(M, K, row, col, val, pipeline, p0, p1, N, dtype="bf16", over=None):
    over = over or {}
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline(pipeline, N, p0, p1).compile().upload(dtype, 0)
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def rel_err(C, ref):
    C, ref = np.asarray(C, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(C - ref) / np.maximum(1.0, np.abs(ref))).max())


def assert_bits(C, ref, what):
    assert C.dtype == BF and ref.dtype == BF
    bad = C.view(torch.int16) != ref.view(torch.int16)
    n_bad = int(bad.sum().item())
    if n_bad:
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {n_bad} elements differ, first at {i}: {C[i[0], i[1]].item()} vs "
                             f"{ref[i[0], i[1]].item()}")


# ------------------------------------------------------------------ the base shape (k_mfma_ks)
M0, K0 = 640, 2048  # 8 row blocks of 80 rows, 64 k-steps; a partial last block at 112 rows


@functools.lru_cache(maxsize=None)
def base_pattern():
    row, col, val = ds.pruned_weight(M0, K0, 0.7, 5)
    ival = np.random.default_rng(5).choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), len(row))
    return row, col, val, ival


@functools.lru_cache(maxsize=None)
def int_case(N):
    """B in {-2..2} as bf16 and bf16(A @ B) from the exact integer product, computed once per N"""
    row, col, _, ival = base_pattern()
    g = torch.Generator(device=DEV)
    g.manual_seed(100 + N)
    B = torch.randint(-2, 3, (K0, N), device=DEV, generator=g).to(BF)
    A = torch.zeros((M0, K0), dtype=torch.float64, device=DEV)
    A[torch.from_numpy(row.astype(np.int64)).to(DEV), torch.from_numpy(col.astype(np.int64)).to(DEV)] = \
        torch.from_numpy(ival.astype(np.float64)).to(DEV)
    exact = A @ B.double()
    assert exact.abs().max().item() < 2 ** 24  # every partial sum an exact fp32 integer
    return B, exact.float().to(BF)


# (rows, N) on k_mfma_ks at fp16 and bf16 alike: 112-row blocks (RT 7) are built for tiles of at
# most 32 columns, so (112, 64) and (112, 128) run another kernel at either type (tested below)
KS_CASES = [(rows, N, split, nt) for rows in (40, 80, 112) for N in (8, 32, 64, 128) if not (rows == 112 and N > 32)
            for split in (0, 1, 3) for nt in ((0, 1) if N == 32 else (0,))]


@pytest.mark.parametrize("rows,N,split,nt", KS_CASES)
def test_ks_integer_known_answer_bit_for_bit(rows, N, split, nt):
    """A in {+-1, +-2}, B in {-2..2}: every product and partial sum is an exact fp32 integer, so
    C must be bf16(exact) bit for bit whatever the K ranges and the slab combine do"""
    row, col, _, ival = base_pattern()
    B, ref = int_case(N)
    plan = build(M0, K0, row, col, ival, "block_total", rows, 1, N, over={"KS_SPLIT": split, "KS_NT": nt})
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["dtype"] == 2, info
    # auto (0): min(8, 256 CUs / (row blocks x column tiles)) = 8 K ranges on every case here
    assert info["ksplit"] == (split or 8) and info["ks_nt"] == nt, info
    C = plan.spmm(B)
    torch.cuda.synchronize()
    assert C.dtype == BF
    assert_bits(C, ref, "integer")
    C2 = torch.full((M0, N), float("nan"), device=DEV, dtype=BF)
    plan.spmm(B, C=C2)
    torch.cuda.synchronize()
    assert_bits(C2, ref, "integer relaunch")
    plan.device_status()
    plan.free()


@pytest.mark.parametrize("N", [64, 128])
def test_tall_blocks_at_wide_N_leave_k_mfma_ks_at_both_types(N):
    """the (rows, N) pairs left out above: not on k_mfma_ks at fp16 either; the bf16 plan runs its
    gather family and is still bit-exact"""
    row, col, _, ival = base_pattern()
    B, ref = int_case(N)
    p16 = build(M0, K0, row, col, ival, "block_total", 112, 1, N, dtype="f16")
    assert p16.info()["device_kernel"] != "k_mfma_ks", p16.info()
    p16.free()
    plan = build(M0, K0, row, col, ival, "block_total", 112, 1, N)
    assert plan.info()["device_kernel"] == "k_block_rows", plan.info()
    assert_bits(plan.spmm(B), ref, "integer on the gather family")
    plan.free()


def test_ks_rounding_ladder():
    """all-ones A and B: C[i][:] = bf16-RNE(nnz(row i)).  Above 256 bf16 steps by 2 (by 4 above
    512, 8 above 1024): truncation fails 259, 263 and 511, round-half-away 257, 261 and 513"""
    M, K, N = 96, 2048, 32
    ladder = [255, 256, 257, 258, 259, 261, 263, 511, 513, 1025]
    lens = np.array(ladder + [300 + (37 * i) % 400 for i in range(M - len(ladder))])
    rng = np.random.default_rng(7)
    order = rng.permutation(M)  # the rungs spread over the three row blocks
    lens = lens[order]
    row = np.repeat(np.arange(M, dtype=np.uint64), lens)
    col = np.concatenate([np.sort(rng.choice(K, n, replace=False)) for n in lens]).astype(np.uint64)
    plan = build(M, K, row, col, np.ones(len(row), np.float32), "block_total", 32, 1, N,
                 over={"KS_MIN_ROWS": 32, "MFMA_MAX_FILL": 1 << 30})
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["n_units"] == 3, info
    C = plan.spmm(torch.ones((K, N), device=DEV, dtype=BF))
    torch.cuda.synchronize()
    plan.device_status()
    want = torch.from_numpy(lens.astype(np.float32)).to(BF)
    got = C.float().cpu().numpy()
    rne = {255: 255, 256: 256, 257: 256, 258: 258, 259: 260, 261: 260, 263: 264, 511: 512, 513: 512, 1025: 1024}
    for n, r in rne.items():
        i = int(np.nonzero(lens == n)[0][0])
        assert want[i].item() == r
        assert (got[i] == r).all(), (n, r, got[i][:4])
    assert_bits(C, want[:, None].expand(M, N).contiguous().to(DEV), "ladder")
    plan.free()


@pytest.mark.parametrize("N", [8, 32, 128])
def test_ks_random_parity(N):
    row, col, val, _ = base_pattern()
    B = round_bf16(np.random.default_rng(N).standard_normal((K0, N)))
    ref = ofi.spmm_ref(M0, N, row, col, round_bf16(val), B, "f64")
    plan = build(M0, K0, row, col, val, "block_total", 40, 1, N)
    assert plan.info()["device_kernel"] == "k_mfma_ks", plan.info()
    C = plan.spmm(torch.from_numpy(B).to(BF).to(DEV))
    torch.cuda.synchronize()
    plan.device_status()
    err = rel_err(C.float().cpu().numpy(), ref)
    print(f"k_mfma_ks bf16 N={N}: max rel err {err:.3g} (bound {TIGHT_BF16})")
    assert err <= TIGHT_BF16, err
    plan.free()


def test_range_past_fp16():
    """why the dtype exists: an A value of 3e5 is finite at bf16 and Inf at fp16"""
    N = 32
    row, col, val, _ = base_pattern()
    val = val.copy()
    e = len(row) // 2
    r0, c0 = int(row[e]), int(col[e])
    val[e] = 3.0e5
    B = round_bf16(np.random.default_rng(3).uniform(-1, 1, (K0, N)))
    B[c0, :] = 1.0
    ref = ofi.spmm_ref(M0, N, row, col, round_bf16(val), B, "f64")
    plan = build(M0, K0, row, col, val, "block_total", 40, 1, N)
    assert plan.info()["device_kernel"] == "k_mfma_ks"
    C = plan.spmm(torch.from_numpy(B).to(BF).to(DEV)).float().cpu().numpy()
    assert np.isfinite(C).all() and (C[r0] > 2.9e5).all(), C[r0][:4]
    assert rel_err(C, ref) <= TIGHT_BF16
    plan.free()
    p16 = build(M0, K0, row, col, val, "block_total", 40, 1, N, dtype="f16")
    assert p16.info()["device_kernel"] == "k_mfma_ks"
    C16 = p16.spmm(torch.from_numpy(B).half().to(DEV)).float().cpu().numpy()
    assert np.isposinf(C16[r0]).all(), C16[r0][:4]
    p16.free()


def test_non_finite_B():
    """One Inf and one NaN in B, as tests/test_gpu_spmm.py test_mfma_non_finite_B_deviation does
    for fp16.  On the bf16 gather kernels (MFMA_TILES = 0: the reference's semantics) they reach
    exactly the rows of C with a nonzero in that column of A.  k_mfma_ks multiplies the row
    block's whole dense tile, zeros included (DESIGN.md §3 deviation, the same at fp16): there
    the Inf's output column is non-finite in every row -- Inf where A has the entry, NaN from
    0 x Inf elsewhere -- and every other column stays as the reference has it."""
    N = 32
    row, col, val, _ = base_pattern()
    B = round_bf16(np.random.default_rng(5).uniform(-1, 1, (K0, N)))
    k1, j1, k2, j2 = 77, 3, 1500, 20
    B[k1, j1] = np.inf
    B[k2, j2] = np.nan
    Bt = torch.from_numpy(B).to(BF).to(DEV)
    has1 = np.zeros(M0, bool)
    has1[row[col == k1].astype(np.int64)] = True
    has2 = np.zeros(M0, bool)
    has2[row[col == k2].astype(np.int64)] = True
    assert has1.any() and not has1.all() and has2.any() and not has2.all()
    plan = build(M0, K0, row, col, val, "block_total", 40, 1, N, over={"MFMA_TILES": 0})
    assert plan.info()["device_kernel"] == "k_block_rows", plan.info()
    C = plan.spmm(Bt).float().cpu().numpy()
    np.testing.assert_array_equal(np.isinf(C[:, j1]), has1)
    np.testing.assert_array_equal(np.isfinite(C[:, j1]), ~has1)
    np.testing.assert_array_equal(np.isnan(C[:, j2]), has2)
    assert np.isfinite(np.delete(C, [j1, j2], axis=1)).all()
    plan.free()
    plan = build(M0, K0, row, col, val, "block_total", 40, 1, N)
    assert plan.info()["device_kernel"] == "k_mfma_ks", plan.info()
    C = plan.spmm(Bt).float().cpu().numpy()
    np.testing.assert_array_equal(np.isinf(C[:, j1]), has1)
    assert np.isnan(C[~has1, j1]).all() and np.isnan(C[:, j2]).all()
    assert np.isfinite(np.delete(C, [j1, j2], axis=1)).all()
    plan.free()


def test_grouped_launch_never_mixes_types():
    """bf16 and fp16 plans of one shape and instantiation: grouped per type only"""
    N = 32
    row, col, val, _ = base_pattern()
    plans = [build(M0, K0, row, col, val, "block_total", 80, 1, N, dtype=d) for d in ("bf16", "bf16", "f16", "f16")]
    for p in plans:
        assert p.info()["device_kernel"] == "k_mfma_ks", p.info()
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    Bf = [torch.rand((K0, N), device=DEV, generator=g) * 2 - 1 for _ in plans]
    Bs = [b.to(BF if p.info()["dtype"] == 2 else torch.float16) for b, p in zip(Bf, plans)]
    singles = [p.spmm(b) for p, b in zip(plans, Bs)]
    torch.cuda.synchronize()
    for order, launches in (([0, 1, 2, 3], [2, 2]), ([0, 2, 1, 3], [1, 1, 1, 1])):
        Cs = [torch.full((M0, N), float("nan"), device=DEV, dtype=Bs[i].dtype) for i in order]
        bat = gsa.Batch([(plans[i], 0, Bs[i], c) for i, c in zip(order, Cs)], N)
        assert bat.launches() == launches, bat.launches()
        bat.run(torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        for i, c in zip(order, Cs):
            assert torch.equal(c.view(torch.int16), singles[i].view(torch.int16)), (order, i)
    for p in plans:
        p.device_status()
        p.free()


# ------------------------------------------------------------------ every gather family
# the parameters tests/test_gpu_spmm.py and tests/test_gpu_nm.py use for each pipeline
PIPE_PARAMS = {"thread_total": (4, 1), "warp_total": (0, 1), "block_total": (20, 1), "thread_bit_map": (4, 1),
               "warp_segment": (4, 1), "tblock_warp_total": (4, 1), "balanced_warp_total": (256, 1),
               "warp_bit_map": (4, 1), "tblock_bit_map": (4, 1), "col_direction_nm": (32, 1)}


@functools.lru_cache(maxsize=None)
def gather_matrices():
    """300 x 400 random with 10% empty rows (rows long enough for the col-direction padding rule);
    ragged: one 1500-entry row, 70-entry rows and single entries (no trailing empty rows: the
    balanced splitters refuse those)"""
    out = [("random", 300, 400) + tuple(ds.random_rows(300, 400, 40.0, seed=21, empty_frac=0.1))]
    rows = np.concatenate([np.zeros(1500, np.uint64), np.repeat(np.arange(1, 40, dtype=np.uint64), 70),
                           np.arange(40, 60, dtype=np.uint64)])
    cols = np.concatenate([np.arange(1500, dtype=np.uint64), np.tile(np.arange(70, dtype=np.uint64) * 7, 39),
                           np.arange(40, 60, dtype=np.uint64)])
    out.append(("ragged", 60, 1500, rows, cols, np.linspace(-1, 1, len(rows)).astype(np.float32)))
    return out


@functools.lru_cache(maxsize=None)
def gather_reference(case, N):
    """(B rounded to bf16, fp64 oracle on the rounded operands), once per (matrix, N)"""
    name, M, K, row, col, val = gather_matrices()[case]
    B = round_bf16(np.random.default_rng(40 + N).uniform(-1, 1, (K, N)))
    ref = ofi.spmm_ref(M, N, row, col, round_bf16(val), B, "f64")
    B.setflags(write=False)
    ref.setflags(write=False)
    return B, ref


def test_pipeline_table_covers_the_product():
    assert set(PIPE_PARAMS) == set(gsa.PIPELINES)


@pytest.mark.parametrize("N", [8, 13, 32])
@pytest.mark.parametrize("pipeline", sorted(PIPE_PARAMS))
def test_every_gather_family_at_bf16(pipeline, N):
    p0, p1 = PIPE_PARAMS[pipeline]
    for case, (name, M, K, row, col, val) in enumerate(gather_matrices()):
        B, ref = gather_reference(case, N)
        p32 = build(M, K, row, col, val, pipeline, p0, p1, N, dtype="f32")
        family = p32.info()["device_kernel"]
        p32.free()
        plan = build(M, K, row, col, val, pipeline, p0, p1, N)
        info = plan.info()
        assert info["dtype"] == 2 and info["device_kernel"] == family, (name, family, info)
        C = plan.spmm(torch.from_numpy(B.copy()).to(BF).to(DEV))
        torch.cuda.synchronize()
        assert C.dtype == BF
        err = rel_err(C.float().cpu().numpy(), ref)
        print(f"{pipeline} {name} N={N}: {family} max rel err {err:.3g} (bound {TIGHT_BF16})")
        assert err <= TIGHT_BF16, (name, family, err)
        plan.free()


def test_bf16_refuses_16_bit_atomic_launches():
    """warp_segment built for N = 32 keeps its fp32 workspace at that width; fp16 falls back to
    16-bit atomic adds into C at another N, bf16 refuses the launch and says what to do"""
    name, M, K, row, col, val = gather_matrices()[0]
    plan = build(M, K, row, col, val, "warp_segment", 4, 1, 32)
    assert plan.info()["device_kernel"].startswith("k_bitmap_segment"), plan.info()
    C = torch.full((M, 8), 7.0, device=DEV, dtype=BF)
    with pytest.raises(gsa.GsError) as ex:
        plan.spmm(torch.ones((K, 8), device=DEV, dtype=BF), C=C)
    assert ex.value.code == -1
    assert "16-bit atomic" in str(ex.value) and "re-run the pipeline" in str(ex.value), str(ex.value)
    torch.cuda.synchronize()
    assert (C == 7.0).all()  # nothing was launched
    B, ref = gather_reference(0, 32)
    assert rel_err(plan.spmm(torch.from_numpy(B.copy()).to(BF).to(DEV)).float().cpu().numpy(), ref) <= TIGHT_BF16
    plan.free()


def test_two_four_falls_back_to_the_gather_family():
    """k_nm_mfma is an fp16 kernel: the bf16 plan of a 2:4 matrix runs k_row_chunks"""
    M, K, N = 256, 512, 32
    row, col, val = ds.two_four(M, K, 30)
    B = round_bf16(np.random.default_rng(9).uniform(-1, 1, (K, N)))
    plan = build(M, K, row, col, val, "col_direction_nm", 32, 1, N)
    assert plan.info()["device_kernel"].startswith("k_row_chunks"), plan.info()  # (+ the plan's level)
    ref = ofi.spmm_ref(M, N, row, col, round_bf16(val), B, "f64")
    assert rel_err(plan.spmm(torch.from_numpy(B).to(BF).to(DEV)).float().cpu().numpy(), ref) <= TIGHT_BF16
    plan.free()
    p16 = build(M, K, row, col, val, "col_direction_nm", 32, 1, N, dtype="f16")
    assert p16.info()["device_kernel"] == "k_nm_mfma", p16.info()
    p16.free()


def test_operands_are_checked_per_dtype():
    M, K, N = 300, 200, 16
    row, col, val = ds.random_rows(M, K, 12.0, seed=5)
    pb = build(M, K, row, col, val, "block_total", 40, 1, N)
    ph = build(M, K, row, col, val, "block_total", 40, 1, N, dtype="f16")
    Bb = torch.rand((K, N), device=DEV, dtype=BF)
    Bh = Bb.half()
    with pytest.raises(TypeError):
        pb.spmm(Bh)
    with pytest.raises(TypeError):
        ph.spmm(Bb)
    for bad in (torch.zeros((M - 1, N), device=DEV, dtype=BF), torch.zeros((M, N + 8), device=DEV, dtype=BF),
                torch.zeros((M, N), device=DEV, dtype=torch.float16)):
        with pytest.raises(ValueError):
            pb.spmm(Bb, C=bad)
        with pytest.raises(ValueError):
            pb.rotation([Bb], [bad])
        with pytest.raises(ValueError):
            gsa.Batch([(pb, 0, Bb, bad)], N)
        assert not bad.any()
    good = torch.empty((M, N), device=DEV, dtype=BF)
    ref = pb.spmm(Bb)
    pb.rotation([Bb], [good]).run(2, 0)
    torch.cuda.synchronize()
    assert torch.equal(good.view(torch.int16), ref.view(torch.int16))
    pb.free()
    ph.free()
