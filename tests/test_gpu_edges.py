"""Edge sweeps of every kernel family on guarded operands (tests/guarded.py): column tiles past the
first, the narrowest widths, K edges of k_mfma_ks's peeled fast iterations, and what a kernel
touches outside B and C.

Inputs are small integers (A in {-2, -1, 1, 2}, B in {-2 .. 2}, at most 256 nonzeros per row), so
every partial sum is an exact integer of at most 1024 at fp32, at fp16 (k_bitmap_segment's fp16
atomics) and under the K-split slab tag: C must equal the exact product rounded once to the plan
dtype, bit for bit, whatever the summation order.  The reference is a float64 dense product
(NumPy, exact), cast once.  Every launch runs on guarded_B / guarded_C and is followed by three
checks: bit-exact, both operands' guard bands intact, and a second launch into the NaN-refilled
payload giving the same bits.

C1 gather side (MFMA_TILES = 0): every pipeline of tests/test_gpu_spmm.py's PIPES + COL_PIPES at
   fp32 and fp16, tests/test_gpu_bf16.py's PIPE_PARAMS at bf16, on the edge pattern below (its
   long-row variant for the col-direction pipelines, which refuse the short rows: REFUSALS).
   k_lds_rows takes none of those widths (it needs a power-of-two count of 16-byte pieces per B
   row); it runs on tblock_warp_total(20,2) at N = 4 .. 64.
The matrix-core kernels (C2 .. C4) are in tests/test_gpu_edges_mfma.py, the non-finite-B sweep of
the gather families in tests/test_gpu_edges_nonfinite.py."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C, int_values  # noqa: E402
from test_gpu_bf16 import PIPE_PARAMS  # noqa: E402
from test_gpu_spmm import BALANCED, COL_PIPES, PIPES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
EBYTES = {"f32": 4, "f16": 2, "bf16": 2}
MAX_ABS = 1024  # 256 nonzeros x |a| <= 2 x |b| <= 2


# ------------------------------------------------------------------ the edge pattern
EDGE_M, EDGE_K = 131, 203
EDGE_K1, EDGE_I = 150, 9  # row EDGE_I's last stored entry is at column EDGE_K1; row EDGE_I + 1 holds one entry


@functools.lru_cache(maxsize=None)
def edge_pattern(long_rows=False):
    """(row, col, val, row_ptr) of the 131 x 203 edge matrix, row-sorted, columns sorted inside a row:
    - row 0 empty; rows 5, 37, 38 and 90 empty inside; rows 128..130 (three trailing rows) empty;
    - row 20 holds 256 nonzeros: every one of the 203 columns, 53 of them twice (the reference
      accepts repeated coordinates and adds them);
    - rows 10..13 hold exactly 1, 7, 8 and 9 nonzeros and row 10 starts 5 entries past a multiple
      of 8, so the 4- and 8-entry aligned chunks of the wave families cross the row boundaries;
    - row 9's last entry is at column EDGE_K1, row 10's one entry elsewhere (non-finite-B tests);
    - rows 1 and 20 hold columns 0 and K - 1; row 127, the last non-empty row, ends at column K - 1
      with the very last stored nonzero;
    - the other rows hold 2..20 nonzeros.
    long_rows: the same with 17..60 nonzeros in the other rows and 1, 63, 64 and 65 in rows 10..13
    (one short of, exactly and one past a 64-entry BMT), for the col-direction pipelines: they pad
    every row to a multiple of 64 entries and refuse a pattern that grows fourfold by it"""
    M, K = EDGE_M, EDGE_K
    rng = np.random.default_rng(2025 if long_rows else 2024)
    lens = rng.integers(17, 61, M) if long_rows else rng.integers(2, 21, M)
    lens[[0, 5, 37, 38, 90, 128, 129, 130]] = 0
    lens[10:14] = [1, 63, 64, 65] if long_rows else [1, 7, 8, 9]
    lens[20] = 256
    lens[8] += (5 - int(lens[:10].sum())) % 8
    rows, cols = [], []
    for r in range(M):
        n = int(lens[r])
        if r == 20:
            c = np.sort(np.concatenate([np.arange(K), rng.choice(K, n - K, replace=False)]))
        elif r == EDGE_I:
            c = np.concatenate([np.sort(rng.choice(np.arange(1, EDGE_K1), n - 1, replace=False)), [EDGE_K1]])
        elif r == EDGE_I + 1:
            c = np.array([7])
        elif r in (1, 127):
            c = np.sort(rng.choice(np.arange(1, K - 1), n - 1, replace=False))
            c = np.concatenate([[0] if r == 1 else [], c[1:] if r == 1 else c, [K - 1]])
        else:
            c = np.sort(rng.choice(K, n, replace=False))
        assert len(c) == n
        rows.append(np.full(n, r))
        cols.append(c)
    row = np.concatenate(rows).astype(np.uint64)
    col = np.concatenate(cols).astype(np.uint64)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert row_ptr[EDGE_I + 1] % 8 == 5 and col[row_ptr[EDGE_I + 1] - 1] == EDGE_K1
    assert int(row[-1]) == 127 and int(col[-1]) == K - 1 and lens.max() == 256
    val = int_values(len(row), 78 if long_rows else 77)
    for a in (row, col, val, row_ptr):
        a.setflags(write=False)
    return row, col, val, row_ptr


def dense_f64(M, K, row, col, val):
    A = np.zeros((M, K), np.float64)
    np.add.at(A, (row.astype(np.int64), col.astype(np.int64)), val.astype(np.float64))  # repeated coordinates add
    return A


@functools.lru_cache(maxsize=None)
def edge_dense(long_rows=False):
    row, col, val, _ = edge_pattern(long_rows)
    return dense_f64(EDGE_M, EDGE_K, row, col, val)


@functools.lru_cache(maxsize=None)
def int_B_cpu(K, N, dtype, seed=0):
    g = torch.Generator()
    g.manual_seed(1000 * seed + 7 * K + N)
    return torch.randint(-2, 3, (K, N), generator=g).to(TORCH_DT[dtype])


def exact_ref(A, B_cpu, dtype):
    """dtype(A @ B) from the float64 product (integers: exact), rounded once; |.| <= 1024 asserted first"""
    ref = A @ B_cpu.double().numpy()
    assert np.abs(ref).max() <= MAX_ABS, np.abs(ref).max()
    return torch.from_numpy(ref).to(TORCH_DT[dtype])


@functools.lru_cache(maxsize=None)
def edge_case(N, dtype, long_rows=False):
    """(B, reference) of the edge pattern on the CPU, once per width and dtype; never written"""
    B = int_B_cpu(EDGE_K, N, dtype)
    return B, exact_ref(edge_dense(long_rows), B, dtype)


def build(M, K, row, col, val, pipeline, p0, p1, N, dtype, over=None):
    over = over or {}
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline(pipeline, N, p0, p1).compile().upload(dtype, 0)
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def kernel_of(plan):
    """device_kernel, or k_lds_rows where the LDS-staged kernel takes the launches at the plan's N
    (lds_stage 1: device_kernel keeps the plan's family name there)"""
    info = plan.info()
    return "k_lds_rows" if info["lds_stage"] == 1 else info["device_kernel"]


def run_guarded(plan, B_cpu, ref_cpu, what, replica=0):
    """one guarded launch and its three checks"""
    M, N = ref_cpu.shape
    B, hb = guarded_B(B_cpu, DEV)
    C, hc = guarded_C(M, N, ref_cpu.dtype, DEV)
    ref = ref_cpu.to(DEV)
    for again in ("", " relaunch"):
        plan.spmm(B, C=C, replica=replica)
        torch.cuda.synchronize()
        plan.device_status()
        assert_bits(C, ref, what + again)
        assert_guards_intact(hc, what + again + " C")
        assert_guards_intact(hb, what + again + " B")
        hc.refill()


# ------------------------------------------------------------------ C1: the gather side
C1_N = [1, 2, 5, 12, 24, 67, 130, 260, 520]
BF16_N = [5, 67, 520]
C1_PIPES = PIPES + COL_PIPES
MANY_TILES = {  # the column tiles the launch makes (N, element bytes): gather_layout.hpp lanes_per_row
    (67, 2): 2, (67, 4): 2, (130, 2): 3, (130, 4): 3, (260, 2): 5, (260, 4): 2, (520, 2): 2, (520, 4): 3,
    (1, 2): 1, (2, 2): 1, (5, 2): 1, (12, 2): 1, (24, 2): 1, (1, 4): 1, (2, 4): 1, (5, 4): 1, (12, 4): 1, (24, 4): 1}
# Refusals (GsError): these and no other.  The col-direction
# pipelines pad every row to a multiple of 64 entries and refuse a pattern that grows fourfold or
# more by it (PADDING_RATE_UP_BOUND): the edge pattern with its 2..20-entry rows, at every width
# and dtype.  They run on its long-row variant instead.  (pipeline) -> a word the message holds
COL_NAMES = tuple(p[0] for p in COL_PIPES)
REFUSALS = {name: "col-direction" for name in COL_NAMES}
FAMILIES = ("k_thread_total", "k_warp_rows", "k_block_rows", "k_bitmap_segment", "k_row_chunks", "k_merge_path")


def pow2ceil(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def column_tiles(N, ebytes):
    """(tiles, lanes per row X, columns per lane CF) of a gather-family launch: 16-byte pieces of a
    B row when N allows (else single elements), X = the pieces rounded up to a power of two, at most
    one wave; tiles = ceil(N / (X * CF))"""
    cfv = 16 // ebytes
    cf = cfv if N % cfv == 0 else 1
    X = min(64, pow2ceil((N + cf - 1) // cf))
    return (N + X * cf - 1) // (X * cf), X, cf


def test_column_tile_rule():
    for (N, eb), t in MANY_TILES.items():
        assert column_tiles(N, eb)[0] == t, (N, eb)
    assert column_tiles(260, 4) == (2, 64, 4)  # the second tile holds one 16-byte piece
    for N, eb in ((12, 4), (24, 2)):           # vector path, 3 pieces on 4 lanes: one idle lane
        tiles, X, cf = column_tiles(N, eb)
        assert tiles == 1 and cf > 1 and N // cf < X
    assert column_tiles(24, 4) == (1, 8, 4) and column_tiles(12, 2) == (1, 16, 1)


def edge_matrix(pipeline):
    """(M, K, row, col, val, long_rows) a pipeline runs on: the edge pattern; its long-row variant
    for the col-direction pipelines (REFUSALS); the balanced splitters refuse trailing empty rows
    (as the reference's assert), so they get the same entries as a 128-row matrix"""
    long_rows = pipeline in COL_NAMES
    row, col, val, _ = edge_pattern(long_rows)
    return (128 if pipeline in BALANCED else EDGE_M), EDGE_K, row, col, val, long_rows


_SWEEPS = {}


def gather_sweep(pipe, dtype):
    """every width of one pipeline and dtype on guarded operands; [(N, device_kernel, column tiles)].
    A GsError is a failure: the patterns are chosen so that nothing is refused.  Run once per
    (pipeline, dtype): a sweep that failed is not launched again, its error is raised again"""
    if (pipe, dtype) not in _SWEEPS:
        try:
            _SWEEPS[pipe, dtype] = _gather_sweep(pipe, dtype)
        except Exception as e:  # noqa: BLE001  (kept, to be raised for every test that shares the sweep)
            _SWEEPS[pipe, dtype] = e
    if isinstance(_SWEEPS[pipe, dtype], Exception):
        raise _SWEEPS[pipe, dtype]
    return _SWEEPS[pipe, dtype]


def _gather_sweep(pipe, dtype):
    name, p0, p1 = pipe
    M, K, row, col, val, long_rows = edge_matrix(name)
    seen = []
    old = gsa.get_config("MFMA_TILES")
    gsa.set_config("MFMA_TILES", 0)
    try:
        for N in (BF16_N if dtype == "bf16" else C1_N):
            B, ref = edge_case(N, dtype, long_rows)
            what = f"{name}({p0},{p1}) {dtype} N={N}"
            plan = build(M, K, row, col, val, name, p0, p1, N, dtype)
            try:
                kernel = kernel_of(plan)
                run_guarded(plan, B, ref[:M], what + " " + kernel)
            finally:
                plan.free()
            assert not kernel.startswith(("k_mfma", "k_nm")), (what, kernel)
            seen.append((N, kernel, column_tiles(N, EBYTES[dtype])[0]))
    finally:
        gsa.set_config("MFMA_TILES", old)
    print(f"{name}({p0},{p1}) {dtype}: " + ", ".join(f"N={n} {k} x{t}" for n, k, t in seen))
    return tuple(seen)


@pytest.mark.parametrize("name", COL_NAMES)
def test_refusals_are_the_tabled_ones(name):
    """the short-row edge pattern on a col-direction pipeline: refused when the pipeline runs,
    whatever the width, by a message that names the family"""
    row, col, val, _ = edge_pattern()
    for dtype, N in [(d, n) for d in ("f32", "f16", "bf16") for n in (1, 12, 67, 520)]:
        with pytest.raises(gsa.GsError) as ex:
            build(EDGE_M, EDGE_K, row, col, val, name, 4, 1, N, dtype, over={"MFMA_TILES": 0}).free()
        assert ex.value.code == -1 and REFUSALS[name] in str(ex.value), str(ex.value)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("pipe", C1_PIPES, ids=lambda p: f"{p[0]}-{p[1]}")
def test_gather_edge_widths(pipe, dtype):
    assert [n for n, _, _ in gather_sweep(pipe, dtype)] == C1_N


@pytest.mark.parametrize("pipeline", sorted(PIPE_PARAMS))
def test_gather_edge_widths_bf16(pipeline):
    assert [n for n, _, _ in gather_sweep((pipeline,) + PIPE_PARAMS[pipeline], "bf16")] == BF16_N


def test_every_gather_family_ran_past_its_first_column_tile():
    """every family kernel of gather_launch.hip's switch at a width of more than one column tile;
    k_merge_path there is the unfused route (the launch fuses the fix-up only at one tile)"""
    many = {}
    for dtype in ("f32", "f16"):
        for pipe in C1_PIPES:
            for N, kernel, tiles in gather_sweep(pipe, dtype):
                if tiles > 1:
                    for f in FAMILIES:
                        if kernel.startswith(f):
                            many.setdefault(f, set()).add((N, dtype))
    print({f: sorted(v) for f, v in many.items()})
    for f in FAMILIES:
        assert many.get(f), (f, many)


# ------------------------------------------------------------------ the LDS-staged kernel
LDS_PIPE = ("tblock_warp_total", 20, 2)  # BMTBs of 20 rows, BMWs of 2: k_lds_rows (tests/test_gpu_spmm.py LDS_PIPES)


@pytest.mark.parametrize("dtype,N", [("f32", 4), ("f32", 8), ("f32", 32), ("f16", 8), ("f16", 32), ("f16", 64)])
def test_lds_rows_guarded(dtype, N):
    """k_lds_rows on the edge pattern: one, two, eight 16-byte pieces per B row"""
    name, p0, p1 = LDS_PIPE
    row, col, val, _ = edge_pattern()
    B, ref = edge_case(N, dtype)
    plan = build(EDGE_M, EDGE_K, row, col, val, name, p0, p1, N, dtype, over={"MFMA_TILES": 0})
    try:
        info = plan.info()
        assert info["lds_stage"] == 1 and info["lds_n"] == N, info
        run_guarded(plan, B, ref, f"k_lds_rows {dtype} N={N}")
    finally:
        plan.free()
