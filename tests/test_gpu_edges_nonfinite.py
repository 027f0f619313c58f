"""A non-finite element of B on the gather families (MFMA_TILES = 0), on the edge patterns of
tests/test_gpu_edges.py and guarded operands.

The reference's contract: with B[k, j] = +Inf, C[i, j] is non-finite exactly in the rows i that
hold column k, +-Inf by the sign of A[i, k], and every other element is the exact product with
that B element taken as 0, bit for bit (small integers: tests/test_gpu_edges.py).

k_bitmap_segment, k_merge_path, k_block_rows and k_warp_rows meet it: wave_row and the grouped passes
mask an entry outside its row (the aligned over-read of 16-byte chunks, a padding chunk) in its B
piece as well as in its value.  Four kernels still multiply entries of value 0 with the B row of
their column, and 0 x Inf = NaN ("Non-finite B on the gather families").
What is asserted of them is the containment that text describes:
- no element outside column j differs from the contract by a bit;
- a row outside the documented set meets the contract in column j too (+-Inf where it holds
  column k, the exact value elsewhere);
- a row inside the documented set meets the contract or is NaN; nothing else.
The documented set is computed here from row_ptr, the columns and the chunk width, per kernel:
- k_warp_rows_mc (fp32 plans with 16-bit columns at N a multiple of 4 whose BMWs hold several
  rows; it masks the value only, the B-piece selects cost C1 3.9%): rows whose aligned window of
  4-entry chunks covers an entry of column k that is not theirs, the zero padding after the last
  stored entry counting as column 0; for k = 0 any row (a slot's chunks past its row's end are
  (column 0, value 0) chunks);
- k_thread_total and k_row_chunks (rows padded with their last column at value 0): rows whose last
  column is k -- they hold it, and give NaN where the contract says Inf;
- k_lds_rows (tblock_warp_total(20,2) at N = 8; in every column chunk of KC columns a row's entries
  are padded to a multiple of 4 with the row's last column of that chunk at value 0): rows whose
  entry count in k's chunk is no multiple of 4 and whose last column there is k -- again rows that
  hold it."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_guards_intact, guarded_B, guarded_C  # noqa: E402
from test_gpu_edges import (C1_PIPES, DEV, EBYTES, EDGE_I, EDGE_K1, EDGE_M, LDS_PIPE, TORCH_DT, build,  # noqa: E402
                            edge_case, edge_dense, edge_matrix, edge_pattern, exact_ref, kernel_of)

pytestmark = pytest.mark.gpu
STRICT = ("k_bitmap_segment", "k_merge_path", "k_block_rows", "k_warp_rows")  # (k_warp_rows_mc: multi_chunk below)
LAST_COLUMN = ("k_thread_total", "k_row_chunks")
INF_AT = ((EDGE_K1, 3), (0, 5))  # (k1, j1): row EDGE_I ends at k1 and row EDGE_I + 1's chunk covers it; (k0 = 0, j0)


def one_row_bmws(pipe):
    """pipelines whose BMWs hold one row each: k_warp_rows takes no grouped passes on their plans"""
    return pipe[0] == "warp_total" or (pipe[0] == "tblock_warp_total" and pipe[2] == 1)


@functools.lru_cache(maxsize=None)
def window_rows(long_rows, k, scf):
    """rows whose window [row start rounded down to scf, row end rounded up to scf) of the stored
    entries covers an entry of column k outside the row; past the last entry the arrays hold
    (column 0, value 0).  A row whose start is aligned and that is empty has no window"""
    _, col, _, rp = edge_pattern(long_rows)
    colp = np.concatenate([col.astype(np.int64), np.zeros(scf, np.int64)])
    out = set()
    for i in range(EDGE_M):
        b, e = int(rp[i]), int(rp[i + 1])
        a = b - b % scf
        if a >= e:
            continue
        hi = (e + scf - 1) // scf * scf
        if any(colp[p] == k for p in range(a, hi) if not b <= p < e):
            out.add(i)
    return frozenset(out)


def lds_padded_rows(long_rows, k, KC):
    """rows that k_lds_rows pads in k's column chunk with column k itself"""
    _, col, _, rp = edge_pattern(long_rows)
    out = set()
    for i in range(EDGE_M):
        c = col[rp[i]:rp[i + 1]].astype(np.int64)
        c = c[c // KC == k // KC]
        if len(c) % 4 and int(c.max()) == k:
            out.add(i)
    return frozenset(out)


def documented_rows(kernel, pipe, dtype, long_rows, k, N, col_bytes, KC):
    # device_kernel says k_warp_rows for k_warp_rows_mc too: the launch's own rule (gather_launch.hip)
    multi_chunk = (kernel.startswith("k_warp_rows") and dtype == "f32" and N % 4 == 0 and col_bytes == 2
                   and not one_row_bmws(pipe))
    if multi_chunk:
        return frozenset(range(EDGE_M)) if k == 0 else window_rows(long_rows, k, 16 // EBYTES[dtype])
    if kernel.startswith(STRICT):
        return frozenset()
    if kernel == "k_lds_rows":
        return lds_padded_rows(long_rows, k, KC)
    assert kernel.startswith(LAST_COLUMN), f"{kernel}: no rule for this kernel's zero-valued entries yet"
    _, col, _, rp = edge_pattern(long_rows)
    return frozenset(i for i in range(EDGE_M) if rp[i + 1] > rp[i] and int(col[rp[i + 1] - 1]) == k)


@functools.lru_cache(maxsize=None)
def contract(N, dtype, long_rows, k, j):
    """(B with +Inf at [k, j], the result with that element taken as 0, the rows holding column k,
    what the contract puts in column j of those rows)"""
    row, col, val, _ = edge_pattern(long_rows)
    B0, _ = edge_case(N, dtype, long_rows)
    Bz, Bi = B0.clone(), B0.clone()
    Bz[k, j] = 0
    Bi[k, j] = float("inf")
    ref0 = exact_ref(edge_dense(long_rows), Bz, dtype)
    sel = col.astype(np.int64) == k
    r64 = row.astype(np.int64)
    pos, neg = np.zeros(EDGE_M, bool), np.zeros(EDGE_M, bool)
    pos[r64[sel & (val > 0)]] = True
    neg[r64[sel & (val < 0)]] = True
    want = np.where(pos & neg, np.nan, np.where(pos, np.inf, -np.inf))  # (a repeated coordinate of both signs: NaN)
    return Bi, ref0, pos | neg, want


def test_the_edge_pattern_sets_the_trap():
    """row EDGE_I ends at column k1, the next row holds one entry elsewhere and its chunk covers
    that entry at either chunk width; some row that does not hold column 0 over-reads one"""
    for long_rows in (False, True):
        row, col, _, rp = edge_pattern(long_rows)
        held = set(row[col == EDGE_K1].astype(int))
        assert EDGE_I in held and EDGE_I + 1 not in held and rp[EDGE_I + 2] - rp[EDGE_I + 1] == 1
        for scf in (4, 8):
            assert EDGE_I + 1 in window_rows(long_rows, EDGE_K1, scf)
            assert window_rows(long_rows, 0, scf) - set(row[col == 0].astype(int))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("pipe", C1_PIPES + [LDS_PIPE], ids=lambda p: f"{p[0]}-{p[1]}")
def test_non_finite_B_stays_contained(pipe, dtype):
    name, p0, p1 = pipe
    M, K, row, col, val, long_rows = edge_matrix(name)
    gsa.set_config("MFMA_TILES", 0)
    try:
        for N in (8, 13):
            plan = build(M, K, row, col, val, name, p0, p1, N, dtype)
            kernel, col_bytes, KC = kernel_of(plan), plan.info()["col_bytes"], plan.info()["lds_kc"]
            if pipe == LDS_PIPE and N == 8:
                assert kernel == "k_lds_rows", plan.info()
            C, hc = guarded_C(M, N, TORCH_DT[dtype], DEV)
            for k, j in INF_AT:
                what = f"{name}({p0},{p1}) {dtype} N={N} {kernel} +Inf at B[{k},{j}]"
                Bi, ref0, holds, want = contract(N, dtype, long_rows, k, j)
                B, hb = guarded_B(Bi, DEV)
                hc.refill()
                plan.spmm(B, C=C)
                torch.cuda.synchronize()
                plan.device_status()
                assert_guards_intact(hc, what + " C")
                assert_guards_intact(hb, what + " B")
                got = C.cpu()
                idt = torch.int16 if EBYTES[dtype] == 2 else torch.int32
                same = (got.view(idt) == ref0[:M].view(idt)).numpy()
                others = np.delete(same, j, axis=1)
                assert others.all(), f"{what}: {int((~others).sum())} elements outside column {j} differ"
                gj = got[:, j].float().numpy()
                meets = np.where(holds[:M], (gj == want[:M]) | (np.isnan(gj) & np.isnan(want[:M])), same[:, j])
                off = set(np.nonzero(~meets)[0].tolist())
                allowed = documented_rows(kernel, pipe, dtype, long_rows, k, N, col_bytes, KC)
                print(f"{what}: rows off the contract {sorted(off)}; documented {len(allowed)}")
                assert off <= allowed, f"{what}: rows {sorted(off - allowed)} are outside the documented set"
                assert np.isnan(gj[sorted(off)]).all(), f"{what}: {gj[sorted(off)]}"
            plan.free()
    finally:
        gsa.set_config("MFMA_TILES", 1)
