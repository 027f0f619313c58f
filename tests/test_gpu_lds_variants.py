"""Every kernel of the LDS-staged gather family on the edge sweeps of tests/test_gpu_edges.py and
tests/test_gpu_edges_nonfinite.py: k_lds_rows at MAXR 1, 2 and 4 (fp16 and fp32, one to eight 16-byte pieces
per B row, and the pair-banks entry order without LDS-DMA), k_lds_rows_dma, and k_lds_rows_rs (one row per
slot, its own LDS-DMA issue, columns as byte offsets), each with one K range, two, and the upload's own split.

All on the 131 x 203 edge pattern with MFMA_TILES = 0 and tblock_warp_total(p0, p1).  Every plan first shows
its route in plan.info(): the kernel, the chunking and the K split of TABLE, the one that
tools/gather_layout_check.cc pins for this size at the upload's LDS budgets ("edge ..." cases).  K = 203 never
goes as one chunk: a chunk is a multiple of 8 columns and build_lds_tiles passes over one wider than K, so
LDS_KSPLIT = 1 is two chunks of 104 columns in one range (no slab combine), 2 the same chunks in two ranges,
0 (automatic) three chunks of 72 in three ranges.  tblock_warp_total(12,1) reaches the one-row-BMW forms
(MAXR = 1) only under LDS_STAGE_ANY: the upload otherwise keeps BMTBs of under 16 rows or one-row BMWs on the
gather kernel.

Per plan:
- run_guarded: the bits of the float64 product rounded once, both guard bands of B and C intact, and a second
  launch into NaN-refilled C with the same bits (the arrival counters of the K split re-arm);
- +Inf at B[k, j] for the two positions of the existing sweep and for k = KC - 1, KC and K - 1: nothing outside
  column j differs by a bit, a row outside the documented set meets the contract in column j, a row inside it
  meets the contract or is NaN.  The documented set is lds_padded_rows (tests/test_gpu_edges_nonfinite.py),
  from the pattern and KC alone, for all three kernels: rows whose entry count in k's chunk is no multiple of
  4 and whose last column there is k (the padding entries, value 0, repeat that column; the parity orders of
  k_lds_rows_dma / _rs and of fp32 N = 32 move them inside the row only).
No tolerance anywhere: integers, exact in every summation order (tests/test_gpu_edges.py)."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402,F401
from guarded import assert_guards_intact, guarded_B, guarded_C  # noqa: E402
from test_gpu_edges import (DEV, EBYTES, EDGE_K, EDGE_K1, EDGE_M, TORCH_DT, build, edge_case, edge_pattern,  # noqa: E402
                            run_guarded)
from test_gpu_edges_nonfinite import INF_AT, contract, lds_padded_rows  # noqa: E402

PIPELINE = "tblock_warp_total"
# LDS_KSPLIT -> (lds_kc, lds_chunks, ksplit): tools/gather_layout_check.cc, the "edge ..." cases
TABLE = {1: (104, 2, 1), 2: (104, 2, 2), 0: (72, 3, 3)}
ROW_PIPES = ((20, 2), (16, 4), (12, 1))            # MAXR 2, 4, 1
SLOT_PIPES = ((40, 5), (48, 6), (64, 8), (16, 8))  # (40,5): the last BMTB holds 11 rows = BMWs of 5, 5 and 1
# (kernel, dtype, N, configs)
VARIANTS = [("k_lds_rows", "f16", 8, {}), ("k_lds_rows", "f16", 32, {}), ("k_lds_rows", "f16", 64, {}),
            ("k_lds_rows", "f32", 4, {}), ("k_lds_rows", "f32", 8, {}),
            ("k_lds_rows", "f32", 32, {"LDS_DMA": 0}),  # the pair-banks entry order without LDS-DMA
            ("k_lds_rows_dma", "f32", 32, {}), ("k_lds_rows_rs", "f32", 32, {})]
CASES = [(v, p) for v in VARIANTS for p in (SLOT_PIPES if v[0] == "k_lds_rows_rs" else ROW_PIPES)]


def case_id(c):
    (kernel, dtype, N, over), (p0, p1) = c
    return f"{kernel}-{dtype}-N{N}{'-nodma' if over else ''}-{p0}x{p1}"


def inf_positions(KC, N):
    """(k, j): the existing sweep's two, then the last column of the first chunk, the first of the second,
    and the last column of B; j inside the narrowest widths too"""
    return tuple((k, j % N) for k, j in INF_AT + ((KC - 1, 2), (KC, 6), (EDGE_K - 1, 1)))


def routed_plans(case):
    """the case's plan at LDS_KSPLIT = 1, 2 and 0, its route asserted against TABLE; the configs go back to
    what they were when a plan is built (test_gpu_edges.build: finally)"""
    (kernel, dtype, N, over), (p0, p1) = case
    row, col, val, _ = edge_pattern()
    for ks, (kc, nc, ranges) in TABLE.items():
        cfg = dict(over, MFMA_TILES=0, LDS_KSPLIT=ks)
        if p1 == 1:
            cfg["LDS_STAGE_ANY"] = 1
        before = {k: gsa.get_config(k) for k in cfg}
        plan = build(EDGE_M, EDGE_K, row, col, val, PIPELINE, p0, p1, N, dtype, over=cfg)
        try:
            assert {k: gsa.get_config(k) for k in cfg} == before
            info = plan.info()
            got = {k: info[k] for k in ("device_kernel", "lds_stage", "lds_n", "lds_kc", "lds_chunks", "ksplit")}
            want = {"device_kernel": kernel, "lds_stage": 1, "lds_n": N, "lds_kc": kc, "lds_chunks": nc, "ksplit": ranges}
            assert got == want, (case_id(case), ks, got)
            yield plan, f"{kernel} {dtype} N={N} ({p0},{p1}) LDS_KSPLIT={ks}: KC {kc} x {nc}, {ranges} K ranges", kc
        finally:
            plan.free()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_exact_and_guarded(case):
    _, dtype, N, _ = case[0]
    B, ref = edge_case(N, dtype)
    for plan, what, _ in routed_plans(case):
        run_guarded(plan, B, ref, what)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_non_finite_B_stays_contained(case):
    _, dtype, N, _ = case[0]
    idt = torch.int16 if EBYTES[dtype] == 2 else torch.int32
    for plan, what0, KC in routed_plans(case):
        C, hc = guarded_C(EDGE_M, N, TORCH_DT[dtype], DEV)
        for k, j in inf_positions(KC, N):
            what = f"{what0} +Inf at B[{k},{j}]"
            Bi, ref0, holds, want = contract(N, dtype, False, k, j)
            B, hb = guarded_B(Bi, DEV)
            hc.refill()
            plan.spmm(B, C=C)
            torch.cuda.synchronize()
            plan.device_status()
            assert_guards_intact(hc, what + " C")
            assert_guards_intact(hb, what + " B")
            got = C.cpu()
            same = (got.view(idt) == ref0.view(idt)).numpy()
            others = np.delete(same, j, axis=1)
            assert others.all(), f"{what}: {int((~others).sum())} elements outside column {j} differ"
            gj = got[:, j].float().numpy()
            meets = np.where(holds, (gj == want) | (np.isnan(gj) & np.isnan(want)), same[:, j])
            off = set(np.nonzero(~meets)[0].tolist())
            allowed = lds_padded_rows(False, k, KC)
            print(f"{what}: rows off the contract (NaN) {sorted(off)}; documented {sorted(allowed)}")
            assert off <= allowed, f"{what}: rows {sorted(off - allowed)} are outside the documented set"
            assert np.isnan(gj[sorted(off)]).all(), f"{what}: {gj[sorted(off)]}"


# ------------------------------------------------------------------ the trap, without a GPU
@functools.lru_cache(maxsize=None)
def stored_order(p0, KC):
    """[(BMTB, chunk)] -> [(row, column)] as build_lds_tiles stores a segment before any parity order: row
    after row, a row's entries of the chunk by column, then copies of its last one up to a multiple of 4"""
    _, col, _, rp = edge_pattern()
    segs = {}
    for r in range(EDGE_M):
        c = col[rp[r]:rp[r + 1]].astype(np.int64)
        for ch in sorted(set((c // KC).tolist())):
            cc = c[c // KC == ch].tolist()
            cc += [cc[-1]] * (-len(cc) % 4)
            segs.setdefault((r // p0, ch), []).extend((r, x) for x in cc)
    return segs


def trapped_rows(p0, KC, k):
    """rows that do not hold column k, outside the documented set, with a stored entry next to one of column k:
    a slot that walks past either end of its row there multiplies B[k, :]"""
    row, col, _, _ = edge_pattern()
    holders = set(row[col == k].astype(int).tolist())
    seg = stored_order(p0, KC).get
    out = set()
    for g in range((EDGE_M + p0 - 1) // p0):
        s = seg((g, k // KC), [])
        for a, b in zip(s, s[1:]):
            for (r, _), (_, x) in ((a, b), (b, a)):
                if x == k and r not in holders:
                    out.add(r)
    return out - lds_padded_rows(False, k, KC)


def test_the_edge_pattern_sets_the_trap():
    """for every pinned chunk width and BMTB height: some tested k has a non-empty documented set, and some
    tested k has a row outside its documented set stored next to an entry of column k"""
    assert (EDGE_K1, 3) in INF_AT
    for KC in sorted({kc for kc, _, _ in TABLE.values()}):
        ks = [k for k, _ in inf_positions(KC, 32)]
        assert KC - 1 in ks and KC in ks and EDGE_K - 1 in ks and KC < EDGE_K
        assert any(lds_padded_rows(False, k, KC) for k in ks), KC
        for p0 in sorted({p[0] for p in ROW_PIPES + SLOT_PIPES}):
            trapped = {k: sorted(trapped_rows(p0, KC, k)) for k in ks}
            print(f"KC {KC}, BMTBs of {p0} rows: documented "
                  f"{ {k: sorted(lds_padded_rows(False, k, KC)) for k in ks} }, rows next to column k {trapped}")
            assert any(trapped.values()), (KC, p0, trapped)
