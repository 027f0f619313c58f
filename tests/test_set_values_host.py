"""CPU checks of the value-source map behind Plan.set_values (gs_plan_value_sources, no device): the map
is the map of exactly the layout upload would build -- gathering another plan's values through it gives
that plan's value array bit for bit -- over every k_mfma_ks layout variant of the default build (u16
positions with and without head steps, K ranges, KS_WPOS), under a row order that is not the identity,
and its refusals; gs_plan_pattern without values."""
import ctypes
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from generalsparse_amd import _lib  # noqa: E402
from test_gpu_edges_mfma import KS_M, ks_pattern, mfma_everywhere  # noqa: E402,F401  (fixture)

NONE = 0xFFFFFFFF
# (K, rows): ks_pattern(K)'s first `rows` rows -- 120: three full 40-row blocks, 131: a short last block.
# The upload gives a plan head steps only where padding them costs at most 6% more groups, which ks_pattern's
# uneven steps never meet: K = 1184 stands for an even pattern of that size (pattern()), which does
# (test_variants_differ asserts that its layout changes with KS_HEAD)
EVEN_K = 1184
SHAPES = [(40, 120), (40, 131), (1176, 120), (1176, 131), (EVEN_K, 120)]
# f16 with and without head steps, window positions and K ranges; bf16 (no KS_WPOS: an fp16 layout)
VARIANTS = [(dt, head, wpos, split) for dt in ("f16", "bf16") for head in (0, 1) for wpos in ((0, 1) if dt == "f16" else (0,))
            for split in (0, 2)]


@functools.lru_cache(maxsize=None)
def pattern(K, M):
    """(row, col) of ks_pattern(K)'s first M rows -- K = EVEN_K: of the even pattern, every third column of a row,
    shifted by the row -- and two sets of random non-integer values"""
    if K == EVEN_K:
        r, c = np.nonzero((np.arange(M)[:, None] + np.arange(K)[None, :]) % 3 == 0)
        row, col = r.astype(np.uint64), c.astype(np.uint64)
    else:
        row, col, _, _ = ks_pattern(K)
        keep = row < M
        row, col = row[keep], col[keep]
    rng = np.random.default_rng(7 * K + M)
    v1 = rng.standard_normal(len(row)).astype(np.float32)
    v2 = (rng.standard_normal(len(row)) * np.exp2(rng.integers(-6, 6, len(row)))).astype(np.float32)
    assert (v1 != np.round(v1)).all() and (v2 != np.round(v2)).all()
    return row, col, v1, v2


def compiled(M, K, row, col, val, over=None, sort=False):
    over = dict(over or {})
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        plan = gsa.Plan.from_coo(M, K, row, col, val)
        if sort:
            plan.add_operator("sort_operator")
        return plan.run_pipeline("block_total", 32, 40, 1).compile()
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def sources(plan, dtype, over):
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        return plan.value_sources(dtype)
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def check_map(A, B, v2, dtype, over, wpos):
    """plan A's map applied to plan B's values is plan B's value array; the maps agree; every entry has its slot"""
    srcA, valsA = sources(A, dtype, over)
    srcB, valsB = sources(B, dtype, over)
    assert srcA.dtype == np.uint32 and valsB.dtype == np.uint16 and len(srcA) == len(valsB) and len(srcA) % 8 == 0
    np.testing.assert_array_equal(srcA, srcB)
    live = srcA != NONE
    assert srcA[live].max() < len(v2)
    w = np.zeros(len(srcA), np.uint16)
    w[live] = gsa.convert_values(v2, dtype)[srcA[live]]
    np.testing.assert_array_equal(w, valsB)
    assert not valsA[~live].any() and not (srcA[-8:] != NONE).any()  # the spare group holds no entry
    count = np.bincount(srcA[live], minlength=len(v2))
    if not wpos:
        np.testing.assert_array_equal(count, np.ones(len(v2), np.int64))
    else:
        # window positions pad a window's last group with copies of that group's first entry (both slots
        # scatter one value to one place), so an entry may be named again -- inside its own group only
        assert (count >= 1).all()
        groups = srcA.reshape(-1, 8)
        first = np.full(len(v2), -1, np.int64)
        g_of = np.repeat(np.arange(len(groups)), 8)[live]
        for e, g in zip(srcA[live], g_of):
            assert first[e] in (-1, g), f"entry {e} in groups {first[e]} and {g}"
            first[e] = g
        assert sum(len(set(g[g != NONE])) for g in groups) == len(v2)


@pytest.mark.parametrize("dtype,head,wpos,split", VARIANTS)
@pytest.mark.parametrize("K,M", SHAPES)
def test_map_equals_layout(K, M, dtype, head, wpos, split, mfma_everywhere):
    row, col, v1, v2 = pattern(K, M)
    over = {"KS_HEAD": head, "KS_WPOS": wpos, "KS_SPLIT": split}
    A, B = compiled(M, K, row, col, v1), compiled(M, K, row, col, v2)
    check_map(A, B, v2, dtype, over, wpos)
    # ... and the plan's own values come back through its own map
    src, vals = sources(A, dtype, over)
    live = src != NONE
    np.testing.assert_array_equal(vals[live], gsa.convert_values(v1, dtype)[src[live]])
    # no device was needed: neither plan is on one
    assert A.info()["replicas"] == 0 and A.info()["value_map_bytes"] == 0 and A.info()["host_values_stale"] == 0
    A.free(), B.free()


def test_variants_differ(mfma_everywhere):
    """the cases above are different layouts: head steps and window positions move the slots, and so do K
    ranges where there are head steps (without them the groups lie back to back in column order either way)"""
    K, M = EVEN_K, 120
    row, col, v1, _ = pattern(K, M)
    A = compiled(M, K, row, col, v1)
    plain = {"KS_HEAD": 0, "KS_WPOS": 0, "KS_SPLIT": 1}
    for a, b in ((plain, dict(plain, KS_HEAD=1)), (plain, dict(plain, KS_WPOS=1)),
                 (dict(plain, KS_HEAD=1), dict(plain, KS_HEAD=1, KS_SPLIT=2))):
        sa, sb = sources(A, "f16", a)[0], sources(A, "f16", b)[0]
        assert len(sa) != len(sb) or (sa != sb).any(), (a, b)
    A.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K", [40, 1176])
def test_row_order(K, dtype, mfma_everywhere):
    """sort_operator ahead of the pipeline: the layout is built from the sorted rows, the pattern keeps the
    original ones"""
    M = KS_M
    row, col, v1, v2 = pattern(K, M)
    A, B = compiled(M, K, row, col, v1, sort=True), compiled(M, K, row, col, v2, sort=True)
    order = A.array("GLOBAL_META_original_nz_row_indices_0")
    assert len(order) == M and (order != np.arange(M)).any(), "the plan's row order is the identity"
    r, c = A.pattern()
    np.testing.assert_array_equal(r, row)
    np.testing.assert_array_equal(c, col)
    check_map(A, B, v2, dtype, {}, 0)
    # the unsorted plan of the same matrix has another map
    U = compiled(M, K, row, col, v1)
    su, sa = U.value_sources(dtype)[0], A.value_sources(dtype)[0]
    assert len(su) != len(sa) or (su != sa).any()
    A.free(), B.free(), U.free()


def test_trailing_empty_rows(mfma_everywhere):
    """a matrix whose last rows hold no entry (the plan then has fewer rows than the matrix) is no padded plan"""
    K, M = 1176, 120
    row, col, v1, v2 = pattern(K, M)
    A, B = compiled(M + 11, K, row, col, v1), compiled(M + 11, K, row, col, v2)
    assert A.info()["rows"] == M + 11
    check_map(A, B, v2, "f16", {}, 0)
    A.free(), B.free()


def test_duplicate_coordinate_refused(mfma_everywhere):
    K, M = 40, 120
    row, col, v1, _ = pattern(K, M)
    i = len(row) // 2
    row2, col2 = np.insert(row, i, row[i]), np.insert(col, i, col[i])
    plan = compiled(M, K, row2, col2, np.insert(v1, i, 0.5))
    with pytest.raises(gsa.GsError, match="twice"):
        plan.value_sources("f16")
    plan.free()


def test_other_refusals(mfma_everywhere):
    K, M = 40, 120
    row, col, v1, _ = pattern(K, M)
    plan = compiled(M, K, row, col, v1)
    with pytest.raises(gsa.GsError, match="f16 and bf16"):
        plan.value_sources("f32")
    plan.free()
    gather = gsa.Plan.from_coo(M, K, row, col, v1).run_pipeline("thread_total", 32, 4, 1).compile()
    with pytest.raises(gsa.GsError, match="k_mfma_ks"):
        gather.value_sources("f16")
    gather.free()
    raw = gsa.Plan.from_coo(M, K, row, col, v1)
    with pytest.raises(gsa.GsError, match="compiled"):
        raw.value_sources("f16")
    # an update needs the plan on a device: refused here, whatever the pointers
    with pytest.raises(gsa.GsError, match="not on the device"):
        _lib.check(raw._L.gs_plan_values_prepare(raw._h))
    x = np.zeros(len(row), np.float32)
    with pytest.raises(gsa.GsError, match="not on the device"):
        _lib.check(raw._L.gs_plan_set_values(raw._h, None, x.ctypes.data_as(_lib.f32p), None))
    with pytest.raises(gsa.GsError, match="neither"):
        _lib.check(raw._L.gs_plan_set_values(raw._h, None, None, None))
    raw.free()


def test_pattern_without_values(mfma_everywhere):
    K, M = 1176, 131
    row, col, v1, _ = pattern(K, M)
    plan = compiled(M, K, row, col, v1, sort=True)
    n = ctypes.c_uint64(0)
    L = plan._L
    _lib.check(L.gs_plan_pattern(plan._h, None, None, None, 0, ctypes.byref(n)))
    assert n.value == len(row)
    full = [np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64), np.zeros(n.value, np.float32)]
    _lib.check(L.gs_plan_pattern(plan._h, full[0].ctypes.data_as(_lib.u64p), full[1].ctypes.data_as(_lib.u64p),
                                 full[2].ctypes.data_as(_lib.f32p), n.value, ctypes.byref(n)))
    r, c = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
    _lib.check(L.gs_plan_pattern(plan._h, r.ctypes.data_as(_lib.u64p), c.ctypes.data_as(_lib.u64p), None, n.value,
                                 ctypes.byref(n)))
    np.testing.assert_array_equal(r, full[0])
    np.testing.assert_array_equal(c, full[1])
    np.testing.assert_array_equal(full[2], v1)
    pr, pc = plan.pattern()
    np.testing.assert_array_equal(pr, row)
    np.testing.assert_array_equal(pc, col)
    np.testing.assert_array_equal(plan.values(), v1)
    plan.free()


def test_info_prefix_unchanged():
    """the two new gs_plan_info fields are appended: every older field keeps its offset"""
    names = [f[0] for f in _lib.GsPlanInfo._fields_]
    assert names[-2:] == ["host_values_stale", "value_map_bytes"] and names[-3] == "weights"
    assert _lib.GsPlanInfo.host_values_stale.offset == _lib.GsPlanInfo.weights.offset + 4
