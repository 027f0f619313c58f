"""Host-side checks of the backward pass's interface (no GPU): the pattern of a plan in its canonical
order after every kind of pipeline (Plan.pattern / Plan.values, gs_plan_pattern), k_sddmm_tm's geometry,
what Plan.sddmm and SparseLinear(grad=...) refuse before anything touches a device, and the stand-alone
sanitizer program of the pattern builder.  The GPU side is tests/test_gpu_sddmm.py and
tests/test_gpu_linear_backward.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import generalsparse_amd as gsa
from generalsparse_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "generalsparse_amd", "csrc")
ENTRY_POINTS = ("gs_plan_pattern", "gs_sddmm", "gs_plan_sddmm_prepare", "gs_sddmm_geometry")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_are_exported_and_bound(name):
    assert name in _lib.SIGNATURES
    fn = getattr(gsa.load_library(), name)
    args, res = _lib.SIGNATURES[name]
    assert fn.argtypes == args and fn.restype is res is ctypes.c_int
    assert f"int {name}(" in open(os.path.join(ROOT, "include", "generalsparse.h")).read()


def matrix(M=37, K=70, seed=3):
    """row-major COO of a 30% dense matrix with an empty row, a full row and distinct values"""
    rng = np.random.default_rng(seed)
    mask = rng.random((M, K)) < 0.3
    mask[5] = False
    mask[9] = True
    mask[0, 0] = mask[M - 1, K - 1] = True
    r, c = np.nonzero(mask)
    return M, K, r.astype(np.uint64), c.astype(np.uint64), (1 + np.arange(len(r))).astype(np.float32)


# a pipeline of each kind: none, row blocks, one that sorts the rows by length (sort_operator), one whose
# rows are padded and stored interleaved (interlance_storage_operator), one that pads empty rows
PIPELINES = [None, ("block_total", 40, 1), ("thread_total", 4, 1), ("warp_bit_map_interleaved", 4, 1),
             ("empty_pad_warp_total", 0, 1)]


@pytest.mark.parametrize("pipe", PIPELINES, ids=lambda p: p[0] if p else "none")
def test_pattern_is_the_input_after_any_pipeline(pipe):
    M, K, row, col, val = matrix()
    plan = gsa.Plan.from_coo(M, K, row, col, val)
    if pipe is not None:
        plan.run_pipeline(pipe[0], 32, pipe[1], pipe[2]).compile()
        keys = plan.keys()
        if pipe[0] == "thread_total":  # the stored rows are in another order, and padded
            assert any("original_nz_row_indices" in k for k in keys) and plan.info()["nnz_stored"] > len(row)
        if pipe[0] == "warp_bit_map_interleaved":
            assert any("after_interlance_storage" in k for k in keys) and plan.info()["nnz_stored"] > len(row)
        if pipe[0] == "empty_pad_warp_total":  # one stored entry for the empty row
            assert plan.info()["nnz_stored"] == len(row) + 1
    r, c = plan.pattern()
    assert r.dtype == c.dtype == np.uint64
    assert np.array_equal(r, row) and np.array_equal(c, col)
    v = plan.values()
    assert v.dtype == np.float32 and np.array_equal(v, val)
    plan.free()


def test_unsorted_columns_and_duplicates():
    """columns come in any order inside a row: the pattern is by row, then column; the three stored copies
    of (1, 4) stay adjacent and in input order (values 20, 21, 22)"""
    row = np.array([0, 0, 0, 1, 1, 1, 1, 1, 3], np.uint64)
    col = np.array([5, 0, 3, 4, 9, 4, 1, 4, 2], np.uint64)
    val = np.array([10, 11, 12, 20, 30, 21, 40, 22, 50], np.float32)
    for pipe in (None, ("block_total", 2, 1)):
        plan = gsa.Plan.from_coo(4, 10, row, col, val)
        if pipe:
            plan.run_pipeline(pipe[0], 32, pipe[1], pipe[2]).compile()
        r, c = plan.pattern()
        assert r.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 3] and c.tolist() == [0, 3, 5, 1, 4, 4, 4, 9, 2]
        assert plan.values().tolist() == [11, 12, 10, 40, 20, 21, 22, 30, 50]
        plan.free()


def test_cap_zero_counts_and_a_short_buffer_is_refused():
    M, K, row, col, val = matrix()
    plan = gsa.Plan.from_coo(M, K, row, col, val)
    L, n = plan._L, ctypes.c_uint64(0)
    assert L.gs_plan_pattern(plan._h, None, None, None, 0, ctypes.byref(n)) == 0 and n.value == len(row)
    r, c, v = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.full(4, 7, np.float32)
    rc = L.gs_plan_pattern(plan._h, r.ctypes.data_as(_lib.u64p), c.ctypes.data_as(_lib.u64p), v.ctypes.data_as(_lib.f32p), 4,
                           ctypes.byref(n))
    assert rc == -1 and (v == 7).all()
    plan.free()


def test_a_saved_and_loaded_plan(tmp_path):
    """a plan file holds the COO as the pipeline left it: an unpadded one (sorted rows or not) gives the
    pattern back, one with padding entries is refused"""
    M, K, row, col, val = matrix()
    for pipe, ok in ((("block_total", 40, 1), True), (("empty_pad_warp_total", 0, 1), False)):
        path = str(tmp_path / (pipe[0] + ".plan"))
        gsa.Plan.from_coo(M, K, row, col, val).run_pipeline(pipe[0], 32, pipe[1], pipe[2]).compile().save(path)
        plan = gsa.Plan.load(path)
        if ok:
            r, c = plan.pattern()
            assert np.array_equal(r, row) and np.array_equal(c, col) and np.array_equal(plan.values(), val)
        else:
            with pytest.raises(gsa.GsError, match="no pattern"):
                plan.pattern()
        plan.free()


def test_from_dense_pattern_is_np_nonzero():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    w = rng.standard_normal((37, 48)).astype(np.float32)
    w[rng.random(w.shape) < 0.7] = 0.0
    w[11] = 0.0
    layer = gsa.SparseLinear.from_dense(torch.from_numpy(w), upload=False)
    r, c = layer.plan.pattern()
    wr, wc = np.nonzero(w)
    assert np.array_equal(r, wr.astype(np.uint64)) and np.array_equal(c, wc.astype(np.uint64))
    assert np.array_equal(layer.plan.values(), w[wr, wc])
    layer.plan.free()


def test_geometry():
    rb, cs, tc = gsa.sddmm_geometry()
    assert rb > 0 and cs > 0 and tc > 0 and rb % 16 == 0 and cs % 16 == 0 and tc % 32 == 0
    assert gsa.load_library().gs_sddmm_geometry(None, None, None) == -1


def compiled_plan():
    M, K, row, col, val = matrix()
    return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", 40, 1, 1).compile(), len(row)


def test_sddmm_refusals_without_a_gpu():
    """every refusal comes before the library touches a device: there is none here"""
    torch = pytest.importorskip("torch")
    plan, nnz = compiled_plan()
    g, x = torch.zeros(8, 37, dtype=torch.float16), torch.zeros(8, 70, dtype=torch.float16)
    out = torch.full((nnz,), 7.0)
    with pytest.raises(ValueError, match="columns"):
        plan.sddmm(torch.zeros(8, 36, dtype=torch.float16), x, out)          # g is not (n, M)
    with pytest.raises(ValueError, match="columns"):
        plan.sddmm(g, torch.zeros(8, 71, dtype=torch.float16), out)          # x is not (n, K)
    with pytest.raises(ValueError, match="tokens"):
        plan.sddmm(g, torch.zeros(9, 70, dtype=torch.float16), out)          # token counts differ
    with pytest.raises(ValueError, match="tokens"):
        plan.sddmm(g[:0], x[:0], out)                                          # no token
    with pytest.raises(ValueError, match="2-D"):
        plan.sddmm(g[0], x, out)
    with pytest.raises(ValueError, match="contiguous"):
        plan.sddmm(torch.zeros(37, 8, dtype=torch.float16).t(), x, out)
    with pytest.raises(TypeError):
        plan.sddmm(g.float(), x.float(), out)                                  # no plan dtype is float32 here
    with pytest.raises(gsa.GsError, match="not on the device"):
        plan.sddmm(g, x, out)                                                  # CPU tensors, plan not uploaded
    with pytest.raises(gsa.GsError, match="not on the device"):
        plan.sddmm_prepare()
    assert (out == 7).all()
    # the C entry point itself: refused (GS_ERR) before the pointers are looked at
    L = plan._L
    buf = (ctypes.c_uint16 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.gs_sddmm(plan._h, p, p, 1, p, None) == -1 and "not on the device" in L.gs_last_error().decode()
    assert L.gs_sddmm(plan._h, p, p, 0, p, None) == -1
    assert L.gs_sddmm(plan._h, None, p, 1, p, None) == -1
    plan.free()


def test_sparse_linear_grad_modes_without_a_gpu():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(6)
    w = rng.standard_normal((37, 48)).astype(np.float32)
    w[rng.random(w.shape) < 0.7] = 0.0
    wt = torch.from_numpy(w)
    with pytest.raises(ValueError, match="bogus"):
        gsa.SparseLinear.from_dense(wt, grad="bogus", upload=False)
    for grad in ("input", "all"):
        with pytest.raises(ValueError, match="FP8"):
            gsa.SparseLinear.from_dense(wt, grad=grad, weights="fp8", upload=False)
    layer = gsa.SparseLinear.from_dense(wt, torch.zeros(37), upload=False)
    with pytest.raises(ValueError, match="bogus"):
        gsa.SparseLinear(layer.plan, grad="bogus")
    assert layer.grad is None and not list(layer.parameters())
    with pytest.raises(RuntimeError, match="inference"):
        layer(torch.zeros(2, 48, requires_grad=True))       # the default layer: today's message
    with pytest.raises(RuntimeError, match="inference"):
        layer.prepare_backward()
    every = gsa.SparseLinear(layer.plan, torch.zeros(37), grad="all")
    names = dict(every.named_parameters())
    assert set(names) == {"values", "bias"} and names["bias"].dtype == names["values"].dtype == torch.float32
    wr, wc = np.nonzero(w)
    assert np.array_equal(names["values"].detach().numpy(), w[wr, wc])
    only_x = gsa.SparseLinear(layer.plan, torch.zeros(37), grad="input")
    assert not list(only_x.parameters()) and only_x.bias.dtype == torch.float32
    assert "grad='input'" in repr(only_x)
    layer.plan.free()


def test_the_sanitizer_program_of_the_pattern_builder():
    """tools/sddmm_layout_check.cc, a stand-alone program, built with the Makefile's SANFLAGS (ASan + UBSan on
    the host objects) and run: hand-written patterns against tables.  It is part of `make san_check`; the
    whole target, tools/gather_layout_check.cc included (its expectations follow the gather layouts' padding
    columns again), runs in tests/test_san_check.py."""
    dry = subprocess.run(["make", "-n", "-B", "-C", CSRC, "san_check"], capture_output=True, text=True, check=True).stdout
    assert "./build_san/sddmm_layout_check" in dry
    link = [ln for ln in dry.splitlines() if "-o build_san/sddmm_layout_check" in ln]
    assert link and "-fsanitize=address,undefined" in link[0], link
    subprocess.run(["make", "-s", "-j", str(min(16, os.cpu_count() or 8)), "-C", CSRC, "build_san/sddmm_layout_check"], check=True)
    run = subprocess.run([os.path.join(CSRC, "build_san", "sddmm_layout_check")], capture_output=True, text=True)
    assert run.returncode == 0 and "sddmm_layout_check: ok" in run.stdout, run.stdout + run.stderr
