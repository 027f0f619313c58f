"""GPU checks of k_mfma_ks with window positions (KS_WPOS): the kernel scatters the same wave images
as with u16 positions, so C must equal the u16 plan's C bit for bit (and meet tests/tolerance.py
against the CPU oracle).  The shapes cover window boundaries that do not divide the block height
(40, 56, 112 rows), the zero row's window, k-steps without entries (the random-rows matrix has
empty rows and short rows), more than 64 groups per k-step (112 and 128 rows: MAXG > 1), and a
ragged shape (a K tail that is no multiple of 32 and a short last row block)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle_ffi as ofi  # noqa: E402
from tolerance import bound, rel_err  # noqa: E402

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from generalsparse_amd import datasets as ds  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 32
M0, K0 = 640, 2048


@functools.lru_cache(maxsize=None)
def case(name):
    """(M, K, row, col, val, B on the GPU, fp64 oracle on the fp16-rounded operands), once per matrix"""
    if name == "pruned":
        M, K = M0, K0
        row, col, val = ds.pruned_weight(M, K, 0.7, 8)
    elif name == "random_rows":
        M, K = M0, K0
        row, col, val = ds.random_rows(M, K, 400.0, seed=3, empty_frac=0.2)
    else:  # ragged: a short last row block, a K tail that is no multiple of 32
        M, K = 650, 2000
        row, col, val = ds.pruned_weight(M, K, 0.7, 9)
    B = np.random.default_rng(17).uniform(-1, 1, (K, N)).astype(np.float16)
    ref = ofi.spmm_ref(M, N, row, col, val.astype(np.float16).astype(np.float32), B.astype(np.float32), "f64")
    ref.setflags(write=False)
    return M, K, row, col, val, torch.from_numpy(B).to(DEV), ref


def build(M, K, row, col, val, rows, over):
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        return gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", N, rows, 1).compile().upload("f16", 0)
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def check_pair(name, rows, split, nt):
    M, K, row, col, val, B, ref = case(name)
    p16 = build(M, K, row, col, val, rows, {"KS_SPLIT": split, "KS_NT": nt, "KS_WPOS": 0})
    pw = build(M, K, row, col, val, rows, {"KS_SPLIT": split, "KS_NT": nt, "KS_WPOS": 1})
    i16, iw = p16.info(), pw.info()
    assert i16["device_kernel"] == iw["device_kernel"] == "k_mfma_ks", (i16, iw)
    assert i16["ks_wpos"] == 0 and iw["ks_wpos"] == 1 and iw["ks_nt"] == nt, (i16, iw)
    assert iw["ksplit"] == i16["ksplit"]
    assert iw["tile_bytes"] < i16["tile_bytes"] and iw["device_bytes_A"] < i16["device_bytes_A"], (i16, iw)
    C16 = p16.spmm(B)
    Cw = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float16)
    pw.spmm(B, C=Cw)
    torch.cuda.synchronize()
    p16.device_status()
    pw.device_status()
    c16, cw = C16.cpu().numpy(), Cw.cpu().numpy()
    np.testing.assert_array_equal(cw.view(np.uint16), c16.view(np.uint16))
    err = rel_err(cw, ref)
    assert err <= bound("f16", "k_mfma_ks"), err
    p16.free()
    return pw, cw


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("split", [0, 1, 3])
@pytest.mark.parametrize("rows", [40, 56, 80, 112, 128])
@pytest.mark.parametrize("name", ["pruned", "random_rows"])
def test_wpos_equals_the_u16_plan_bit_for_bit(name, rows, split, nt):
    pw, _ = check_pair(name, rows, split, nt)
    pw.free()


@pytest.mark.parametrize("nt", [0, 1])
@pytest.mark.parametrize("rows", [40, 112])
def test_wpos_ragged_shape(rows, nt):
    """M = 650, K = 2000: the last row block is short and the last k-step has 16 rows of B (the
    rows past K are stored as zeros)"""
    pw, _ = check_pair("ragged", rows, 3, nt)
    pw.free()


def test_wpos_grouped_launch_and_no_mixing_with_u16():
    """two replicas of a KS_WPOS plan run as ONE grouped launch with the single launch's bits; a
    KS_WPOS entry and a u16 entry of the same shape never share a launch"""
    M, K, row, col, val, B, ref = case("pruned")
    pw, cw = check_pair("pruned", 80, 0, 1)
    pw.add_replica()
    p16 = build(M, K, row, col, val, 80, {"KS_NT": 1, "KS_WPOS": 0})
    B2 = (B.float() * 0.5).to(torch.float16)
    single2 = pw.spmm(B2)
    single16 = p16.spmm(B2)
    torch.cuda.synchronize()
    Cs = [torch.full((M, N), float("nan"), device=DEV, dtype=torch.float16) for _ in range(2)]
    bat = gsa.Batch([(pw, 0, B, Cs[0]), (pw, 1, B2, Cs[1])], N)
    assert bat.launches() == [2], bat.launches()
    bat.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Cs[0].cpu().numpy().view(np.uint16), cw.view(np.uint16))
    assert torch.equal(Cs[1].view(torch.int16), single2.view(torch.int16))
    Cs = [torch.full((M, N), float("nan"), device=DEV, dtype=torch.float16) for _ in range(3)]
    bat = gsa.Batch([(pw, 0, B, Cs[0]), (p16, 0, B2, Cs[1]), (pw, 1, B2, Cs[2])], N)
    assert bat.launches() == [1, 1, 1], bat.launches()
    bat.run(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(Cs[0].cpu().numpy().view(np.uint16), cw.view(np.uint16))
    assert torch.equal(Cs[1].view(torch.int16), single16.view(torch.int16))
    assert torch.equal(Cs[2].view(torch.int16), single2.view(torch.int16))
    for p in (pw, p16):
        p.device_status()
        p.free()


def test_wpos_saved_and_loaded_plan_computes_the_same(tmp_path):
    M, K, row, col, val, B, ref = case("pruned")
    over = {"KS_SPLIT": 1, "KS_NT": 1, "KS_WPOS": 1}
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        p = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", N, 40, 1).compile()
        p.save(tmp_path / "plan.bin")
        p.upload("f16", 0)
        q = gsa.Plan.load(tmp_path / "plan.bin").upload("f16", 0)
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)
    assert p.info()["ks_wpos"] == 1 and q.info()["ks_wpos"] == 1, (p.info(), q.info())
    Cp, Cq = p.spmm(B), q.spmm(B)
    torch.cuda.synchronize()
    assert torch.equal(Cp.view(torch.int16), Cq.view(torch.int16))
    assert rel_err(Cq.cpu().numpy(), ref) <= bound("f16", "k_mfma_ks")
    for x in (p, q):
        x.device_status()
        x.free()


def test_wpos_refusals_and_fallback():
    """bf16 plans refuse KS_WPOS with a message; N = 128 falls back to the u16 layout"""
    M, K, row, col, val, B, ref = case("pruned")
    old = gsa.get_config("KS_WPOS")
    try:
        gsa.set_config("KS_WPOS", 1)
        with pytest.raises(gsa.GsError, match="KS_WPOS"):
            gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", N, 40, 1).compile().upload("bf16", 0)
        p = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", 128, 40, 1).compile().upload("f16", 0)
    finally:
        gsa.set_config("KS_WPOS", old)
    info = p.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ks_wpos"] == 0, info
    B128 = torch.from_numpy(np.random.default_rng(3).uniform(-1, 1, (K, 128)).astype(np.float16)).to(DEV)
    C = p.spmm(B128)
    torch.cuda.synchronize()
    r128 = ofi.spmm_ref(M, 128, row, col, val.astype(np.float16).astype(np.float32), B128.float().cpu().numpy(), "f64")
    assert rel_err(C.cpu().numpy(), r128) <= bound("f16", "k_mfma_ks")
    p.device_status()
    p.free()
