"""CPU checks of the grouped token-major linear's host side: the grid layout of one k_mfma_ks_tm_group launch
(gs_linear_group_layout), the argument checks of gs_linear_batch / gs_linear_batch_launches, which come before
any launch -- no GPU is needed to be refused -- and the LinearBatch constructor's own."""
import ctypes

import numpy as np
import pytest

import generalsparse_amd as gsa

CAP = 32  # kKsTmGroupMax


def arr(t, v):
    return (t * len(v))(*v)


# ------------------------------------------------------------------ the grid layout
def test_group_max():
    assert gsa.linear_group_max() == CAP


def test_a_single_entry_starts_at_zero():
    assert gsa.linear_group_layout([4], [1]) == [0, 4]
    assert gsa.linear_group_layout([12], [3]) == [0, 36]
    assert gsa.linear_group_layout([1], [1]) == [0, 1]


def test_hand_cases():
    # (nwg, T) = (4, 1), (12, 3), (8, 4): 4, 36 and 32 workgroups; 4 -> 8, 8 + 36 = 44 -> 48, 48 + 32 = 80
    assert gsa.linear_group_layout([4, 12, 8], [1, 3, 4]) == [0, 8, 48, 80]
    # an entry that ends on a multiple of 8 leaves no gap; the last entry's end is the grid, not rounded
    assert gsa.linear_group_layout([8, 16, 3], [1, 2, 3]) == [0, 8, 40, 49]
    assert gsa.linear_group_layout([3, 3], [3, 3]) == [0, 16, 25]


def test_every_begin_is_a_multiple_of_8_and_the_shares_do_not_overlap():
    rng = np.random.default_rng(5)
    for n in (2, 7, CAP):
        nwg = rng.integers(1, 500, n).tolist()
        T = rng.integers(1, 9, n).tolist()
        begin = gsa.linear_group_layout(nwg, T)
        assert len(begin) == n + 1 and begin[0] == 0
        for i in range(n):
            assert begin[i] % 8 == 0
            end = begin[i] + nwg[i] * T[i]
            assert end <= begin[i + 1] and begin[i + 1] - end < 8
        assert begin[n] == begin[n - 1] + nwg[-1] * T[-1]


def test_refused_layouts():
    with pytest.raises(gsa.GsError, match="2\\^31"):
        gsa.linear_group_layout([1 << 20, 1 << 20], [1 << 10, 1 << 10])  # 2^30 + 2^30 = 2^31
    with pytest.raises(gsa.GsError, match="2\\^31"):
        gsa.linear_group_layout([1 << 16], [1 << 16])  # one entry of 2^32
    assert gsa.linear_group_layout([0x7fffffff], [1]) == [0, 0x7fffffff]
    with pytest.raises(gsa.GsError, match="2\\^31"):
        gsa.linear_group_layout([0x7ffffff9, 1], [1, 1])  # the second begin rounds up to 2^31
    with pytest.raises(gsa.GsError, match="without workgroups"):
        gsa.linear_group_layout([4, 0], [1, 1])
    with pytest.raises(gsa.GsError, match="more than 32"):
        gsa.linear_group_layout([1] * (CAP + 1), [1] * (CAP + 1))
    assert len(gsa.linear_group_layout([1] * CAP, [1] * CAP)) == CAP + 1
    with pytest.raises(gsa.GsError):
        gsa.linear_group_layout([], [])
    with pytest.raises(ValueError):
        gsa.linear_group_layout([1, 2], [1])


# ------------------------------------------------------------------ the C ABI's refusals
def compiled_plan():
    """a plan that is compiled and not on the device"""
    M, K = 48, 64
    r, c = np.nonzero(np.random.default_rng(0).random((M, K)) < 0.3)
    plan = gsa.Plan.from_coo(M, K, r.astype(np.uint64), c.astype(np.uint64), np.ones(len(r), np.float32))
    return plan.run_pipeline("block_total", 32, 40, 1).compile()


def test_gs_linear_batch_refuses_before_any_launch():
    L = gsa.load_library()
    plan = compiled_plan()
    P, R = arr(ctypes.c_void_p, [plan._h]), arr(ctypes.c_int, [0])
    X, Y, T = arr(ctypes.c_void_p, [256]), arr(ctypes.c_void_p, [4096]), arr(ctypes.c_int, [32])  # never dereferenced
    bad = [
        ("null plans", (None, R, X, Y, T, None, 1, None), "bad argument"),
        ("null replicas", (P, None, X, Y, T, None, 1, None), "bad argument"),
        ("null X", (P, R, None, Y, T, None, 1, None), "bad argument"),
        ("null Y", (P, R, X, None, T, None, 1, None), "bad argument"),
        ("null n_tokens", (P, R, X, Y, None, None, 1, None), "bad argument"),
        ("negative n", (P, R, X, Y, T, None, -1, None), "bad argument"),
        ("a null plan", (arr(ctypes.c_void_p, [None]), R, X, Y, T, None, 1, None), "bad batch entry 0"),
        ("a null x", (P, R, arr(ctypes.c_void_p, [None]), Y, T, None, 1, None), "bad batch entry 0"),
        ("a null y", (P, R, X, arr(ctypes.c_void_p, [None]), T, None, 1, None), "bad batch entry 0"),
        ("no token", (P, R, X, Y, arr(ctypes.c_int, [0]), None, 1, None), "bad batch entry 0"),
        ("not uploaded", (P, R, X, Y, T, None, 1, None), "not on the device"),
    ]
    for what, args, msg in bad:
        assert L.gs_linear_batch(*args) == -1, what
        assert msg in L.gs_last_error().decode(), (what, L.gs_last_error())
    assert "batch entry 0: plan is not on the device" in L.gs_last_error().decode()
    # the entries are checked in order, each refusal by its number
    P2, R2 = arr(ctypes.c_void_p, [plan._h, None]), arr(ctypes.c_int, [0, 0])
    X2, Y2, T2 = arr(ctypes.c_void_p, [256, 256]), arr(ctypes.c_void_p, [4096, 8192]), arr(ctypes.c_int, [32, 32])
    assert L.gs_linear_batch(P2, R2, X2, Y2, T2, None, 2, None) == -1
    assert "batch entry 0" in L.gs_last_error().decode()
    P2[0], P2[1] = None, plan._h
    assert L.gs_linear_batch(P2, R2, X2, Y2, T2, None, 2, None) == -1
    assert "bad batch entry 0" in L.gs_last_error().decode()
    # an empty batch is no error and launches nothing
    assert L.gs_linear_batch(P, R, X, Y, T, None, 0, None) == 0


def test_gs_linear_batch_launches_refusals():
    L = gsa.load_library()
    plan = compiled_plan()
    P, R = arr(ctypes.c_void_p, [plan._h]), arr(ctypes.c_int, [0])
    X, T = arr(ctypes.c_void_p, [256]), arr(ctypes.c_int, [32])
    out = (ctypes.c_int * 4)()
    assert L.gs_linear_batch_launches(None, R, X, T, 1, out, 4) == -1
    assert L.gs_linear_batch_launches(P, R, X, T, 1, None, 4) == -1
    assert L.gs_linear_batch_launches(P, R, X, arr(ctypes.c_int, [0]), 1, out, 4) == -1
    assert L.gs_linear_batch_launches(P, R, X, T, 1, out, 4) == -1
    assert "not on the device" in L.gs_last_error().decode()
    assert L.gs_linear_batch_launches(P, R, X, T, 0, out, 4) == 0


# ------------------------------------------------------------------ the LinearBatch constructor
def test_linear_batch_constructor_refusals():
    """lengths and epilogue keys are checked first, before an operand or a device is looked at"""
    plan = compiled_plan()
    entries = [(plan, 0, None, None), (plan, 0, None, None)]
    with pytest.raises(ValueError, match="one item"):
        gsa.LinearBatch(entries, [None])
    with pytest.raises(ValueError, match="one item"):
        gsa.LinearBatch(entries, [None, None, None])
    with pytest.raises(ValueError, match="unknown epilogue keys"):
        gsa.LinearBatch(entries, [None, {"beta": 2.0}])
    with pytest.raises(ValueError, match="activation"):
        gsa.LinearBatch(entries, [{"activation": "gelu"}, None])
    with pytest.raises(ValueError, match=r"\(plan, replica, x, out\)"):
        gsa.LinearBatch([(plan, 0, None)])
    with pytest.raises(ValueError, match="replica"):
        gsa.LinearBatch([(plan, 1, None, None)])
    with pytest.raises(ValueError, match="out must be a tensor"):
        gsa.LinearBatch([(plan, 0, None, None)])
    empty = gsa.LinearBatch([])
    assert empty.launches() == [] and empty.run() is None
