"""Host-side checks of the token-major linear at any token count (no GPU): the new entry points are
exported, bound and declared, a plan that is not on the device is refused, the LINEAR_WS_KB key
round-trips, and the arithmetic that sizes the K-split state of a token tile and splits a call into
launches (gs_linear_tile_split) gives hand-computed values.  The GPU side is
tests/test_gpu_linear_tokens.py."""
import ctypes
import os

import numpy as np
import pytest

import generalsparse_amd as gsa
from generalsparse_amd import _lib

ENTRY_POINTS = ("gs_plan_linear_launches", "gs_linear_tile_split")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_are_exported_and_bound(name):
    assert name in _lib.SIGNATURES
    fn = getattr(gsa.load_library(), name)
    args, res = _lib.SIGNATURES[name]
    assert fn.argtypes == args and fn.restype is res is ctypes.c_int


def test_header_declares_them():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "generalsparse.h")
    text = open(header).read()
    assert "int gs_plan_linear_launches(gs_plan_t *p, int n_tokens, int *tiles, int cap);" in text
    assert "int gs_linear_tile_split(uint64_t row_blocks, int k_ranges, int row_tiles, int n_tokens, long long ws_kb," in text


def test_a_plan_that_is_not_uploaded():
    row = np.array([0, 0, 1, 2], np.uint64)
    col = np.array([0, 2, 1, 3], np.uint64)
    plan = gsa.Plan.from_coo(3, 4, row, col, np.ones(4, np.float32)).run_pipeline("warp_total", 8, 0, 1).compile()
    L = plan._L
    buf = (ctypes.c_int * 4)()
    assert L.gs_plan_linear_launches(plan._h, 8, buf, 4) < 0
    assert "not on the device" in L.gs_last_error().decode()
    assert L.gs_plan_linear_launches(plan._h, 0, buf, 4) < 0  # n_tokens >= 1
    assert L.gs_plan_linear_launches(plan._h, 8, None, 4) < 0  # cap entries without an array
    assert L.gs_plan_linear_launches(None, 8, buf, 4) < 0
    with pytest.raises(gsa.GsError):
        plan.linear_launches(8)
    assert plan.linear_fused(8) == 0 and plan.linear_fused(100) == 0
    plan.free()


def test_linear_ws_kb_round_trips():
    assert gsa.get_config("LINEAR_WS_KB") == 65536  # the default
    try:
        gsa.set_config("LINEAR_WS_KB", 100)
        assert gsa.get_config("LINEAR_WS_KB") == 100
    finally:
        gsa.set_config("LINEAR_WS_KB", 65536)
    assert gsa.get_config("LINEAR_WS_KB") == 65536


def split(nb, S, RT, n, kb, cap=64):
    L = gsa.load_library()
    buf = (ctypes.c_int * max(cap, 1))()
    per = ctypes.c_ulonglong(0)
    k = L.gs_linear_tile_split(nb, S, RT, n, kb, ctypes.byref(per), buf if cap else None, cap)
    return k, list(buf[:min(max(k, 0), cap)]), per.value


def test_tile_state_and_split_on_hand_values():
    # 4 row blocks of 3 row tiles over 3 K ranges: a tile's 32 tokens x 48 rows x 4 bytes = 6144 bytes of
    # slab per (row block, K range) -- 12 of them -- and 4 arrival counters
    per = 4 * 3 * 3 * 2048 + 4 * 4
    assert per == 73744
    assert split(4, 3, 3, 100, 65536) == (1, [4], per)      # 65536 KB hold 910 tiles
    assert split(4, 3, 3, 32, 65536) == (1, [1], per)
    assert split(4, 3, 3, 1, 65536) == (1, [1], per)
    assert split(4, 3, 3, 33, 65536) == (1, [2], per)
    assert split(4, 3, 3, 100, 72) == (4, [1, 1, 1, 1], per)   # 73728 bytes: not one tile's state -> one tile at a time
    assert split(4, 3, 3, 100, 73) == (4, [1, 1, 1, 1], per)   # 74752: one
    assert split(4, 3, 3, 100, 145) == (2, [2, 2], per)        # 148480 >= 2 * 73744 = 147488
    assert split(4, 3, 3, 100, 144) == (4, [1, 1, 1, 1], per)  # 147456 < 147488
    assert split(4, 3, 3, 100, 217) == (2, [3, 1], per)        # 222208 >= 3 * 73744 = 221232: a remainder of one tile
    assert split(4, 3, 3, 32 * 7, 217) == (3, [3, 3, 1], per)
    assert split(4, 3, 3, 32 * 8 - 5, 217) == (3, [3, 3, 2], per)
    assert split(4, 3, 3, 100, 0) == (4, [1, 1, 1, 1], per)
    assert split(4, 3, 3, 100, -5) == (4, [1, 1, 1, 1], per)
    # 65536 KB / 73744 = 910 tiles per launch: 29120 tokens; one more token is a second launch
    assert split(4, 3, 3, 910 * 32, 65536) == (1, [910], per)
    assert split(4, 3, 3, 910 * 32 + 1, 65536) == (2, [910, 1], per)
    # one K range keeps no state: the budget does not matter, the 14-bit tile count does
    assert split(4, 1, 3, 100, 0)[:2] == (1, [4])
    assert split(4, 1, 3, 16383 * 32, 0)[:2] == (1, [16383])
    assert split(4, 1, 3, 16383 * 32 + 1, 0)[:2] == (2, [16383, 1])
    # ... and the grid stays below 2^31 workgroups: 2^20 row blocks x 2 K ranges -> 1023 tiles
    assert split(1 << 20, 2, 2, 1024 * 32, 1 << 40)[:2] == (2, [1023, 1])
    # the count is returned whatever the array holds
    assert split(4, 3, 3, 100, 72, cap=2) == (4, [1, 1], per)
    assert split(4, 3, 3, 100, 72, cap=0) == (4, [], per)


def test_tile_split_refuses_bad_arguments():
    L = gsa.load_library()
    buf = (ctypes.c_int * 4)()
    for args in ((0, 3, 3, 100), (4, 0, 3, 100), (4, 3, 0, 100), (4, 3, 3, 0)):
        assert L.gs_linear_tile_split(*args, 65536, None, buf, 4) < 0, args
    assert L.gs_linear_tile_split(4, 3, 3, 100, 65536, None, None, 4) < 0
    assert L.gs_linear_tile_split(4, 3, 3, 100, 65536, None, buf, -1) < 0
