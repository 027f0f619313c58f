"""Host-side checks of the SpMM epilogue interface (no GPU): the three entry points are exported
and bound, the activation name is refused before anything touches a device, and the EPILOGUE_FUSE
config key round-trips.  The GPU side is tests/test_gpu_epilogue.py."""
import ctypes

import numpy as np
import pytest

import generalsparse_amd as gsa
from generalsparse_amd import _lib

ENTRY_POINTS = ("gs_spmm_ex", "gs_spmm_batch_ex", "gs_plan_epilogue_fused")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_are_exported_and_bound(name):
    assert name in _lib.SIGNATURES
    fn = getattr(gsa.load_library(), name)
    args, res = _lib.SIGNATURES[name]
    assert fn.argtypes == args and fn.restype is res is ctypes.c_int


def test_gs_epilogue_struct_is_24_bytes():
    """alpha, activation, bias, residual: the layout of include/generalsparse.h's gs_epilogue"""
    assert ctypes.sizeof(_lib.GsEpilogue) == 24
    assert [f[0] for f in _lib.GsEpilogue._fields_] == ["alpha", "activation", "bias", "residual"]
    assert (_lib.GsEpilogue.alpha.offset, _lib.GsEpilogue.activation.offset, _lib.GsEpilogue.bias.offset,
            _lib.GsEpilogue.residual.offset) == (0, 4, 8, 16)


def small_plan():
    row = np.array([0, 0, 1, 2], np.uint64)
    col = np.array([0, 2, 1, 3], np.uint64)
    return gsa.Plan.from_coo(3, 4, row, col, np.ones(4, np.float32))


def test_unknown_activation_is_a_value_error_without_a_gpu():
    """the name is checked first: before the plan's device state or the operands are looked at"""
    plan = small_plan()
    with pytest.raises(ValueError, match="gelu"):
        plan.spmm(None, activation="gelu")
    with pytest.raises(ValueError, match="gelu"):
        gsa.Batch([(plan, 0, 0, 0)], 8, epilogues=[{"activation": "gelu"}])
    with pytest.raises(ValueError, match="beta"):
        gsa.Batch([(plan, 0, 0, 0)], 8, epilogues=[{"beta": 1.0}])
    with pytest.raises(ValueError):
        gsa.Batch([(plan, 0, 0, 0)], 8, epilogues=[])
    plan.free()


def test_epilogue_fused_needs_an_uploaded_plan():
    plan = small_plan()
    with pytest.raises(gsa.GsError) as ex:
        plan.epilogue_fused(8)
    assert ex.value.code == -1
    plan.free()


def test_epilogue_fuse_config_round_trips():
    assert gsa.get_config("EPILOGUE_FUSE") == 1  # the default
    try:
        gsa.set_config("EPILOGUE_FUSE", 0)
        assert gsa.get_config("EPILOGUE_FUSE") == 0
    finally:
        gsa.set_config("EPILOGUE_FUSE", 1)
    assert gsa.get_config("EPILOGUE_FUSE") == 1
