"""Host-side checks of the token-major linear interface (no GPU): the two entry points are exported
and bound, a plan that is not on the device is refused by gs_linear and reports linear_fused 0, the
LINEAR_FUSE config key round-trips, SparseLinear.from_dense builds the plan of a pruned weight, and
the activation name is refused before anything touches a device.  The GPU side is
tests/test_gpu_linear.py."""
import ctypes

import numpy as np
import pytest

import generalsparse_amd as gsa
from generalsparse_amd import _lib

ENTRY_POINTS = ("gs_linear", "gs_plan_linear_fused")


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_entry_points_are_exported_and_bound(name):
    assert name in _lib.SIGNATURES
    fn = getattr(gsa.load_library(), name)
    args, res = _lib.SIGNATURES[name]
    assert fn.argtypes == args and fn.restype is res is ctypes.c_int


def test_header_declares_them():
    import os
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "generalsparse.h")
    text = open(header).read()
    for name in ENTRY_POINTS:
        assert f"int {name}(gs_plan_t *p" in text, name


def compiled_plan():
    row = np.array([0, 0, 1, 2], np.uint64)
    col = np.array([0, 2, 1, 3], np.uint64)
    return gsa.Plan.from_coo(3, 4, row, col, np.ones(4, np.float32)).run_pipeline("warp_total", 8, 0, 1).compile()


def test_a_plan_that_is_not_uploaded():
    """gs_linear returns GS_ERR (-1) before it looks at the pointers' memory; linear_fused is 0"""
    plan = compiled_plan()
    L = plan._L
    x = (ctypes.c_uint16 * 32)()
    y = (ctypes.c_uint16 * 24)()
    rc = L.gs_linear(plan._h, 0, ctypes.cast(x, ctypes.c_void_p), ctypes.cast(y, ctypes.c_void_p), 8, None, None)
    assert rc == -1, rc
    assert "not on the device" in L.gs_last_error().decode()
    assert L.gs_plan_linear_fused(plan._h, 8) == 0 and plan.linear_fused(8) == 0
    assert L.gs_plan_linear_fused(plan._h, 0) == -1  # n_tokens >= 1
    assert L.gs_linear(plan._h, 0, ctypes.cast(x, ctypes.c_void_p), ctypes.cast(y, ctypes.c_void_p), 0, None, None) == -1
    plan.free()


def test_linear_fuse_config_round_trips():
    assert gsa.get_config("LINEAR_FUSE") == 1  # the default
    try:
        gsa.set_config("LINEAR_FUSE", 0)
        assert gsa.get_config("LINEAR_FUSE") == 0
    finally:
        gsa.set_config("LINEAR_FUSE", 1)
    assert gsa.get_config("LINEAR_FUSE") == 1


def test_unknown_activation_is_a_value_error_without_a_gpu():
    """the name is checked first: before the plan's device state or the operands are looked at"""
    plan = compiled_plan()
    with pytest.raises(ValueError, match="gelu"):
        plan.linear(None, activation="gelu")
    plan.free()


def test_sparse_linear_from_dense_without_upload():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    w = rng.standard_normal((37, 48)).astype(np.float32)
    w[rng.random(w.shape) < 0.7] = 0.0
    w[11] = 0.0  # an empty row inside
    with pytest.raises(ValueError, match="gelu"):
        gsa.SparseLinear.from_dense(torch.from_numpy(w), activation="gelu", upload=False)
    layer = gsa.SparseLinear.from_dense(torch.from_numpy(w), torch.zeros(37), tokens=32, pipeline=("warp_total", 0, 1),
                                        activation="relu", upload=False)
    assert isinstance(layer, torch.nn.Module) and layer.tokens == 32
    info = layer.plan.info()
    assert (info["rows"], info["cols"], info["nnz"]) == (37, 48, int(np.count_nonzero(w))), info
    assert (layer.out_features, layer.in_features) == (37, 48) and layer.bias.dtype == torch.float32
    assert info["replicas"] == 0 and layer.plan.linear_fused(32) == 0
    assert "in_features=48" in repr(layer) and "linear_fused(32)=0" in repr(layer), repr(layer)
    with pytest.raises(ValueError):
        gsa.SparseLinear(layer.plan, bias=torch.zeros(36))
    with pytest.raises(ValueError, match="gelu"):
        gsa.SparseLinear(layer.plan, activation="gelu")
    x = torch.zeros(2, 48, requires_grad=True)
    with pytest.raises(RuntimeError, match="inference"):
        layer(x)
    layer.plan.free()
