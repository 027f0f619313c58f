"""GPU checks of SparseLinear's backward pass (nn.py: grad="input" / "all"): grad_x by Plan.linear on
plan_T, the plan of the transposed weight -- k_mfma_ks_tm when M is a multiple of 8, the three-launch
path otherwise -- grad_values by Plan.sddmm (k_sddmm_tm), grad_bias, grad_residual, the ReLU mask.

Integer operands as in tests/test_gpu_linear.py: ks_pattern(K) weights in {-2, -1, 1, 2}, integer x,
bias, residual and incoming gradient.  Every product and sum is exact in fp32 and in float64, so each
gradient must equal the float64 reference, cast once to its dtype, bit for bit."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits  # noqa: E402
from test_gpu_edges import DEV, TORCH_DT  # noqa: E402
from test_gpu_edges_mfma import ks_pattern, mfma_everywhere  # noqa: E402,F401  (fixture)

pytestmark = pytest.mark.gpu

CASES = [(K, M) for K in (40, 1176) for M in (120, 131)]  # M = 120: plan_T fused; 131: three launches


@functools.lru_cache(maxsize=None)
def weight(K, M):
    """(W: M x K float64, row, col of its non-zeros in np.nonzero's order)"""
    W = ks_pattern(K)[3][:M].copy()
    r, c = np.nonzero(W)
    return W, r, c


@functools.lru_cache(maxsize=None)
def operands(K, M, n):
    """integer x (n, K), bias (M), residual (n, M), incoming gradient (n, M) as float64 arrays"""
    rng = np.random.default_rng(31 * K + 7 * M + n)
    return (rng.integers(-2, 3, (n, K)).astype(np.float64), rng.integers(-3, 4, M).astype(np.float64),
            rng.integers(-2, 3, (n, M)).astype(np.float64), rng.integers(-2, 3, (n, M)).astype(np.float64))


def reference(W, r, c, x, bias, residual, gy, relu):
    """y and every gradient in float64 (exact: integers)"""
    a = x @ W.T + bias
    mask = a > 0 if relu else np.ones_like(a, bool)
    a = np.where(mask, a, 0.0) if relu else a
    g = np.where(mask, gy, 0.0)
    return {"y": a + (residual if residual is not None else 0.0), "x": g @ W, "residual": gy, "bias": g.sum(0),
            "values": (g.T @ x)[r, c]}


def to_dev(a, dtype, grad=False):
    return torch.from_numpy(a).to(DEV, dtype).requires_grad_(grad)


def same_bits(got, ref64, dtype, what):
    ref = torch.from_numpy(np.ascontiguousarray(ref64)).to(dtype).to(DEV)
    assert_bits(got.detach().reshape(-1, 1).contiguous(), ref.reshape(-1, 1), what)


def make_layer(K, M, dtype, bias, activation, grad):
    W = weight(K, M)[0]
    layer = gsa.SparseLinear.from_dense(torch.from_numpy(W), torch.from_numpy(bias), dtype=dtype, activation=activation, grad=grad)
    info = layer.plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and layer.plan.linear_fused(24) == 1, info
    return layer


def check_plans(layer, M, n):
    layer.plan.device_status()
    layer.plan_T.device_status()
    assert layer.plan_T.linear_fused(n) == (1 if M % 8 == 0 else 0)
    ti = layer.plan_T.info()
    assert (ti["rows"], ti["cols"], ti["nnz"]) == (layer.in_features, M, layer.plan.info()["nnz"])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K,M", CASES)
def test_grad_input(K, M, dtype, mfma_everywhere):
    """ReLU with a fused residual: x.grad = (gy masked by the activation's own output) @ W, residual.grad =
    gy; y has the bits of the layer without grad; a second backward accumulates"""
    td = TORCH_DT[dtype]
    W, r, c = weight(K, M)
    for n in (24, 100):
        x64, bias, res64, gy64 = operands(K, M, n)
        ref = reference(W, r, c, x64, bias, res64, gy64, True)
        layer = make_layer(K, M, dtype, bias, "relu", "input")
        assert not list(layer.parameters())
        plain = make_layer(K, M, dtype, bias, "relu", None)
        x, res, gy = to_dev(x64, td, True), to_dev(res64, td, True), to_dev(gy64, td)
        y = layer(x, residual=res)
        y0 = plain(x.detach(), residual=res.detach())
        assert y.requires_grad and not y0.requires_grad
        same_bits(y, ref["y"], td, f"y {dtype} K={K} M={M} n={n}")
        assert torch.equal(y.detach().view(torch.int16), y0.view(torch.int16))
        y.backward(gy, retain_graph=True)
        same_bits(x.grad, ref["x"], td, f"x.grad {dtype} K={K} M={M} n={n}")
        same_bits(res.grad, ref["residual"], td, f"residual.grad {dtype} K={K} M={M} n={n}")
        y.backward(gy)
        same_bits(x.grad, 2 * ref["x"], td, "x.grad after a second backward")
        same_bits(res.grad, 2 * ref["residual"], td, "residual.grad after a second backward")
        same_bits(gy, gy64, td, "the incoming gradient is left as it was")
        check_plans(layer, M, n)
        with pytest.raises(RuntimeError, match="inference"):
            plain(x)
        layer.plan.free(), layer.plan_T.free(), plain.plan.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K,M", CASES)
def test_grad_all(K, M, dtype, mfma_everywhere):
    """values.grad is the integer SDDMM reference and bias.grad the column sums of the masked gradient, in
    float32; without an activation at n = 24, with ReLU and a residual at n = 100"""
    td = TORCH_DT[dtype]
    W, r, c = weight(K, M)
    for n, act in ((24, None), (100, "relu")):
        x64, bias, res64, gy64 = operands(K, M, n)
        residual = res64 if act else None
        ref = reference(W, r, c, x64, bias, residual, gy64, act == "relu")
        layer = make_layer(K, M, dtype, bias, act, "all").prepare_backward()
        assert layer.values.dtype == layer.bias.dtype == torch.float32 and layer.values.numel() == len(r)
        x, gy = to_dev(x64, td, True), to_dev(gy64, td)
        res = to_dev(res64, td, True) if act else None
        y = layer(x, residual=res)
        same_bits(y, ref["y"], td, f"y {dtype} K={K} M={M} n={n}")
        with torch.no_grad():
            y0 = layer(x, residual=res)
        assert torch.equal(y.detach().view(torch.int16), y0.view(torch.int16))
        y.backward(gy, retain_graph=True)
        what = f"{dtype} K={K} M={M} n={n} {act}"
        same_bits(x.grad, ref["x"], td, "x.grad " + what)
        same_bits(layer.values.grad, ref["values"], torch.float32, "values.grad " + what)
        same_bits(layer.bias.grad, ref["bias"], torch.float32, "bias.grad " + what)
        if act:
            same_bits(res.grad, ref["residual"], td, "residual.grad " + what)
        y.backward(gy)
        same_bits(layer.values.grad, 2 * ref["values"], torch.float32, "values.grad after a second backward")
        same_bits(layer.bias.grad, 2 * ref["bias"], torch.float32, "bias.grad after a second backward")
        same_bits(gy, gy64, td, "the incoming gradient is left as it was")
        check_plans(layer, M, n)
        # only the parameters require grad: x does not
        layer.zero_grad()
        layer(x.detach(), residual=res.detach() if act else None).backward(gy)
        same_bits(layer.values.grad, ref["values"], torch.float32, "values.grad, x without grad")
        layer.plan.free(), layer.plan_T.free()


def test_leading_dimensions(mfma_everywhere):
    """x of shape (2, n / 2, K): the leading dimensions are flattened, the gradients come back in x's shape"""
    K, M, n, td = 40, 120, 24, torch.float16
    W, r, c = weight(K, M)
    x64, bias, res64, gy64 = operands(K, M, n)
    ref = reference(W, r, c, x64, bias, res64, gy64, True)
    layer = make_layer(K, M, "f16", bias, "relu", "all")
    x = to_dev(x64.reshape(2, n // 2, K), td, True)
    res = to_dev(res64.reshape(2, n // 2, M), td, True)
    y = layer(x, residual=res)
    assert tuple(y.shape) == (2, n // 2, M)
    y.backward(to_dev(gy64.reshape(2, n // 2, M), td))
    assert tuple(x.grad.shape) == tuple(x.shape) and tuple(res.grad.shape) == tuple(res.shape)
    same_bits(x.grad, ref["x"], td, "x.grad (2, n/2, K)")
    same_bits(layer.values.grad, ref["values"], torch.float32, "values.grad (2, n/2, K)")
    check_plans(layer, M, n)
    layer.plan.free(), layer.plan_T.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K,M", [(40, 131), (1176, 120)])
def test_sync_values(K, M, dtype, mfma_everywhere):
    """values.data += 1, sync_values(): the next forward and backward run on the changed weight"""
    td, n = TORCH_DT[dtype], 24
    W, r, c = weight(K, M)
    x64, bias, res64, gy64 = operands(K, M, n)
    layer = make_layer(K, M, dtype, bias, None, "all").prepare_backward()
    with torch.no_grad():
        layer.values += 1
    x, gy = to_dev(x64, td, True), to_dev(gy64, td)
    same_bits(layer(x), reference(W, r, c, x64, bias, None, gy64, False)["y"], td, "the forward before sync_values")
    layer.sync_values()
    W1 = W.copy()
    W1[r, c] += 1  # (entries that become 0 stay stored)
    ref = reference(W1, r, c, x64, bias, None, gy64, False)
    assert np.array_equal(layer.plan.values(), W1[r, c].astype(np.float32)) and layer.plan.info()["nnz"] == len(r)
    y = layer(x)
    same_bits(y, ref["y"], td, f"y after sync_values {dtype} K={K} M={M}")
    y.backward(gy)
    same_bits(x.grad, ref["x"], td, "x.grad after sync_values")
    same_bits(layer.values.grad, ref["values"], torch.float32, "values.grad after sync_values")
    check_plans(layer, M, n)
    layer.plan.free(), layer.plan_T.free()
