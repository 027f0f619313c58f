"""torch.nn modules over the engine: SparseLinear, a pruned linear layer run by Plan.linear.

    layer = SparseLinear.from_dense(weight, bias, tokens=32, activation="relu")   # weight: (out, in), pruned
    y = layer(x)                                                                     # x: (..., in) -> (..., out)

Inference only: the engine has no backward pass."""
import numpy as np
import torch

from . import GS_W_FP8_E4M3, Plan, _check_activation, _dtype_code, _torch_dtype, _weights_code


class SparseLinear(torch.nn.Module):
    """y = activation(x @ W.T + bias) [+ residual] with W held as a compiled, uploaded Plan
    (gs_linear: activations token-major, as torch holds them, no transposes around the SpMM).
    plan: an uploaded Plan of the (out, in) weight; bias: None or `out` values (kept as a float32
    buffer on the plan's device); activation: None or "relu".
    tokens is the width the plan's tiles are built for, not a batch size the layer is tied to: a
    layer built with tokens=32 (a k_mfma_ks plan) runs the one kernel k_mfma_ks_tm at any token
    count -- 8 tokens of a decode step, 100 of a prefill chunk -- on ceil(n / 32) token tiles, and a
    token's output has the same bits in every such call (Plan.linear_fused, Plan.linear_launches)."""

    def __init__(self, plan, bias=None, activation=None):
        super().__init__()
        _check_activation(activation)  # before anything touches a device
        self.plan, self.activation = plan, activation
        info = plan.info()
        self.in_features, self.out_features = int(info["cols"]), int(info["rows"])
        self.tokens = int(info["lds_n"]) or None  # the width the plan's tiles were built for
        if bias is not None:
            bias = torch.as_tensor(bias).detach().to(torch.float32).reshape(-1).contiguous()
            if bias.numel() != self.out_features:
                raise ValueError(f"bias must hold {self.out_features} values (one per output feature)")
        self.register_buffer("bias", bias)

    @classmethod
    def from_dense(cls, weight, bias=None, *, tokens=32, dtype="f16", pipeline=("block_total", 40, 1), activation=None,
                   device=0, upload=True, weights=None, row_scale=None):
        """the plan from the non-zeros of a pruned (out, in) weight: from_coo, run_pipeline at
        N = tokens, compile, upload (upload=False stops before the device: the plan can be inspected,
        the module cannot run).  tokens: the tile width (17 .. 32 for the one-kernel path), whatever
        token counts forward will see.  weights="fp8" (with row_scale: one scale per output feature, or
        the default power-of-two rule): the weight's values as e4m3 codes, Plan.upload's weight-only
        quantisation -- activations, bias and output stay `dtype`, which must be f16"""
        _check_activation(activation)
        _dtype_code(dtype)
        _weights_code(weights)
        w = torch.as_tensor(weight).detach().to("cpu", torch.float32).numpy()
        if w.ndim != 2:
            raise ValueError("weight must be (out_features, in_features)")
        r, c = np.nonzero(w)  # row-major order: row-sorted, columns sorted inside a row
        name, p0, p1 = pipeline
        plan = Plan.from_coo(w.shape[0], w.shape[1], r.astype(np.uint64), c.astype(np.uint64), w[r, c])
        plan.run_pipeline(name, int(tokens), int(p0), int(p1)).compile()
        if upload:
            plan.upload(dtype, int(device), weights=weights, row_scale=row_scale)
            if bias is not None:
                bias = torch.as_tensor(bias).detach().to(torch.device("cuda", int(device)), torch.float32)
        layer = cls(plan, bias, activation)
        layer.tokens = int(tokens)
        return layer

    def forward(self, x, residual=None):
        """x: (..., in_features) of the plan's dtype on its device -> (..., out_features); the leading
        dimensions are flattened into the token count.  residual: (..., out_features), added last."""
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("SparseLinear is inference only (no backward pass): run it under torch.no_grad() "
                               "or on a tensor that does not require grad")
        if x.dim() < 1 or x.shape[-1] != self.in_features:
            raise ValueError(f"x must be (..., {self.in_features})")
        lead = tuple(x.shape[:-1])
        x2 = x.reshape(-1, self.in_features)
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        if residual is not None:
            if tuple(residual.shape) != lead + (self.out_features,):
                raise ValueError(f"residual must be {lead + (self.out_features,)}")
            residual = residual.reshape(-1, self.out_features)
            if not residual.is_contiguous():
                residual = residual.contiguous()
        y = self.plan.linear(x2, bias=self.bias, activation=self.activation, residual=residual)
        return y.reshape(lead + (self.out_features,))

    def extra_repr(self):
        info = self.plan.info()
        kernel = info["device_kernel"] or info["kernel_name"]
        s = f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, " \
            f"activation={self.activation!r}, kernel={kernel}"
        if self.tokens:
            s += f", linear_fused({self.tokens})={self.plan.linear_fused(self.tokens)}"
        if info["replicas"]:
            s += f", dtype={_torch_dtype(info['dtype'])}"
            if info["weights"] == GS_W_FP8_E4M3:
                s += ", weights=fp8_e4m3"
        return s
