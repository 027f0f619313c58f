"""torch.nn modules over the engine: SparseLinear, a pruned linear layer run by Plan.linear.

    layer = SparseLinear.from_dense(weight, bias, tokens=32, activation="relu")   # weight: (out, in), pruned
    y = layer(x)                                                                     # x: (..., in) -> (..., out)

Inference only by default.  Gradients are opt-in:

    layer = SparseLinear.from_dense(weight, bias, grad="input")   # a frozen sparse layer gradients flow through
    layer = SparseLinear.from_dense(weight, bias, grad="all")     # ... and layer.values / layer.bias are trained
    loss(layer(x)).backward(); optimizer.step(); layer.sync_values()

The backward pass is the engine's own: grad_x = Plan.linear of the transposed weight (a second plan, so
the weight is resident twice), grad_values = Plan.sddmm (k_sddmm_tm, the product sampled at the
weight's non-zeros, in float32).  Once differentiable; FP8-weight layers stay inference only.

sync_values() carries layer.values into the uploaded plans on the GPU (Plan.set_values, k_set_values): no
plan is rebuilt, the plan objects and their device arrays stay where they are.  By default it also copies
the values to the CPU and refreshes the plans' host copies; sync_values(host=False) leaves the GPU not at
all, at the price of stale host values (Plan.values(), Plan.save() and a launch at another width refuse
until a sync_values() with host=True).  sync_values(rebuild=True) is the host-side rebuild of both plans."""
import numpy as np
import torch

from . import GS_W_FP8_E4M3, GsError, LinearBatch, Plan, _check_activation, _dtype_code, _torch_dtype, _weights_code

GRAD_MODES = (None, "input", "all")


def _check_grad(grad):
    """the gradient mode; checked before anything touches a device"""
    if grad not in GRAD_MODES:
        raise ValueError(f"grad must be None, 'input' or 'all', not {grad!r}")
    return grad


class _SparseLinearFn(torch.autograd.Function):
    """y = layer's Plan.linear(x) -- the call and the bits of the inference path -- with the engine's
    backward.  values and bias are inputs only so that autograd routes their gradients: the forward runs
    on the values the plan holds (SparseLinear.sync_values)."""

    @staticmethod
    def forward(ctx, x, residual, values, bias, layer):
        plan, act = layer.plan, layer.activation
        b = bias.detach() if bias is not None else None
        y = plan.linear(x, bias=b, activation=act, residual=residual)
        mask = None
        if act == "relu":
            # the activation's own output decides the mask; with a residual fused after it that output
            # is not y: it is computed once more without the residual, never from y - residual
            mask = (y if residual is None else plan.linear(x, bias=b, activation=act)) > 0
        ctx.layer, ctx.plan = layer, plan
        ctx.save_for_backward(x, mask)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gy):
        x, mask = ctx.saved_tensors
        need_x, need_res, need_val, need_bias = ctx.needs_input_grad[:4]
        gy = gy.contiguous()
        g = gy if mask is None else torch.where(mask, gy, torch.zeros((), dtype=gy.dtype, device=gy.device))
        grad_x = ctx.layer.prepare_backward().plan_T.linear(g) if need_x else None
        grad_values = ctx.plan.sddmm(g, x) if need_val else None
        grad_bias = g.float().sum(0) if need_bias else None
        # (the residual's gradient is a copy: autograd may keep a returned tensor as .grad and add to it in place)
        return grad_x, (gy.clone() if need_res else None), grad_values, grad_bias, None


class SparseLinear(torch.nn.Module):
    """y = activation(x @ W.T + bias) [+ residual] with W held as a compiled, uploaded Plan
    (gs_linear: activations token-major, as torch holds them, no transposes around the SpMM).
    plan: an uploaded Plan of the (out, in) weight; bias: None or `out` values (kept as a float32
    buffer on the plan's device); activation: None or "relu".
    tokens is the width the plan's tiles are built for, not a batch size the layer is tied to: a
    layer built with tokens=32 (a k_mfma_ks plan) runs the one kernel k_mfma_ks_tm at any token
    count -- 8 tokens of a decode step, 100 of a prefill chunk -- on ceil(n / 32) token tiles, and a
    token's output has the same bits in every such call (Plan.linear_fused, Plan.linear_launches).

    grad: None -- inference only, an input that requires grad is refused; "input" -- gradients flow to
    x, and to residual when given; "all" -- also to layer.values, a float32 Parameter of the plan's nnz
    stored values in Plan.pattern()'s order (np.nonzero's for from_dense), and to layer.bias, a float32
    Parameter in this mode only.  The forward under grad is the same Plan.linear call with the same
    bits (ReLU with a residual runs it a second time, without the residual, for the mask).  The
    backward needs plan_T, a plan of the transposed weight built from the pattern with the layer's
    pipeline, token width, dtype and device -- on the first backward, or by prepare_backward() -- which
    DOUBLES the resident weight.  The forward keeps running on the values the plans hold: after an
    optimizer step sync_values() writes layer.values into both uploaded plans in place, on the GPU (one
    small kernel per plan; the plans' gather maps, 4 bytes per value slot each, are uploaded by
    prepare_backward or by the first sync_values).
    A layer with FP8 weights is inference only: asking it for grad raises."""

    def __init__(self, plan, bias=None, activation=None, grad=None):
        super().__init__()
        _check_activation(activation)  # before anything touches a device
        _check_grad(grad)
        self.plan, self.activation, self.grad = plan, activation, grad
        self.plan_T = None
        self._order = None  # plan_T's entries in layer.values' order: an index tensor on the device (prepare_backward)
        info = plan.info()
        if grad is not None and info["weights"] == GS_W_FP8_E4M3:
            raise ValueError("a SparseLinear with FP8 weights is inference only: the transposed product would run on "
                             "other weights than the forward did")
        self.in_features, self.out_features = int(info["cols"]), int(info["rows"])
        self.tokens = int(info["lds_n"]) or None  # the width the plan's tiles were built for
        # how plan_T (and sync_values' plans) are built; from_dense records its own arguments
        self._build = {"tokens": self.tokens or 32, "dtype": info["dtype"], "pipeline": ("block_total", 40, 1),
                       "device": getattr(plan, "_device", 0), "rebuild": False}
        if bias is not None:
            bias = torch.as_tensor(bias).detach().to(torch.float32).reshape(-1).contiguous()
            if bias.numel() != self.out_features:
                raise ValueError(f"bias must hold {self.out_features} values (one per output feature)")
        if grad == "all":
            self.register_parameter("bias", torch.nn.Parameter(bias) if bias is not None else None)
            values = torch.from_numpy(plan.values())
            if info["replicas"]:
                values = values.to(torch.device("cuda", self._build["device"]))
            self.values = torch.nn.Parameter(values)
        else:
            self.register_buffer("bias", bias)

    @classmethod
    def from_dense(cls, weight, bias=None, *, tokens=32, dtype="f16", pipeline=("block_total", 40, 1), activation=None,
                   device=0, upload=True, weights=None, row_scale=None, grad=None):
        """the plan from the non-zeros of a pruned (out, in) weight: from_coo, run_pipeline at
        N = tokens, compile, upload (upload=False stops before the device: the plan can be inspected,
        the module cannot run).  tokens: the tile width (17 .. 32 for the one-kernel path), whatever
        token counts forward will see.  weights="fp8" (with row_scale: one scale per output feature, or
        the default power-of-two rule): the weight's values as e4m3 codes, Plan.upload's weight-only
        quantisation -- activations, bias and output stay `dtype`, which must be f16; not with grad.
        grad: the constructor's"""
        _check_activation(activation)
        _check_grad(grad)
        code, wcode = _dtype_code(dtype), _weights_code(weights)
        if grad is not None and wcode == GS_W_FP8_E4M3:
            raise ValueError("a SparseLinear with FP8 weights is inference only: grad must be None")
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
        layer = cls(plan, bias, activation, grad)
        layer.tokens = int(tokens)
        layer._build = {"tokens": int(tokens), "dtype": code, "pipeline": (name, int(p0), int(p1)), "device": int(device),
                        "rebuild": True}
        return layer

    # ------------------------------------------------------------- backward
    def _plan_of(self, n_rows, n_cols, row, col, val):
        b = self._build
        name, p0, p1 = b["pipeline"]
        plan = Plan.from_coo(n_rows, n_cols, row, col, val).run_pipeline(name, b["tokens"], p0, p1).compile()
        return plan.upload(b["dtype"], b["device"])

    def _current_values(self):
        if self.grad == "all":
            return self.values.detach().to("cpu", torch.float32).numpy()
        return self.plan.values()

    def prepare_backward(self):
        """builds plan_T, the plan of the transposed weight that grad_x runs on, now rather than in the
        first backward (host-side plan building and an upload; the weight is then resident twice).  With
        grad="all" it also uploads both plans' value maps (Plan.values_prepare), so that a later
        sync_values() allocates nothing"""
        if self.grad is None:
            raise RuntimeError("SparseLinear(grad=None) is inference only: build it with grad='input' or 'all'")
        if self.plan_T is None:
            row, col = self.plan.pattern()
            val = self._current_values()
            order = np.lexsort((row, col))  # by column, then row: the transposed weight, row-major
            self.plan_T = self._plan_of(self.in_features, self.out_features, col[order], row[order], val[order])
            self._order = None
            if self.grad == "all":
                self._order = torch.from_numpy(order.astype(np.int64)).to(self.values.device)
        if self.grad == "all":
            for plan in (self.plan, self.plan_T):
                try:
                    plan.values_prepare()
                except GsError:
                    pass  # (a plan set_values refuses: sync_values rebuilds it on the host)
        return self

    def _rebuild(self, transposed):
        """the host-side way: one plan built from the pattern and the current layer.values, and uploaded"""
        if not self._build["rebuild"]:
            raise RuntimeError("rebuilding a plan on the host is for SparseLinear.from_dense layers, which remember how "
                               "their plan was built")
        if transposed:
            self.plan_T = None
            return self.prepare_backward()
        row, col = self.plan.pattern()
        self.plan = self._plan_of(self.out_features, self.in_features, row, col, np.ascontiguousarray(self._current_values()))
        return self

    def sync_values(self, rebuild=False, host=True):
        """carries the current layer.values into the plan (and plan_T, if built), so that an optimizer step
        reaches the forward and the backward.  On the GPU: Plan.set_values rewrites the uploaded plans' value
        arrays in place (k_set_values); no plan is rebuilt, layer.plan and layer.plan_T stay the same objects
        with the same device arrays, for any layer with grad="all", from_dense or wrapped around an uploaded plan.
        host=True (the default) also copies the values to the CPU and refreshes the plans' host copies, so
        Plan.values(), Plan.save() and a launch at another dense width keep working; host=False leaves the
        GPU not at all and leaves those host copies stale (they refuse until a sync_values() with host=True).
        A plan set_values refuses -- one off k_mfma_ks, or one that holds its CSR on the device, as plan_T does
        once it ran the three-launch path (out_features not a multiple of 8) -- is rebuilt on the host instead,
        that plan only.  rebuild=True is the host-side way for both: two plan builds and uploads (slow; for
        from_dense layers, which remember how their plan was built)."""
        if self.grad != "all":
            raise RuntimeError("sync_values is for SparseLinear layers with grad='all'")
        if rebuild:
            had_T = self.plan_T is not None
            self._rebuild(False)
            self.plan_T = None
            if had_T:
                self.prepare_backward()
            return self
        values = self.values.detach()
        if not values.is_contiguous():
            values = values.contiguous()
        try:
            self.plan.set_values(values, host=host)
        except GsError as e:
            if e.code != -1:  # (only a refusal, which launched nothing, falls back)
                raise
            self._rebuild(False)
        if self.plan_T is not None:
            try:
                self.plan_T.set_values(values[self._order], host=host)
            except GsError as e:
                if e.code != -1:
                    raise
                self._rebuild(True)
        return self

    def forward(self, x, residual=None):
        """x: (..., in_features) of the plan's dtype on its device -> (..., out_features); the leading
        dimensions are flattened into the token count.  residual: (..., out_features), added last."""
        lead, x2, residual = self._flatten(x, residual)
        if self._wants_grad(x2, residual):
            values = self.values if self.grad == "all" else None
            y = _SparseLinearFn.apply(x2, residual, values, self.bias, self)
            return y.reshape(lead + (self.out_features,))
        bias = self.bias.detach() if isinstance(self.bias, torch.nn.Parameter) else self.bias
        y = self.plan.linear(x2, bias=bias, activation=self.activation, residual=residual)
        return y.reshape(lead + (self.out_features,))

    def _flatten(self, x, residual):
        """forward's operands as Plan.linear takes them: (leading shape, x as (n, in), residual as (n, out) or
        None), after forward's refusals"""
        if self.grad is None and torch.is_grad_enabled() and x.requires_grad:
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
        return lead, x2, residual

    def _wants_grad(self, x2, residual):
        """forward goes through autograd (_SparseLinearFn): grad is enabled and an operand asks for it"""
        if self.grad is None or not torch.is_grad_enabled():
            return False
        values = self.values if self.grad == "all" else None
        return any(t is not None and t.requires_grad for t in (x2, residual, values, self.bias))

    def extra_repr(self):
        info = self.plan.info()
        kernel = info["device_kernel"] or info["kernel_name"]
        s = f"in_features={self.in_features}, out_features={self.out_features}, bias={self.bias is not None}, " \
            f"activation={self.activation!r}, kernel={kernel}"
        if self.grad is not None:
            s += f", grad={self.grad!r}"
        if self.tokens:
            s += f", linear_fused({self.tokens})={self.plan.linear_fused(self.tokens)}"
        if info["replicas"]:
            s += f", dtype={_torch_dtype(info['dtype'])}"
            if info["weights"] == GS_W_FP8_E4M3:
                s += ", weights=fp8_e4m3"
        return s


class SparseLinearGroup(torch.nn.Module):
    """several SparseLinear layers run as one call (LinearBatch, gs_linear_batch): the Q/K/V projections of one
    x, an MLP's gate / up pair, experts with their own inputs and token counts.  layers: SparseLinear modules
    (kept as a ModuleList).  forward returns the list of their outputs, each with the bits of the layer's own
    forward.  Layers whose calls are each one k_mfma_ks_tm launch of one instantiation share ONE grouped
    launch; every other layer runs inside the same call through its own path (LinearBatch.launches tells).
    Each layer's bias and activation are its entry's epilogue.
    When grad is enabled and any input, residual, layer.values or layer.bias requires grad, the layers are
    called one by one, so autograd works as for the single layer; a grad=None layer refuses an input that
    requires grad, as alone.  Layers that share a plan object would share its replica 0 -- its K-split tickets
    and slabs -- so such a group is also called one by one.
    A LinearBatch is built per forward (a few ctypes arrays; nothing is cached by data pointer)."""

    def __init__(self, layers):
        super().__init__()
        layers = list(layers)
        if not layers or not all(isinstance(l, SparseLinear) for l in layers):
            raise TypeError("layers must be a non-empty list of SparseLinear modules")
        self.layers = torch.nn.ModuleList(layers)

    def forward(self, x, residuals=None):
        """x: one tensor (..., in_features) that every layer reads, or a list with one tensor per layer (their
        leading shapes -- token counts -- may differ).  residuals: None, or a list with None or a tensor
        per layer.  Returns the list of outputs, (..., out_features) each."""
        n = len(self.layers)
        xs = [x] * n if isinstance(x, torch.Tensor) else list(x)
        res = [None] * n if residuals is None else list(residuals)
        if len(xs) != n or len(res) != n:
            raise ValueError(f"x and residuals must hold one item per layer ({n})")
        flat = [l._flatten(xi, ri) for l, xi, ri in zip(self.layers, xs, res)]
        if isinstance(x, torch.Tensor):  # one flattened x for every layer, not n copies of a strided one
            flat = [(lead, flat[0][1], r) for lead, _, r in flat]
        alone = len({id(l.plan) for l in self.layers}) != n
        if alone or any(l._wants_grad(x2, r) for l, (_, x2, r) in zip(self.layers, flat)):
            return [l(xi, ri) for l, xi, ri in zip(self.layers, xs, res)]
        entries, epis, outs = [], [], []
        for l, (lead, x2, r) in zip(self.layers, flat):
            out = torch.empty((x2.shape[0], l.out_features), dtype=x2.dtype, device=x2.device)
            bias = l.bias.detach() if isinstance(l.bias, torch.nn.Parameter) else l.bias
            entries.append((l.plan, 0, x2, out))
            epis.append({"bias": bias, "activation": l.activation, "residual": r})
            outs.append(out.reshape(lead + (l.out_features,)))
        LinearBatch(entries, epis).run()
        return outs
