"""GPU checks of the grouped token-major linear (LinearBatch / gs_linear_batch, k_mfma_ks_tm_group): several
Plan.linear calls -- their own plans, operands and token counts -- as one call, consecutive single-launch
k_mfma_ks_tm entries of one instantiation as ONE grid, everything else through Plan.linear's own path.

The matrix is the 131-row pattern of tests/test_gpu_edges_mfma.py (40-row blocks of 40 / 40 / 40 / 11 rows, three
row tiles) with the integer operands of tests/test_gpu_linear.py, so every comparison is bit for bit: an entry's
Y against its own Plan.linear output and against epilogue_ref on the exact product (alpha, bias, ReLU and the
residual).  X, Y and the residual are guarded (tests/guarded.py); every run is repeated into the NaN-refilled Y;
device_status() must be clean on every plan.  launches() is asserted, never assumed."""
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits, assert_guards_intact, guarded_B, guarded_C  # noqa: E402
from test_gpu_edges import DEV, PIPE_PARAMS, EDGE_K, TORCH_DT, build, edge_dense, edge_matrix, int_B_cpu  # noqa: E402
from test_gpu_edges_mfma import KS_M, ks_case, ks_pattern, ks_ranges, mfma_everywhere  # noqa: E402,F401  (fixture)
from test_gpu_epilogue import config, epilogue_ref  # noqa: E402
from test_gpu_fp8 import fp8_plan  # noqa: E402
from test_gpu_linear import full_epilogue, ks_operands, ks_plan  # noqa: E402
from test_gpu_linear_tokens import misaligned_B, ws_kb_for  # noqa: E402

pytestmark = pytest.mark.gpu

W = 32  # the width every k_mfma_ks plan here is built for


def tiles(n):
    return (n + 31) // 32


class Entry:
    """one entry of a batch on guarded operands: X (or a tensor given), Y, the full epilogue with a guarded
    residual, the integer reference and -- single=True -- the bits of the entry's own Plan.linear call"""

    def __init__(self, plan, X_cpu, prod, dtype, replica=0, fused=True, x=None, single=True):
        M, n = prod.shape
        self.plan, self.replica, self.n = plan, replica, n
        epi = full_epilogue(M, n, dtype)
        self.ref = epilogue_ref(prod, dtype, fused, **epi).t().contiguous().to(DEV)
        self.hx = None
        self.x = x
        if x is None:
            self.x, self.hx = guarded_B(X_cpu, DEV)
        self.y, self.hy = guarded_C(n, M, TORCH_DT[dtype], DEV)
        res, self.hr = guarded_B(epi["residual"].t().contiguous(), DEV)
        self.kw = dict(alpha=epi["alpha"], bias=epi["bias"].to(DEV), activation=epi["activation"], residual=res)
        self.single = None
        if single:
            self.single = plan.linear(self.x, replica=replica, **self.kw).clone()
            torch.cuda.synchronize()
            plan.device_status()
            assert_bits(self.single, self.ref, "the entry's own Plan.linear against the reference")

    def check(self, what):
        self.plan.device_status()
        if self.single is not None:
            assert_bits(self.y, self.single, what + ": against its own Plan.linear")
        assert_bits(self.y, self.ref, what + ": against the reference")
        assert_guards_intact(self.hy, what + " Y")
        assert_guards_intact(self.hr, what + " residual")
        if self.hx is not None:
            assert_guards_intact(self.hx, what + " X")


def ks_entry(plan, K, n, dtype, **kw):
    X, prod = ks_operands(K, n, dtype)
    return Entry(plan, X, prod, dtype, **kw)


def run_batch(entries, want, what, runs=2):
    b = gsa.LinearBatch([(e.plan, e.replica, e.x, e.y) for e in entries], [e.kw for e in entries])
    assert b.launches() == want, (what, b.launches())
    for again in range(runs):
        b.run()
        torch.cuda.synchronize()
        for i, e in enumerate(entries):
            e.check(f"{what} entry {i} (n={e.n}) run {again}")
            e.hy.refill()
    return b


def check_ks(plan, K, split):
    info = plan.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ksplit"] == ks_ranges(K, split), info


# ------------------------------------------------------------------ 1: the same bits as the single calls
# (KS_SPLIT, K, tokens) per entry: K = 40 and 1176 / 1184, one to three K ranges and one to three token tiles
# inside ONE launch -- with and without K-split state of their own (n > 32 on a plan with K ranges)
GROUPS = [
    [(1, 40, 7), (2, 40, 33), (3, 1176, 72)],
    [(3, 1176, 1), (2, 1184, 32)],
    [(2, 1184, 72), (1, 40, 32), (2, 40, 7)],
]


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("group", GROUPS, ids=lambda g: "-".join(f"s{s}k{k}n{n}" for s, k, n in g))
def test_same_bits_as_single_calls(group, dtype, mfma_everywhere):
    entries = []
    for split, K, n in group:
        plan = ks_plan(K, W, dtype, split)
        check_ks(plan, K, split)
        assert plan.linear_launches(n) == [tiles(n)]
        entries.append(ks_entry(plan, K, n, dtype))
    run_batch(entries, [len(group)], f"{dtype} {group}")
    for e in entries:
        e.plan.free()


# ------------------------------------------------------------------ 2: one x for three plans
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_shared_x(dtype, mfma_everywhere):
    """three plans of one K (one, two and three K ranges) read the same X tensor, 33 tokens"""
    K, n = 1184, 33
    X_cpu, prod = ks_operands(K, n, dtype)
    x, hx = guarded_B(X_cpu, DEV)
    entries = []
    for split in (1, 2, 3):
        plan = ks_plan(K, W, dtype, split)
        check_ks(plan, K, split)
        entries.append(Entry(plan, X_cpu, prod, dtype, x=x))
    assert len({e.x.data_ptr() for e in entries}) == 1
    run_batch(entries, [3], f"shared x {dtype}")
    assert_guards_intact(hx, "the shared X")
    for e in entries:
        e.plan.free()


# ------------------------------------------------------------------ 3: the cap
def test_the_cap_splits_a_run(mfma_everywhere):
    """one more distinct plan than a launch carries: [cap, 1], every output exact"""
    K, dtype, cap = 40, "f16", gsa.linear_group_max()
    assert cap == 32
    X_cpu, prod = ks_operands(K, 7, dtype)
    x, hx = guarded_B(X_cpu, DEV)
    entries = [Entry(ks_plan(K, W, dtype, 1), X_cpu, prod, dtype, x=x, single=i in (0, cap - 1, cap)) for i in range(cap + 1)]
    run_batch(entries, [cap, 1], "cap + 1 entries", runs=1)
    assert_guards_intact(hx, "the shared X")
    for e in entries:
        e.plan.free()


# ------------------------------------------------------------------ 4: splitting and fallbacks inside one batch
def test_a_repeated_replica_splits_and_a_second_replica_joins(mfma_everywhere):
    K, n, dtype, split = 1176, 40, "f16", 3
    plan = ks_plan(K, W, dtype, split)
    check_ks(plan, K, split)
    plan.add_replica()
    a, b = ks_entry(plan, K, n, dtype), ks_entry(plan, K, 7, dtype)
    run_batch([a, b], [1, 1], "one (plan, replica) twice")
    c = ks_entry(plan, K, 72, dtype, replica=1)
    run_batch([a, c], [2], "two replicas of one plan")
    run_batch([a, c, b], [2, 1], "two replicas, then replica 0 again")
    plan.free()


def test_f16_and_bf16_never_share_a_launch(mfma_everywhere):
    K, n = 40, 33
    ps = [ks_plan(K, W, dt, 2) for dt in ("f16", "bf16", "bf16")]
    entries = [ks_entry(p, K, n, dt) for p, dt in zip(ps, ("f16", "bf16", "bf16"))]
    run_batch(entries, [1, 2], "f16 next to bf16")
    for p in ps:
        p.free()


def test_fallbacks_run_alone_and_exact(mfma_everywhere):
    """what k_mfma_ks_tm_group does not run goes through Plan.linear's path inside the batch, between grouped
    neighbours: FP8 weights (k_mfma_ks_tm's VB = 8 form), a gather-family plan and a misaligned x (three
    launches each: the reference that rounds twice), a call LINEAR_WS_KB splits"""
    dtype, K = "f16", 40
    row, col, val, _ = ks_pattern(K)
    ks = [ks_plan(K, W, dtype, s) for s in (1, 2, 1, 2)]
    # FP8 weights between two groupable entries
    f8 = fp8_plan(KS_M, K, row, col, val, W, 1)
    assert f8.info()["weights"] == 1 and f8.linear_fused(W) == 1
    entries = [ks_entry(ks[0], K, 32, dtype), ks_entry(f8, K, 32, dtype), ks_entry(ks[1], K, 7, dtype), ks_entry(ks[2], K, 33, dtype)]
    run_batch(entries, [1, 1, 2], "an FP8-weight plan")
    # a gather-family plan
    p0, p1 = PIPE_PARAMS["warp_total"]
    M, GK, grow, gcol, gval, long_rows = edge_matrix("warp_total")
    n = 5
    gplan = build(M, GK, grow, gcol, gval, "warp_total", p0, p1, n, dtype, over={"MFMA_TILES": 0})
    assert gplan.linear_fused(n) == 0
    B = int_B_cpu(EDGE_K, n, dtype)
    gather = Entry(gplan, B.t().contiguous(), (edge_dense(long_rows) @ B.double().numpy())[:M], dtype, fused=False)
    run_batch([entries[0], entries[2], gather, entries[3]], [2, 1, 1], "a gather-family plan")
    # a misaligned x on a plan the kernel covers
    X_cpu, prod = ks_operands(K, 33, dtype)
    xm, flat = misaligned_B(X_cpu, DEV)
    mis = Entry(ks[3], X_cpu, prod, dtype, fused=False, x=xm)
    run_batch([entries[0], mis, entries[2], entries[3]], [1, 1, 2], "a misaligned x")
    assert bool(torch.isnan(flat[:16]).all()) and bool(torch.isnan(flat[-16:]).all())
    # a call the state budget splits into two launches stays on its own path
    K3, n3 = 1176, 100
    p3 = ks_plan(K3, W, dtype, 3)
    check_ks(p3, K3, 3)
    tile_bytes = 4 * 3 * 3 * 2048 + 4 * 4
    with config(LINEAR_WS_KB=ws_kb_for(tile_bytes, 2)):
        assert p3.linear_launches(n3) == [2, 2]
        big = ks_entry(p3, K3, n3, dtype)
        run_batch([big, entries[0], entries[2]], [1, 2], "a call LINEAR_WS_KB splits")
    assert p3.linear_launches(n3) == [4]
    run_batch([big, entries[0], entries[2]], [3], "the same call under the default budget")
    for p in ks + [f8, gplan, p3]:
        p.free()


# ------------------------------------------------------------------ 5: state in turn on one replica
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_tile_counts_in_turn_through_the_grouped_path(dtype, mfma_everywhere):
    """three K ranges: the arrival counters' epochs and the slabs' tags are laid out by the tile count, and
    the grouped launch, the single launch and the plan's SpMM at N = 32 take turns on one replica's state --
    4, 2, 1 and 3 tiles, each change of layout from cleared state, one tile on the upload's own"""
    split, K = 3, 1176
    plan, mate = ks_plan(K, W, dtype, split), ks_plan(40, W, dtype, 2)
    check_ks(plan, K, split)
    B32, ref32 = ks_case(K, 32, dtype)
    by_n = {n: ks_entry(plan, K, n, dtype, single=False) for n in (100, 40, 32, 72)}
    other = ks_entry(mate, 40, 33, dtype)
    for step, (how, n) in enumerate([("batch", 100), ("single", 40), ("batch", 40), ("batch", 32), ("spmm", 32), ("batch", 72),
                                     ("single", 100), ("batch", 72), ("spmm", 32), ("batch", 100), ("batch", 32)]):
        what = f"step {step}: {how} n={n} {dtype}"
        if how == "batch":
            run_batch([other, by_n[n]], [2], what)
        elif how == "single":
            e = by_n[n]
            plan.linear(e.x, out=e.y, **e.kw)
            torch.cuda.synchronize()
            e.check(what)
            e.hy.refill()
        else:
            c = plan.spmm(B32.to(DEV))
            torch.cuda.synchronize()
            plan.device_status()
            assert_bits(c, ref32.to(DEV), what)
    plan.free()
    mate.free()


# ------------------------------------------------------------------ 6: refusals
def test_refusals_leave_every_out_untouched(mfma_everywhere):
    K, n, dtype = 40, 33, "f16"
    X_cpu, _ = ks_operands(K, n, dtype)
    plans = [ks_plan(K, W, dtype, s) for s in (1, 2, 1)]
    x = X_cpu.to(DEV)
    big = [torch.full((n + 1, KS_M), float("nan"), dtype=torch.float16, device=DEV) for _ in plans]
    outs = [b[:n] for b in big]
    good = [(p, 0, x, o) for p, o in zip(plans, outs)]
    res = torch.zeros((n, KS_M), dtype=torch.float16, device=DEV)

    def with_entry(i, **kw):
        e = dict(zip(("plan", "replica", "x", "out"), good[i]))
        e.update(kw)
        return good[:i] + [(e["plan"], e["replica"], e["x"], e["out"])] + good[i + 1:]

    bad = [
        ("x dtype", TypeError, with_entry(1, x=x.float()), None),
        ("x shape", ValueError, with_entry(2, x=x.t().contiguous()), None),
        ("out shape", ValueError, with_entry(0, out=torch.full((KS_M, n), float("nan"), dtype=torch.float16, device=DEV)), None),
        ("replica out of range", ValueError, with_entry(1, replica=3), None),
        ("residual overlaps its out", ValueError, good, [None, {"residual": big[1][1:]}, None]),
        ("residual is its out", ValueError, good, [None, None, {"residual": outs[2]}]),
        ("activation", ValueError, good, [{"activation": "gelu"}, None, None]),
        ("epilogue key", ValueError, good, [None, {"beta": 1.0}, None]),
    ]
    for what, exc, entries, epis in bad:
        with pytest.raises(exc):
            gsa.LinearBatch(entries, epis).run()
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(b).all()) for b in big), what
    # the C ABI's own checks, every one before the first launch: the last entry's replica
    L = gsa.load_library()
    import ctypes
    arr = lambda t, v: (t * len(v))(*v)  # noqa: E731
    rc = L.gs_linear_batch(arr(ctypes.c_void_p, [p._h for p in plans]), arr(ctypes.c_int, [0, 0, 5]),
                           arr(ctypes.c_void_p, [x.data_ptr()] * 3), arr(ctypes.c_void_p, [o.data_ptr() for o in outs]),
                           arr(ctypes.c_int, [n] * 3), None, 3, None)
    torch.cuda.synchronize()
    assert rc == -1 and b"batch entry 2: bad replica" in L.gs_last_error(), L.gs_last_error()
    assert all(bool(torch.isnan(b).all()) for b in big)
    # and the accepted call still works on the same operands
    b = gsa.LinearBatch(good, [None, {"residual": res}, None])
    assert b.launches() == [3]
    b.run()
    torch.cuda.synchronize()
    for p, o, bg, kw in zip(plans, outs, big, ({}, {"residual": res}, {})):
        assert_bits(o, p.linear(x, **kw), "the accepted batch")
        assert bool(torch.isnan(bg[n]).all())
        p.free()


# ------------------------------------------------------------------ 7: the module
def three_layers(K, dtype, grad=None):
    layers = []
    for i in range(3):
        dense = ks_pattern(K, seed=i)[3]
        bias = torch.arange(KS_M, dtype=torch.float32) - 60.0 - i
        layers.append(gsa.SparseLinear.from_dense(torch.from_numpy(dense).float(), bias, tokens=W, dtype=dtype,
                                                  activation="relu" if i != 1 else None, grad=grad))
    return layers


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_sparse_linear_group(dtype, mfma_everywhere):
    """three from_dense layers: a shared (2, 16, K) input and per-layer inputs of 7, 33 and 72 tokens, with and
    without residuals, bit for bit the layers called one by one"""
    K = 1184
    layers = three_layers(K, dtype)
    group = gsa.SparseLinearGroup(layers)
    assert isinstance(group, torch.nn.Module) and len(group.layers) == 3
    shared = int_B_cpu(K, 32, dtype, seed=1).t().contiguous().reshape(2, 16, K).to(DEV)
    own = [int_B_cpu(K, n, dtype, seed=2 + i).t().contiguous().to(DEV) for i, n in enumerate((7, 33, 72))]
    res = [None, torch.ones((33, KS_M), dtype=TORCH_DT[dtype], device=DEV), None]
    with torch.no_grad():
        for what, xs, rs in (("shared x", shared, None), ("own x", own, None), ("own x, a residual", own, res)):
            want = [l(x, r) for l, x, r in zip(layers, [xs] * 3 if isinstance(xs, torch.Tensor) else xs, rs or [None] * 3)]
            got = group(xs, rs)
            torch.cuda.synchronize()
            assert len(got) == 3
            for i, (g, w) in enumerate(zip(got, want)):
                layers[i].plan.device_status()
                assert g.shape == w.shape and not bool(torch.isnan(g).any())
                assert_bits(g.contiguous(), w.contiguous(), f"SparseLinearGroup {what}, layer {i} {dtype}")
        entries = [(l.plan, 0, x, torch.empty((x.shape[0], KS_M), dtype=x.dtype, device=DEV)) for l, x in zip(layers, own)]
        assert gsa.LinearBatch(entries).launches() == [3]
        with pytest.raises(ValueError):
            group(own[:2])
    with pytest.raises(RuntimeError, match="inference"):
        group(shared.clone().requires_grad_())
    # layers that share a plan object would share replica 0: called one by one, the same bits
    twice = gsa.SparseLinearGroup([layers[0], layers[0]])
    with torch.no_grad():
        a, b = twice(own[:2])
        torch.cuda.synchronize()
        assert_bits(a, layers[0](own[0]), "a shared plan, entry 0")
        assert_bits(b, layers[0](own[1]), "a shared plan, entry 1")
    for l in layers:
        l.plan.free()


def test_sparse_linear_group_under_grad(mfma_everywhere):
    """grad="all" layers and an input that requires grad: the outputs and every gradient are those of the
    layers called one by one"""
    K, dtype, n = 1184, "f16", 40
    layers = three_layers(K, dtype, grad="all")
    group = gsa.SparseLinearGroup(layers)
    x0 = int_B_cpu(K, n, dtype, seed=5).t().contiguous().to(DEV)
    gy = [int_B_cpu(KS_M, n, dtype, seed=6 + i).t().contiguous().to(DEV) for i in range(3)]

    def run(f):
        x = x0.clone().requires_grad_()
        for l in layers:
            l.zero_grad(set_to_none=True)
        ys = f(x)
        torch.autograd.backward(ys, gy)
        torch.cuda.synchronize()
        return [y.detach() for y in ys], [x.grad] + [l.values.grad.clone() for l in layers] + [l.bias.grad.clone() for l in layers]

    ys_a, grads_a = run(lambda x: [l(x) for l in layers])
    ys_b, grads_b = run(group)
    assert len(grads_b) == 7
    for i, (a, b) in enumerate(zip(ys_a, ys_b)):
        assert_bits(b, a, f"output {i} under grad")
    for i, (a, b) in enumerate(zip(grads_a, grads_b)):
        assert a is not None and b is not None and bool(a.abs().sum() > 0)
        assert_bits(b.contiguous(), a.contiguous(), f"gradient {i}")
    for l in layers:
        l.plan.device_status()
        l.plan.free()
