"""GPU checks of the device-side value update of k_mfma_ks plans (Plan.set_values: gs_plan_set_values,
k_set_values) and of SparseLinear.sync_values on top of it.

The yardstick is a fresh plan: a plan uploaded with values v1 and updated to v2 on the device must give
the bits of a plan built from v2 and uploaded -- spmm at the plan's width, linear at 24 and 100 tokens,
every replica, a Batch built before the update -- since both then hold the same 16-bit words in the same
layout and run the same kernel.  v2 holds, besides random values, what the conversion can get wrong:
rounding ties in both directions, results in the subnormal range, the largest finite value and a value
that rounds to it, both zeros, and one value that overflows to Inf.  B and x are small integers."""
import contextlib
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import generalsparse_amd as gsa  # noqa: E402
from guarded import assert_bits  # noqa: E402
from test_gpu_edges import DEV, TORCH_DT, int_B_cpu  # noqa: E402
from test_gpu_edges_mfma import mfma_everywhere  # noqa: E402,F401  (fixture)
from test_set_values_host import EVEN_K, pattern  # noqa: E402

pytestmark = pytest.mark.gpu

N = 32
SHAPES = [(40, 120), (40, 131), (1176, 120), (1176, 131), (EVEN_K, 120)]  # test_set_values_host.py's
VARIANTS = [(dt, head, wpos, split) for dt in ("f16", "bf16") for head in (0, 1) for wpos in ((0, 1) if dt == "f16" else (0,))
            for split in (0, 2)]


@contextlib.contextmanager
def config(over):
    old = {k: gsa.get_config(k) for k in over}
    try:
        for k, v in over.items():
            gsa.set_config(k, v)
        yield
    finally:
        for k, v in old.items():
            gsa.set_config(k, v)


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# what the conversion can get wrong, per dtype: (value, the 16-bit word it must become)
EDGES = {
    "f16": [(1 + 2.0 ** -11, 0x3C00), (1 + 3 * 2.0 ** -11, 0x3C02), (-(1 + 2.0 ** -11), 0xBC00),  # ties, down and up
            (np.nextafter(np.float32(1 + 2.0 ** -11), np.float32(2)), 0x3C01),                    # just past a tie
            (3 * 2.0 ** -24, 0x0003), (2.0 ** -25, 0x0000), (3 * 2.0 ** -25, 0x0002), (-2.0 ** -24, 0x8001),  # subnormal results
            (2.0 ** -14, 0x0400), (1023.5 * 2.0 ** -24, 0x0400),                                  # ... up to the smallest normal
            (65504.0, 0x7BFF), (65519.0, 0x7BFF), (-65504.0, 0xFBFF),                            # the largest finite value
            (0.0, 0x0000), (-0.0, 0x8000)],
    "bf16": [(1 + 2.0 ** -8, 0x3F80), (1 + 3 * 2.0 ** -8, 0x3F82), (-(1 + 2.0 ** -8), 0xBF80),
             (np.nextafter(np.float32(1 + 2.0 ** -8), np.float32(2)), 0x3F81),
             (f32(0x00030000), 0x0003), (f32(0x00008000), 0x0000), (f32(0x00018000), 0x0002), (f32(0x80010000), 0x8001),
             (f32(0x00800000), 0x0080), (f32(0x007FFF00), 0x0080),
             (f32(0x7F7F0000), 0x7F7F), (f32(0x7F7F7FFF), 0x7F7F), (f32(0xFF7F0000), 0xFF7F),
             (0.0, 0x0000), (-0.0, 0x8000)],
}
OVERFLOW = {"f16": (65520.0, 0x7C00), "bf16": (f32(0x7F7F8000), 0x7F80)}  # the tie above the largest finite value: Inf


@functools.lru_cache(maxsize=None)
def case(K, M, dtype):
    """(row, col, v1, v2, inf_at): v2 = random values with EDGES spread over them and OVERFLOW[dtype] at entry
    inf_at; the words v2 must become are asserted here, against the host conversion, once"""
    row, col, v1, v2 = pattern(K, M)
    v2 = v2.copy()
    rng = np.random.default_rng(K + M)
    at = rng.choice(len(v2), len(EDGES[dtype]) + 1, replace=False)
    want = []
    for i, (v, w) in zip(at, EDGES[dtype] + [OVERFLOW[dtype]]):
        v2[i] = v
        want.append(w)
    np.testing.assert_array_equal(gsa.convert_values(v2, dtype)[at], np.array(want, np.uint16))
    for a in (v1, v2):
        a.setflags(write=False)
    return row, col, v1, v2, int(at[-1])


@functools.lru_cache(maxsize=None)
def operands(K, M, dtype, inf_col):
    """integer B (K x N) whose column 0 is one-hot at row inf_col, and integer x for 24 and 100 tokens"""
    B = int_B_cpu(K, N, dtype, seed=3).clone()
    B[:, 0] = 0
    B[inf_col, 0] = 1
    g = torch.Generator()
    g.manual_seed(K + M)
    xs = {n: torch.randint(-2, 3, (n, K), generator=g).to(TORCH_DT[dtype]) for n in (24, 100)}
    return B, xs


def dev(v):
    """a (read-only, cached) numpy array as a device tensor"""
    return torch.from_numpy(v.copy()).to(DEV)


def plan_of(M, K, row, col, val, dtype, over, upload=True):
    with config(over):
        plan = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", N, 40, 1).compile()
        return plan.upload(dtype, 0) if upload else plan


def same(got, want, what, skip_row=None):
    """bit for bit; skip_row: the row that holds the Inf entry is left out (Inf times an integer of B is Inf or NaN)"""
    if skip_row is not None:
        keep = torch.ones(got.shape[0], dtype=torch.bool, device=got.device)
        keep[skip_row] = False
        got, want = got[keep].contiguous(), want[keep].contiguous()
    assert_bits(got, want, what)


@pytest.mark.parametrize("dtype,head,wpos,split", VARIANTS)
@pytest.mark.parametrize("K,M", SHAPES)
def test_update_equals_fresh_upload(K, M, dtype, head, wpos, split, mfma_everywhere):
    over = {"KS_HEAD": head, "KS_WPOS": wpos, "KS_SPLIT": split}
    row, col, v1, v2, inf_at = case(K, M, dtype)
    r_inf, c_inf = int(row[inf_at]), int(col[inf_at])
    B_cpu, xs = operands(K, M, dtype, c_inf)
    B = B_cpu.to(DEV)
    A, F = plan_of(M, K, row, col, v1, dtype, over), plan_of(M, K, row, col, v2, dtype, over)
    info = A.info()
    assert info["device_kernel"] == "k_mfma_ks" and info["ks_wpos"] == wpos and info["value_map_bytes"] == 0, info
    if K == EVEN_K and split:  # (the even pattern with two K ranges: the shape whose head steps the upload keeps)
        assert (info["ks_head_groups"] > 0) == bool(head), info
    if split:
        assert info["ksplit"] == 2, info
    what = f"{dtype} K={K} M={M} {over}"
    with config(over):  # (the map is built under the config the plan was uploaded under)
        A.set_values(dev(v2))
    A.device_status()
    info = A.info()
    with config(over):
        n_slots = len(F.value_sources(dtype)[0])
    assert info["host_values_stale"] == 1 and info["value_map_bytes"] == 4 * n_slots, info  # 4 bytes per slot, once
    want = F.spmm(B)
    got = A.spmm(B)
    torch.cuda.synchronize()
    inf = torch.tensor(float("inf"), dtype=got.dtype, device=DEV)
    assert got[r_inf, 0] == inf and want[r_inf, 0] == inf, (got[r_inf, 0], want[r_inf, 0])
    same(got, want, "spmm after set_values " + what, skip_row=r_inf)
    fused = A.linear_fused(24) == 1
    assert fused == (not wpos)
    if not fused:
        # (the three launches at another width need the CSR, which is built from the host values)
        with pytest.raises(gsa.GsError, match="stale"):
            A.linear(xs[24].to(DEV))
        with config(over):
            A.set_values(dev(v2), host=True)
    for n, x in xs.items():
        x = x.to(DEV)
        got, want = A.linear(x), F.linear(x)
        torch.cuda.synchronize()
        # (token-major: the Inf entry's output feature is column r_inf)
        keep = torch.ones(M, dtype=torch.bool, device=DEV)
        keep[r_inf] = False
        assert_bits(got[:, keep].contiguous(), want[:, keep].contiguous(), f"linear n={n} after set_values " + what)
    A.device_status()
    A.free(), F.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_trailing_empty_rows(dtype, mfma_everywhere):
    """a weight whose last output features are pruned away whole: the plan has fewer rows than the matrix"""
    K, M = 1176, 120
    row, col, v1, v2, inf_at = case(K, M, dtype)
    B = operands(K, M, dtype, int(col[inf_at]))[0].to(DEV)
    A, F = plan_of(M + 11, K, row, col, v1, dtype, {}), plan_of(M + 11, K, row, col, v2, dtype, {})
    assert A.info()["rows"] == M + 11 and A.info()["device_kernel"] == "k_mfma_ks", A.info()
    A.set_values(dev(v2))
    got, want = A.spmm(B), F.spmm(B)
    A.device_status()
    same(got, want, f"{dtype} trailing empty rows", skip_row=int(row[inf_at]))
    assert not got[M:].any()
    A.free(), F.free()


def test_update_under_another_config_is_refused(mfma_everywhere):
    """the map must be the uploaded layout's: a config that changed since the upload is noticed, nothing is launched"""
    K, M, dtype = EVEN_K, 120, "f16"
    row, col, v1, v2, _ = case(K, M, dtype)
    B = operands(K, M, dtype, 0)[0].to(DEV)
    A = plan_of(M, K, row, col, v1, dtype, {"KS_HEAD": 1, "KS_SPLIT": 2})
    before = A.spmm(B)
    with config({"KS_HEAD": 0, "KS_SPLIT": 2}):
        with pytest.raises(gsa.GsError, match="config changed"):
            A.set_values(dev(v2))
    assert A.info()["host_values_stale"] == 0 and A.info()["value_map_bytes"] == 0
    assert_bits(A.spmm(B), before, "a refused update leaves the plan as it was")
    A.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_replicas_and_batch(dtype, mfma_everywhere):
    """add_replica() before the update: both replicas give the new result; a grouped Batch with epilogues built
    before the update gives it too, on the same arrays; a replica added after the update holds the new values"""
    K, M = 1176, 131
    over = {"KS_SPLIT": 2}
    row, col, v1, v2, inf_at = case(K, M, dtype)
    r_inf = int(row[inf_at])
    B = operands(K, M, dtype, int(col[inf_at]))[0].to(DEV)
    A, F = plan_of(M, K, row, col, v1, dtype, over), plan_of(M, K, row, col, v2, dtype, over)
    A.add_replica()
    F.add_replica()
    bias = torch.arange(M, dtype=torch.float32, device=DEV) - 60
    eps = [{"alpha": 0.5, "bias": bias, "activation": "relu"}, None]
    outs = [[torch.zeros(M, N, dtype=TORCH_DT[dtype], device=DEV) for _ in range(2)] for _ in range(2)]
    bat_A = gsa.Batch([(A, i, B, outs[0][i]) for i in range(2)], N, epilogues=eps)
    bat_F = gsa.Batch([(F, i, B, outs[1][i]) for i in range(2)], N, epilogues=eps)
    assert sum(bat_A.launches()) == 2 and (dtype != "f16" or bat_A.launches() == [2]), bat_A.launches()
    s = torch.cuda.current_stream().cuda_stream
    bat_A.run(s)  # once on the old values
    torch.cuda.synchronize()
    old = [o.clone() for o in outs[0]]
    with config(over):
        A.values_prepare()
        assert A.info()["value_map_bytes"] > 0 and A.info()["host_values_stale"] == 0
        A.values_prepare()  # a second call does nothing
        A.set_values(dev(v2))
    for rep in range(2):
        same(A.spmm(B, replica=rep), F.spmm(B, replica=rep), f"{dtype} replica {rep}", skip_row=r_inf)
    bat_A.run(s)
    bat_F.run(s)
    torch.cuda.synchronize()
    for i in range(2):
        same(outs[0][i], outs[1][i], f"{dtype} Batch entry {i} after the update", skip_row=r_inf)
        assert not torch.equal(outs[0][i].view(torch.int16), old[i].view(torch.int16))
    A.add_replica()
    same(A.spmm(B, replica=2), F.spmm(B), f"{dtype} a replica added after the update", skip_row=r_inf)
    A.device_status()
    A.free(), F.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_stale_rule(dtype, tmp_path, mfma_everywhere):
    K, M = 1176, 120
    row, col, v1, v2, inf_at = case(K, M, dtype)
    r_inf = int(row[inf_at])
    B8 = int_B_cpu(K, 8, dtype, seed=4).to(DEV)
    A, F = plan_of(M, K, row, col, v1, dtype, {}), plan_of(M, K, row, col, v2, dtype, {})
    np.testing.assert_array_equal(A.values(), v1)
    A.set_values(dev(v2))
    assert A.info()["host_values_stale"] == 1
    pr, pc = A.pattern()  # asks for no values: legal
    np.testing.assert_array_equal(pr, row)
    np.testing.assert_array_equal(pc, col)
    with pytest.raises(gsa.GsError, match="stale"):
        A.values()
    with pytest.raises(gsa.GsError, match="stale"):
        A.save(tmp_path / "stale.gsplan")
    assert not (tmp_path / "stale.gsplan").exists()
    with pytest.raises(gsa.GsError, match="stale"):
        A.fp8_layout()
    C = torch.full((M, 8), 7.0, dtype=TORCH_DT[dtype], device=DEV)
    with pytest.raises(gsa.GsError, match="stale"):
        A.spmm(B8, C=C)  # N = 8: the gather fallback on the deferred CSR
    torch.cuda.synchronize()
    assert (C == 7.0).all(), "the refused spmm wrote C"
    A.add_replica()  # copies device arrays: legal
    A.set_values(dev(v2), host=True)
    assert A.info()["host_values_stale"] == 0
    np.testing.assert_array_equal(A.values().view(np.uint32), v2.view(np.uint32))
    A.save(tmp_path / "fresh.gsplan")
    L = gsa.Plan.load(tmp_path / "fresh.gsplan")
    np.testing.assert_array_equal(L.values().view(np.uint32), v2.view(np.uint32))
    same(A.spmm(B8), F.spmm(B8), f"{dtype} N=8 after the host refresh", skip_row=r_inf)
    # the CSR is resident now: a further update is refused, with nothing launched
    with pytest.raises(gsa.GsError, match="CSR"):
        A.set_values(dev(v1))
    assert A.info()["host_values_stale"] == 0
    # a host array: a host refresh and a device update in one (on a plan without the CSR)
    G = plan_of(M, K, row, col, v1, dtype, {})
    G.set_values(v2)
    assert G.info()["host_values_stale"] == 0
    np.testing.assert_array_equal(G.values().view(np.uint32), v2.view(np.uint32))
    B = int_B_cpu(K, N, dtype, seed=3).to(DEV)
    same(G.spmm(B), F.spmm(B), f"{dtype} set_values of a numpy array", skip_row=r_inf)
    same(G.spmm(B8), F.spmm(B8), f"{dtype} N=8 after set_values of a numpy array", skip_row=r_inf)
    # an upload uses the host values and clears the flag: after a device-only update that brings the old ones back
    H = plan_of(M, K, row, col, v1, dtype, {})
    H.set_values(dev(v2))
    H.upload(dtype, 0)
    assert H.info()["host_values_stale"] == 0 and H.info()["value_map_bytes"] == 0
    O = plan_of(M, K, row, col, v1, dtype, {})
    same(H.spmm(B), O.spmm(B), f"{dtype} re-upload after a device-only update")
    for p in (A, F, G, H, O, L):
        p.device_status()
        p.free()


def test_refusals_launch_nothing(mfma_everywhere):
    K, M = 40, 120
    row, col, v1, v2, _ = case(K, M, "f16")
    dv2 = dev(v2)
    B = int_B_cpu(K, N, "f16", seed=3).to(DEV)
    # an f32 plan (a gather family)
    P = plan_of(M, K, row, col, v1, "f32", {})
    with pytest.raises(gsa.GsError, match="f16 and bf16"):
        P.set_values(dv2)
    with pytest.raises(gsa.GsError, match="f16 and bf16"):
        P.values_prepare()
    P.free()
    # FP8 weights
    P = gsa.Plan.from_coo(M, K, row, col, v1).run_pipeline("block_total", N, 40, 1).compile().upload("f16", 0, weights="fp8")
    with pytest.raises(gsa.GsError, match="FP8"):
        P.set_values(dv2)
    P.free()
    # a plan off k_mfma_ks
    P = gsa.Plan.from_coo(M, K, row, col, v1).run_pipeline("warp_segment", N, 4, 1).compile().upload("f16", 0)
    with pytest.raises(gsa.GsError, match="k_mfma_ks"):
        P.set_values(dv2)
    P.free()
    # a plan that is not on the device
    P = plan_of(M, K, row, col, v1, "f16", {}, upload=False)
    with pytest.raises(gsa.GsError, match="not on the device"):
        P.set_values(dv2)
    P.free()
    # a plan that ran at N = 8: its CSR is resident
    P = plan_of(M, K, row, col, v1, "f16", {})
    before = P.spmm(B).clone()
    P.spmm(int_B_cpu(K, 8, "f16", seed=4).to(DEV))
    with pytest.raises(gsa.GsError, match="CSR"):
        P.set_values(dv2)
    P.free()
    # the values: length, dtype, shape, contiguity, device
    P = plan_of(M, K, row, col, v1, "f16", {})
    bad = [dv2[:-1], torch.cat([dv2, dv2[:1]]), dv2.double(), dv2.half(), dv2.reshape(1, -1), torch.cat([dv2, dv2])[::2],
           v2[:-1], v2.astype(np.float64), torch.from_numpy(v2.copy()).double()]
    if torch.cuda.device_count() > 1:
        bad.append(dv2.to("cuda:1"))
    for values in bad:
        with pytest.raises((ValueError, TypeError)):
            P.set_values(values)
    info = P.info()
    assert info["host_values_stale"] == 0 and info["value_map_bytes"] == 0, info
    assert_bits(P.spmm(B), before, "refused updates leave the plan as it was")
    np.testing.assert_array_equal(P.values(), v1)
    P.device_status()
    P.free()


def sgd_steps(layer, twin, x64, gy64, td, steps, host, what):
    """`steps` SGD steps on both layers, layer synced on the device and twin by the host rebuild: after each,
    y and x.grad of the two have the same bits"""
    opts = [torch.optim.SGD(l.parameters(), lr=2.0 ** -7) for l in (layer, twin)]
    for step in range(steps):
        res = []
        for l, opt in zip((layer, twin), opts):
            x = torch.from_numpy(x64).to(DEV, td).requires_grad_(True)
            opt.zero_grad()
            y = l(x)
            y.backward(torch.from_numpy(gy64).to(DEV, td))
            opt.step()
            res.append((y.detach(), x.grad))
        assert_bits(res[0][0], res[1][0], f"{what} y in step {step}")
        assert_bits(res[0][1], res[1][1], f"{what} x.grad in step {step}")
        assert torch.equal(layer.values.detach().view(torch.int32), twin.values.detach().view(torch.int32))
        layer.sync_values(host=host)
        twin.sync_values(rebuild=True)
    x = torch.from_numpy(x64).to(DEV, td).requires_grad_(True)
    ys = [l(x) for l in (layer, twin)]
    assert_bits(ys[0].detach(), ys[1].detach(), f"{what} y after the last sync")
    # the values have moved off the integers they started from, and the forward follows them
    assert (layer.values.detach() != layer.values.detach().round()).any()


def make_layers(K, M, dtype):
    from test_gpu_linear_backward import operands as lin_operands, weight
    W = weight(K, M)[0]
    x64, bias, _, gy64 = lin_operands(K, M, 24)
    # (gradients scaled to non-integers, so that the updated values meet the rounding of the plan's dtype)
    mk = lambda: gsa.SparseLinear.from_dense(torch.from_numpy(W), torch.from_numpy(bias), dtype=dtype, grad="all")  # noqa: E731
    return mk(), mk(), x64, gy64 * 0.37


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K", [40, 1176])
def test_sparse_linear_sync_on_the_device(K, dtype, host, mfma_everywhere):
    M, td = 120, TORCH_DT[dtype]
    layer, twin, x64, gy64 = make_layers(K, M, dtype)
    layer.prepare_backward()
    twin.prepare_backward()
    plan, plan_T = layer.plan, layer.plan_T
    assert plan.info()["device_kernel"] == "k_mfma_ks" and plan_T.info()["device_kernel"] == "k_mfma_ks"
    assert plan.info()["value_map_bytes"] > 0 and plan_T.info()["value_map_bytes"] > 0  # prepare_backward uploaded the maps
    ptrs = (plan._h.value, plan_T._h.value)
    sgd_steps(layer, twin, x64, gy64, td, 3, host, f"{dtype} K={K} M={M} host={host}")
    assert layer.plan is plan and layer.plan_T is plan_T and (plan._h.value, plan_T._h.value) == ptrs
    assert plan.info()["host_values_stale"] == (0 if host else 1)
    if host:
        np.testing.assert_array_equal(plan.values().view(np.uint32), layer.values.detach().cpu().numpy().view(np.uint32))
    else:
        with pytest.raises(gsa.GsError, match="stale"):
            plan.values()
    plan.device_status(), plan_T.device_status()
    for l in (layer, twin):
        l.plan.free(), l.plan_T.free()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("K", [40, 1176])
def test_sparse_linear_sync_falls_back_per_plan(K, dtype, mfma_everywhere):
    """M = 131: plan_T (131 input features, not a multiple of 8) runs the three launches and then holds its CSR:
    sync_values rebuilds it on the host, while the forward plan is updated in place"""
    M, td = 131, TORCH_DT[dtype]
    layer, twin, x64, gy64 = make_layers(K, M, dtype)
    layer.prepare_backward()
    twin.prepare_backward()
    plan, plan_T = layer.plan, layer.plan_T
    assert plan_T.linear_fused(24) == 0
    sgd_steps(layer, twin, x64, gy64, td, 2, True, f"{dtype} K={K} M={M}")
    assert layer.plan is plan and layer.plan_T is not plan_T
    for l in (layer, twin):
        l.plan.free(), l.plan_T.free()
    plan_T.free()


def test_sync_values_of_a_wrapped_plan(mfma_everywhere):
    """a layer around an uploaded plan has no build recipe: the device path needs none, the rebuild refuses"""
    K, M, dtype = 40, 120, "f16"
    row, col, v1, v2, _ = case(K, M, dtype)
    plan = plan_of(M, K, row, col, v1, dtype, {})
    layer = gsa.SparseLinear(plan, grad="all")
    x = operands(K, M, dtype, 0)[1][24].to(DEV)
    with torch.no_grad():
        layer.values.copy_(dev(v2))
    layer.sync_values(host=False)
    F = plan_of(M, K, row, col, v2, dtype, {})
    assert layer.plan is plan
    assert_bits(layer(x), F.linear(x), "a wrapped plan after sync_values")
    with pytest.raises(RuntimeError, match="from_dense"):
        layer.sync_values(rebuild=True)
    with pytest.raises(RuntimeError, match="grad='all'"):
        gsa.SparseLinear(F, grad="input").sync_values()
    plan.free(), F.free()
