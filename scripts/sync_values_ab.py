#!/usr/bin/env python3
"""What the device-side value update (Plan.set_values / gs_plan_set_values, k_set_values) buys a training step:
SparseLinear.sync_values() three ways on one pruned layer, and the kernel alone, timed in one process.

  a  device   sync_values(host=False): k_set_values on the plan and on plan_T (plus the gather of
              layer.values into plan_T's order), nothing leaves the GPU
  b  refresh  sync_values(): the same, plus the values copied to the CPU and both plans' host copies
              refreshed (the default: Plan.values(), save() and a launch at another width keep working)
  c  rebuild  sync_values(rebuild=True): both plans rebuilt on the host from COO and uploaded again
  k  kernel   gs_plan_set_values of a device tensor on the forward plan, called through ctypes: one
              k_set_values launch and next to no host work

The layer (f16, 32 tokens, seeded): 5120 x 5120 at 70% sparsity on block_total(40,1), grad="all", plan_T
built.  a, b and k are timed over `steps` calls, after a warm-up, in `rounds` alternating rounds, twice: between
two device events, and by the host clock around the calls and a device synchronise (a and b do Python and torch
work per call, so their wall time is what a training loop sees; b ends in host work); c by the host clock around
a call that ends in a device synchronise (it is seconds).  Back-to-back calls re-read one map, which the
Infinity Cache holds in part: k is the kernel at its best, not behind a training step's other traffic.
The bytes k_set_values moves are counted from the plan: 4 B of map and 2 B of values written per slot of the
value array, 4 B gathered per entry.  After each way the layer's output is compared, bit for bit, with that
of a twin layer built from the same values.
Written to profiles/sync_values_ab.json.

    python scripts/sync_values_ab.py [--rounds 5] [--steps 50] [--warmup 5] [--rebuilds 2] [--size 5120] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12  # bytes / s (spec; a float4 copy reaches 79% of it)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rebuilds", type=int, default=2)
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_values_ab.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import datasets as ds

    if not torch.cuda.is_available():
        raise SystemExit("sync_values_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    M = K = args.size
    N = 32

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    row, col, val = ds.pruned_weight(M, K, args.sparsity, 13)
    W = np.zeros((M, K), np.float32)
    W[row.astype(np.int64), col.astype(np.int64)] = val

    def build(values):
        w = W.copy()
        w[row.astype(np.int64), col.astype(np.int64)] = values
        t0 = time.perf_counter()
        layer = gsa.SparseLinear.from_dense(torch.from_numpy(w), tokens=N, dtype="f16", pipeline=("block_total", 40, 1),
                                            grad="all").prepare_backward()
        torch.cuda.synchronize(dev)
        return layer, time.perf_counter() - t0

    layer, t_build = build(val)
    info, info_T = layer.plan.info(), layer.plan_T.info()
    assert info["device_kernel"] == info_T["device_kernel"] == "k_mfma_ks", (info, info_T)
    assert info["value_map_bytes"] > 0 and info_T["value_map_bytes"] > 0  # (prepare_backward uploaded the maps)
    nnz = info["nnz"]
    slots = info["value_map_bytes"] // 4
    kernel_bytes = 4 * slots + 4 * nnz + 2 * slots
    say(f"layer {M} x {K}, {nnz} non-zeros, built with plan_T in {t_build:.1f} s; value array {slots} slots, "
        f"map {info['value_map_bytes']} B per plan, tile bytes {info['tile_bytes']}")

    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    x = torch.rand((N, K), device=dev, generator=gen).mul_(2).sub_(1).half()

    def step_values(i):
        """new values every call, as an optimizer step leaves them"""
        with torch.no_grad():
            layer.values.mul_(1.0 + 2.0 ** -10 * (1 + i % 3))

    def agrees(what):
        twin, _ = build(layer.values.detach().cpu().numpy())
        with torch.no_grad():
            same = bool((layer(x).view(torch.int16) == twin(x).view(torch.int16)).all())
        twin.plan.free(), twin.plan_T.free()
        assert same, what
        return same

    L, h = layer.plan._L, layer.plan._h
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def kernel():
        rc = L.gs_plan_set_values(h, ctypes.c_void_p(layer.values.data_ptr()), None, stream)
        assert rc == 0, rc

    ways = {"device": lambda: layer.sync_values(host=False), "refresh": lambda: layer.sync_values(), "kernel": kernel}
    same = {}
    for name, fn in ways.items():
        step_values(0)
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize(dev)
        if name != "kernel":
            same[name] = agrees(name)
    us = {k: [] for k in ways}
    wall_us = {k: [] for k in ways}
    for r in range(args.rounds):
        for name, fn in ways.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            e0.record()
            calls = max(1, args.steps // 10) if name == "refresh" else args.steps  # (tens of milliseconds each)
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize(dev)
            wall_us[name].append((time.perf_counter() - t0) / calls * 1e6)
            us[name].append(e0.elapsed_time(e1) / calls * 1e3)
        say(f"round {r}: " + ", ".join(f"{k} {us[k][-1]:.2f} us (wall {wall_us[k][-1]:.2f})" for k in ways))
    layer.sync_values()  # (host values current again: the rebuild below reads layer.values, but leave no stale plan)
    rebuild_s = []
    for i in range(args.rebuilds):
        step_values(i)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        layer.sync_values(rebuild=True)
        torch.cuda.synchronize(dev)
        rebuild_s.append(time.perf_counter() - t0)
        say(f"rebuild {i}: {rebuild_s[-1]:.2f} s")
    same["rebuild"] = agrees("rebuild")
    med = {k: statistics.median(v) for k, v in us.items()}
    wall = {k: statistics.median(v) for k, v in wall_us.items()}
    result = {
        "what": "SparseLinear.sync_values on one pruned layer three ways and k_set_values alone (scripts/sync_values_ab.py)",
        "device": torch.cuda.get_device_name(0), "layer": f"{M} x {K}, {args.sparsity:.0%} sparse, f16, block_total(40,1) at {N} tokens, plan_T built",
        "nnz": nnz, "value_slots": slots, "value_map_bytes_per_plan": info["value_map_bytes"], "tile_bytes": info["tile_bytes"],
        "rounds": args.rounds, "steps_per_round": args.steps, "refresh_steps_per_round": max(1, args.steps // 10), "warmup_calls": args.warmup,
        "unit": "us per call: device events around the round's calls; wall: the host clock around the calls and a synchronise",
        "us_rounds": {k: [round(x, 2) for x in v] for k, v in us.items()},
        "us_median": {k: round(v, 2) for k, v in med.items()},
        "wall_us_rounds": {k: [round(x, 2) for x in v] for k, v in wall_us.items()},
        "wall_us_median": {k: round(v, 2) for k, v in wall.items()},
        "rebuild_seconds": [round(x, 3) for x in rebuild_s],
        "rebuild_over_device_wall": round(statistics.median(rebuild_s) * 1e6 / wall["device"], 1),
        "kernel_bytes": {"map": 4 * slots, "gathered": 4 * nnz, "written": 2 * slots, "total": kernel_bytes},
        "kernel_bytes_per_s": round(kernel_bytes / (med["kernel"] * 1e-6), 0),
        "kernel_fraction_of_hbm_peak": round(kernel_bytes / (med["kernel"] * 1e-6) / HBM_PEAK, 4),
        "same_bits_as_a_fresh_layer": same,
    }
    layer.plan.device_status()
    layer.plan_T.device_status()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
