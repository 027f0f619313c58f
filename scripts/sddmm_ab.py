#!/usr/bin/env python3
"""What the backward pass costs on the flagship layer: k_sddmm_tm against torch's dense product and
gather, and SparseLinear(grad="all") forward + backward against a dense torch.nn.Linear.

Matrix: the 5120^2 70%-pruned stand-in (datasets.pruned_weight, seed 13), f16, block_total(40,1) built for
32 tokens.  Token counts n = 32, 256, 2048.

1. sddmm: Plan.sddmm(G, X) (one k_sddmm_tm launch) against (G.t() @ X)[row, col] in torch (a dense GEMM,
   then an indexed gather with int64 indices).  The engine's side rotates over `copies` plans of the
   pattern, each with its own G, X and out, sized past the Infinity Cache (--rotation-mb); torch's side
   rotates G, X and the dense product and shares the index tensors.  After the warm-up the two sides
   alternate, each round timing `steps` steps between two device events (scripts/linear_ab.py's
   discipline).  The byte model of a step: nnz x (4 + column bytes) + (M + 1) x 4 + n x (M + K) x 2, as a
   fraction of the HBM peak (--hbm-tbs) at the median.
2. layer: SparseLinear.from_dense(W, bias, grad="all") and torch.nn.Linear(K, M) in f16, forward +
   backward (x, the weight's values and the bias all require grad) with one incoming gradient; one
   layer each, no rotation (the weights stay where the caches leave them, for both sides alike).

Written to profiles/sddmm_ab.json.

    python scripts/sddmm_ab.py [--rounds 5] [--steps 50] [--warmup 10] [--out FILE]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = (32, 256, 2048)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotation-mb", type=float, default=320.0)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s for the implied fraction")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm_ab.json"))
    args = ap.parse_args()

    import numpy as np
    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import datasets as ds

    if not torch.cuda.is_available():
        raise SystemExit("sddmm_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    M = K = args.size

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    def rand(*shape):
        return torch.rand(shape, device=dev, generator=gen).mul_(2).sub_(1).half()

    def timed(fns, order):
        """us per step of every side in `order`, round by round, the sides alternating"""
        us = {k: [] for k in order}
        for k in order:
            for i in range(args.warmup):
                fns[k](i)
        torch.cuda.synchronize(dev)
        for _ in range(args.rounds):
            for k in order:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                for i in range(args.steps):
                    fns[k](i)
                e1.record()
                torch.cuda.synchronize(dev)
                us[k].append(e0.elapsed_time(e1) / args.steps * 1e3)
        return {k: {"rounds": [round(x, 2) for x in v], "median": round(statistics.median(v), 2),
                    "min_to_max_spread": round(max(v) - min(v), 2)} for k, v in us.items()}

    row, col, val = ds.pruned_weight(M, K, args.sparsity, 13)
    nnz = len(row)
    col_bytes = 2 if K <= 65536 else 4
    pattern_bytes = nnz * (4 + col_bytes) + (M + 1) * 4
    copies = max(2, int(math.ceil(args.rotation_mb * 1e6 / (pattern_bytes + 2 * (M + K) * max(TOKENS)))))
    plans = []
    for _ in range(copies):
        plan = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", 32, 40, 1).compile().upload("f16", 0)
        plans.append(plan.sddmm_prepare())
    say(f"{M} x {K}, nnz {nnz}, {copies} plans, pattern + out {pattern_bytes} bytes per step")
    ri, ci = torch.from_numpy(row.astype(np.int64)).to(dev), torch.from_numpy(col.astype(np.int64)).to(dev)
    result = {"what": "k_sddmm_tm against torch's dense product + gather, and SparseLinear(grad='all') forward + backward "
                      "against torch.nn.Linear (scripts/sddmm_ab.py): us per step, device events around each round's steps",
              "device": torch.cuda.get_device_name(0), "M": M, "K": K, "nnz": nnz, "sparsity": args.sparsity,
              "rounds": args.rounds, "steps_per_round": args.steps, "warmup_steps": args.warmup, "copies": copies,
              "hbm_peak_tbs": args.hbm_tbs, "geometry": gsa.sddmm_geometry(), "sddmm": {}, "layer": {}}

    for n in TOKENS:
        Gs, Xs = [rand(n, M) for _ in range(copies)], [rand(n, K) for _ in range(copies)]
        outs = [torch.empty(nnz, device=dev) for _ in range(copies)]
        dense = [torch.empty((M, K), device=dev, dtype=torch.float16) for _ in range(2)]
        # once, for the record: the two sides agree to f16's rounding of the dense product
        a = plans[0].sddmm(Gs[0], Xs[0], out=outs[0])
        b = torch.matmul(Gs[0].t(), Xs[0])[ri, ci].float()
        agree = float(((a - b).abs() / b.abs().clamp_min(1.0)).max())

        def engine(i):
            plans[i % copies].sddmm(Gs[i % copies], Xs[i % copies], out=outs[i % copies])

        def torch_side(i):
            torch.matmul(Gs[i % copies].t(), Xs[i % copies], out=dense[i % 2])
            dense[i % 2][ri, ci]

        r = timed({"k_sddmm_tm": engine, "torch_dense_gather": torch_side}, ("k_sddmm_tm", "torch_dense_gather"))
        model = pattern_bytes + n * (M + K) * 2
        r["byte_model"] = model
        r["hbm_fraction_of_byte_model"] = round(model / (r["k_sddmm_tm"]["median"] * 1e-6) / (args.hbm_tbs * 1e12), 4)
        r["max_difference_to_torch_over_max_1_ref"] = round(agree, 5)
        result["sddmm"][f"n={n}"] = r
        say(f"sddmm n={n}: {r}")
        del Gs, Xs, outs, dense
    for p in plans:
        p.device_status()
        p.free()

    W = np.zeros((M, K), np.float32)
    W[row.astype(np.int64), col.astype(np.int64)] = val
    sparse = gsa.SparseLinear.from_dense(torch.from_numpy(W), torch.zeros(M), grad="all").prepare_backward()
    dense_layer = torch.nn.Linear(K, M, device=dev, dtype=torch.float16)
    with torch.no_grad():
        dense_layer.weight.copy_(torch.from_numpy(W))
    for n in TOKENS:
        x, gy = rand(n, K).requires_grad_(True), rand(n, M)

        def step(layer):
            def run(i):
                x.grad = None
                for p in layer.parameters():
                    p.grad = None
                layer(x).backward(gy)
            return run

        r = timed({"SparseLinear": step(sparse), "torch.nn.Linear": step(dense_layer)}, ("SparseLinear", "torch.nn.Linear"))
        result["layer"][f"n={n}"] = r
        say(f"layer forward + backward n={n}: {r}")
    sparse.plan.device_status()
    sparse.plan_T.device_status()

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
