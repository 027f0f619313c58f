#!/usr/bin/env python3
"""What FP8 (e4m3) weight values buy on the flagship layer: the f16 plan and the FP8-weight plan
(Plan.upload(weights="fp8")) of one pattern, timed in one process.

Matrix: the 5120^2 70%-pruned stand-in (datasets.pruned_weight, seed 13) on block_total(40,1) with
KS_NT = 1, built for 32 tokens.  Calls: plan.linear at n = 8, 32 and 128 tokens (k_mfma_ks_tm, one launch
of ceil(n / 32) tiles) and plan.spmm at N = 32 (k_mfma_ks).  Both plans rotate over replicas (and their
operand buffers) past the Infinity Cache.  After the warm-up the two plans alternate (f16, fp8, f16, ...)
call by call, each round timing `steps` steps between two device events -- the discipline of
scripts/linear_ab.py.  Per call: the median and the min-to-max spread over the rounds, the bytes of A's
tiles a step reads (tile_bytes) and the fraction of the HBM peak (--hbm-tbs) they imply at the median.
The FP8 plan's outputs are compared once, before the timing, with the f16 plan's and the difference
reported relative to the output's RMS: the weights differ by the quantisation (4 significant bits), so
this is the quantisation's effect on the layer, not a correctness check -- bit-exactness against the
dequantised weights is tests/test_gpu_fp8.py's.

--f16-only times the f16 plan alone: the same script then runs on a commit without FP8 weights, for the
check that the existing path did not move.
Written to profiles/linear_w8_ab.json.

    python scripts/linear_w8_ab.py [--rounds 5] [--steps 100] [--warmup 10] [--f16-only] [--out FILE]
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TOKENS = (8, 32, 128)
W = 32  # the width the plans are built for


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotation-mb", type=float, default=640.0)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s for the implied fraction")
    ap.add_argument("--f16-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_w8_ab.json"))
    args = ap.parse_args()

    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import datasets as ds

    if not torch.cuda.is_available():
        raise SystemExit("linear_w8_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    M = K = 5120
    variants = ("f16",) if args.f16_only else ("f16", "fp8")
    calls = [f"linear n={n}" for n in TOKENS] + [f"spmm N={W}"]

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    class Step:
        """one replica's operands: x (128 x K), B = x[:32]^T, C (M x 32), y (128 x M)"""

        def __init__(self, plan, replica):
            self.replica, self.h, self.L = replica, plan._h, plan._L
            self.x = torch.rand((max(TOKENS), K), device=dev, generator=gen).mul_(2).sub_(1).half()
            self.B = self.x[:W].t().contiguous()
            self.C = torch.empty((M, W), device=dev, dtype=torch.float16)
            self.y = torch.empty((max(TOKENS), M), device=dev, dtype=torch.float16)
            self.p = {k: ctypes.c_void_p(getattr(self, k).data_ptr()) for k in ("x", "B", "C", "y")}

        def run(self, call):
            if call.startswith("spmm"):
                rc = self.L.gs_spmm_replica(self.h, self.replica, self.p["B"], self.p["C"], W, stream)
            else:
                rc = self.L.gs_linear(self.h, self.replica, self.p["x"], self.p["y"], int(call.split("=")[1]), None, stream)
            assert rc == 0, (call, rc)

    row, col, val = ds.pruned_weight(M, K, args.sparsity, 13)
    plans, steps, infos = {}, {}, {}
    for v in variants:
        old = gsa.get_config("KS_NT")
        gsa.set_config("KS_NT", 1)
        try:
            plan = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", W, 40, 1).compile()
            if v == "fp8":
                plan.upload("f16", 0, weights="fp8")
            else:
                plan.upload("f16", 0)
        finally:
            gsa.set_config("KS_NT", old)
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and plan.linear_fused(W) == 1 and info.get("weights", 0) == (v == "fp8"), info
        copies = max(2, int(math.ceil(args.rotation_mb * 1e6 / (info["device_bytes_A"] + 2 * (K + M) * max(TOKENS) * 2))))
        for _ in range(copies - 1):
            plan.add_replica()
        plans[v], infos[v] = plan, info
        steps[v] = [Step(plan, r) for r in range(copies)]
        say(f"{v}: tile_bytes {info['tile_bytes']}, device_bytes_A {info['device_bytes_A']}, K ranges {info['ksplit']}, "
            f"{copies} replicas")

    near = {}
    if "fp8" in variants:  # the same x through both plans
        a, b = steps["f16"][0], steps["fp8"][0]
        b.x.copy_(a.x)
        b.B.copy_(a.B)
        for call in calls:
            a.run(call)
            b.run(call)
            torch.cuda.synchronize(dev)
            n = W if call.startswith("spmm") else int(call.split("=")[1])
            got, want = (b.C, a.C) if call.startswith("spmm") else (b.y[:n], a.y[:n])
            # e4m3 keeps 4 significant bits: each weight moves by up to 2^-4 of itself, a row's ~1500 terms average it
            diff, rms = (got.float() - want.float()), want.float().pow(2).mean().sqrt()
            near[call] = {"rms_difference_over_rms_output": round(float(diff.pow(2).mean().sqrt() / rms), 5),
                          "max_difference_over_rms_output": round(float(diff.abs().max() / rms), 5)}
            say(f"fp8 against f16, {call}: {near[call]}")

    n_rep = {v: len(steps[v]) for v in variants}
    for v in variants:
        for call in calls:
            for i in range(max(args.warmup, n_rep[v])):
                steps[v][i % n_rep[v]].run(call)
        torch.cuda.synchronize(dev)
    us = {call: {v: [] for v in variants} for call in calls}
    for r in range(args.rounds):
        for call in calls:
            for v in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                for i in range(args.steps):
                    steps[v][i % n_rep[v]].run(call)
                e1.record()
                torch.cuda.synchronize(dev)
                us[call][v].append(e0.elapsed_time(e1) / args.steps * 1e3)
        say(f"round {r}: " + "; ".join(f"{call} " + " / ".join(f"{v} {us[call][v][-1]:.2f}" for v in variants) for call in calls))

    result = {"what": "the f16 plan and the FP8-weight plan of the 5120^2 70% layer (scripts/linear_w8_ab.py): us per step, "
                      "device events around each round's steps, the plans alternating call by call",
              "device": torch.cuda.get_device_name(0), "sparsity": args.sparsity, "rounds": args.rounds,
              "steps_per_round": args.steps, "warmup_steps": args.warmup, "hbm_peak_tbs": args.hbm_tbs,
              "plans": {v: {k: infos[v][k] for k in ("tile_bytes", "device_bytes_A", "ksplit", "ks_nt", "ks_head_groups")}
                        for v in variants},
              "replicas": n_rep, "fp8_difference_to_f16": near, "calls": {}}
    for call in calls:
        out = {}
        for v in variants:
            med = statistics.median(us[call][v])
            tiles = 1 if call.startswith("spmm") else (int(call.split("=")[1]) + 31) // 32
            out[v] = {"rounds": [round(x, 3) for x in us[call][v]], "median": round(med, 3),
                      "min_to_max_spread": round(max(us[call][v]) - min(us[call][v]), 3),
                      # (the tiles of one unit share its A stream through L2: A is counted once per step)
                      "hbm_fraction_of_tile_bytes": round(infos[v]["tile_bytes"] / (med * 1e-6) / (args.hbm_tbs * 1e12), 4),
                      "token_tiles": tiles}
        if "fp8" in variants:
            out["fp8_minus_f16"] = round(out["fp8"]["median"] - out["f16"]["median"], 3)
        result["calls"][call] = out
    for v in variants:
        plans[v].device_status()
        plans[v].free()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
