#!/usr/bin/env python3
"""A/B of the bf16 twins of k_mfma_ks against the fp16 kernels, in one process.

Two workloads, each built once at fp16 and once at bf16 from the same seeded matrices:
  c2     the C2 plan: 5120^2 at 70%, N = 32, block_total(40,1) with KS_NT = 1, through a
         Rotation over replicas past the Infinity Cache (as bench.py times a plan);
  layer  the north_star layer: OPT-30B 70% (4 x attn, fc1, fc2) on block_total(112,1), six
         entries in one gsa.Batch = one k_mfma_ks_group launch per step.
After the settle (200 ms of untimed steps, bench.py's north_star object) and the warm-up, the two
types are timed in interleaved rounds (fp16, bf16, fp16, ...) with HIP events around each
round's steps.  Written to profiles/bf16_ab.json: every round, the medians, the fp16 rounds'
min-to-max spread and the verdict -- the bf16 median is to lie no further from the fp16 median
than that spread.

    python scripts/bf16_ab.py [--rounds 9] [--steps 500] [--warmup 500] [--out profiles/bf16_ab.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=500)
    ap.add_argument("--settle-ms", type=float, default=200.0)
    ap.add_argument("--rotation-mb", type=float, default=640.0)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--only", choices=["c2", "layer"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bf16_ab.json"))
    args = ap.parse_args()

    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import batch as bt
    from generalsparse_amd import datasets as ds
    from generalsparse_amd.autotune import build_candidate

    if not torch.cuda.is_available():
        raise SystemExit("bf16_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    N = 32
    tdt = {"f16": torch.float16, "bf16": torch.bfloat16}
    stream = torch.cuda.current_stream(dev).cuda_stream

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    def c2_objects():
        """{dtype: (step(count, first), info)}: `count` rotated launches of the C2 plan"""
        M = K = 5120
        row, col, val = ds.pruned_weight(M, K, args.sparsity, 13)
        out = {}
        for d in ("f16", "bf16"):
            plan = build_candidate(M, K, row, col, val, ("block_total", 40, 1, {"KS_NT": 1}), N, d)
            info = plan.info()
            assert info["device_kernel"] == "k_mfma_ks" and info["ks_nt"] == 1, info
            copies = max(2, int(math.ceil(args.rotation_mb * 1e6 / (info["device_bytes_A"] + K * N * 2))))
            for _ in range(copies - 1):
                plan.add_replica()
            g = torch.Generator(device=dev)
            g.manual_seed(7)
            Bs = [torch.rand((K, N), device=dev, generator=g).mul_(2).sub_(1).to(tdt[d]) for _ in range(copies)]
            Cs = [torch.empty((M, N), device=dev, dtype=tdt[d]) for _ in range(copies)]
            rot = plan.rotation(Bs, Cs)
            out[d] = (lambda count, first, rot=rot: rot.run(count, first, stream), info, plan)
            say(f"c2 {d}: k_mfma_ks K ranges {info['ksplit']}, {copies} replicas")
        return out

    def layer_objects():
        """{dtype: (step(count, first), info)}: `count` steps of the six-entry grouped launch"""
        out = {"f16": [], "bf16": []}
        plans = {"f16": {}, "bf16": {}}
        for k, (m, n) in bt.C5_SHAPES.items():
            row, col, val = ds.pruned_weight(m, n, args.sparsity, bt.shape_seed(0, k))
            for d in ("f16", "bf16"):
                p = build_candidate(m, n, row, col, val, ("block_total", 112, 1, {}), N, d)
                assert p.info()["device_kernel"] == "k_mfma_ks", p.info()
                for _ in range(bt.C5_SLOTS.count(k) - 1):
                    p.add_replica()
                plans[d][k] = p
                say(f"layer {k} {d}: K ranges {p.info()['ksplit']}")
            del row, col, val
        res = {}
        for d in ("f16", "bf16"):
            g = torch.Generator(device=dev)
            g.manual_seed(11)
            entries = []
            for slot, k in enumerate(bt.C5_SLOTS):
                m, n = bt.C5_SHAPES[k]
                B = torch.rand((n, N), device=dev, generator=g).mul_(2).sub_(1).to(tdt[d])
                C = torch.empty((m, N), device=dev, dtype=tdt[d])
                entries.append((plans[d][k], bt.C5_SLOTS[:slot].count(k), B, C))
            bat = gsa.Batch(entries, N)
            assert bat.launches() == [6], bat.launches()

            def step(count, first, bat=bat):
                for _ in range(count):
                    bat.run(stream)
            res[d] = (step, {"launches_per_step": bat.launches()}, (bat, plans[d]))
        return res

    def measure(name, objs):
        # settle, then the warm-up, both types
        for d in ("f16", "bf16"):
            step = objs[d][0]
            t0 = time.perf_counter()
            while (time.perf_counter() - t0) * 1e3 < args.settle_ms:
                step(10, 0)
                torch.cuda.synchronize(dev)
            step(args.warmup, 0)
            torch.cuda.synchronize(dev)
        rounds = {"f16": [], "bf16": []}
        for r in range(args.rounds):
            for d in ("f16", "bf16"):
                step = objs[d][0]
                step(20, 0)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(args.steps, 20)
                e1.record()
                torch.cuda.synchronize(dev)
                rounds[d].append(e0.elapsed_time(e1) / args.steps * 1e3)  # us per step
            say(f"{name} round {r}: fp16 {rounds['f16'][-1]:.3f} us, bf16 {rounds['bf16'][-1]:.3f} us")
        m16, mbf = statistics.median(rounds["f16"]), statistics.median(rounds["bf16"])
        spread = max(rounds["f16"]) - min(rounds["f16"])
        return {"unit": "us per step (HIP events around the round's steps)",
                "fp16_rounds": [round(x, 4) for x in rounds["f16"]], "bf16_rounds": [round(x, 4) for x in rounds["bf16"]],
                "fp16_median": round(m16, 4), "bf16_median": round(mbf, 4),
                "fp16_min_to_max_spread": round(spread, 4), "bf16_over_fp16": round(mbf / m16, 5),
                "bf16_within_fp16_spread": bool(abs(mbf - m16) <= spread)}

    result = {"what": "bf16 against fp16 on k_mfma_ks, interleaved rounds in one process (scripts/bf16_ab.py)",
              "device": torch.cuda.get_device_name(0), "N": N, "sparsity": args.sparsity, "rounds": args.rounds,
              "steps_per_round": args.steps, "warmup_steps": args.warmup, "settle_ms": args.settle_ms}
    for name, make in (("c2", c2_objects), ("layer", layer_objects)):
        if args.only and args.only != name:
            continue
        objs = make()
        result[name] = measure(name, objs)
        result[name]["plan"] = "block_total(40,1) KS_NT=1, Rotation" if name == "c2" else \
            "block_total(112,1) x 6 entries, one k_mfma_ks_group launch per step (Batch)"
        for d in ("f16", "bf16"):  # free the device copies before the next workload
            held = objs[d][2]
            for p in ([held] if name == "c2" else list(held[1].values())):
                p.device_status()
                p.free()
        del objs
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
