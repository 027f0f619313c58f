#!/usr/bin/env python3
"""What the fused SpMM epilogue buys: four ways to get relu(A @ B + bias) + residual, timed in one
process on two workloads.

  a  plain     the SpMM alone (gs_spmm_batch): the floor, no epilogue at all
  b  torch     the SpMM, then what a user writes without the epilogue: C.add_(bias), C.relu_(),
               C.add_(residual) -- three element-wise kernels per matrix, each reading and writing C
  c  postpass  the epilogue through gs_spmm_batch_ex with EPILOGUE_FUSE = 0: the SpMM, then one
               k_epilogue pass per matrix
  d  fused     the same call with EPILOGUE_FUSE = 1: the epilogue in k_mfma_ks's store, no extra kernel

Workloads (fp16, N = 32, 70% pruned weights, seeded):
  c2     5120^2 on block_total(40,1) with KS_NT = 1, one matrix per step, rotating over replicas
         (and their B / C / residual buffers) past the Infinity Cache;
  layer  the OPT-30B layer batch: 4 x attn, fc1, fc2 on block_total(112,1), six entries in one
         gsa.Batch = one k_mfma_ks_group launch per step.

Every variant is enqueued by one native call per step (a one-entry Batch on c2) plus, for b, the
torch calls.  After 10 warm-up steps per variant the variants alternate (a, b, c, d, a, ...), each
round timing 100 steps between two device events; the per-step host time of the enqueue loop is
recorded next to it, so a variant whose device time is set by the host's launch rate shows as such.
The outputs of b, c and d are compared once before the timing.  Written to profiles/epilogue_ab.json.

    python scripts/epilogue_ab.py [--rounds 5] [--steps 100] [--warmup 10] [--only c2|layer] [--out FILE]
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
VARIANTS = ("plain", "torch", "postpass", "fused")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotation-mb", type=float, default=640.0)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--only", choices=["c2", "layer"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "epilogue_ab.json"))
    args = ap.parse_args()

    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import batch as bt
    from generalsparse_amd import datasets as ds
    from generalsparse_amd.autotune import build_candidate

    if not torch.cuda.is_available():
        raise SystemExit("epilogue_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    N = 32
    stream = torch.cuda.current_stream(dev).cuda_stream
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    def operands(m, n):
        """B, C, bias (fp32 for the epilogue, an fp16 column for the torch ops), residual"""
        B = torch.rand((n, N), device=dev, generator=gen).mul_(2).sub_(1).half()
        C = torch.empty((m, N), device=dev, dtype=torch.float16)
        bias = torch.rand((m,), device=dev, generator=gen).mul_(2).sub_(1)
        res = torch.rand((m, N), device=dev, generator=gen).mul_(2).sub_(1).half()
        return B, C, bias, bias.half()[:, None].contiguous(), res

    class Step:
        """one step's batches (plain, and with the epilogues) and the torch ops of variant b"""

        def __init__(self, entries, ops):
            self.ops = ops
            self.plain = gsa.Batch(entries, N)
            self.epi = gsa.Batch(entries, N, epilogues=[{"bias": o[2], "activation": "relu", "residual": o[4]} for o in ops])
            assert self.plain.launches() == self.epi.launches(), (self.plain.launches(), self.epi.launches())

        def run(self, variant):
            if variant in ("plain", "torch"):
                self.plain.run(stream)
                if variant == "torch":
                    for _, C, _, b16, res in self.ops:
                        C.add_(b16)
                        C.relu_()
                        C.add_(res)
            else:
                self.epi.run(stream)

    def c2_steps():
        M = K = 5120
        row, col, val = ds.pruned_weight(M, K, args.sparsity, 13)
        plan = build_candidate(M, K, row, col, val, ("block_total", 40, 1, {"KS_NT": 1}), N, "f16")
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and plan.epilogue_fused(N) == 1, info
        copies = max(2, int(math.ceil(args.rotation_mb * 1e6 / (info["device_bytes_A"] + K * N * 2))))
        for _ in range(copies - 1):
            plan.add_replica()
        steps = []
        for r in range(copies):
            ops = [operands(M, K)]
            steps.append(Step([(plan, r, ops[0][0], ops[0][1])], ops))
        say(f"c2: k_mfma_ks K ranges {info['ksplit']}, {copies} replicas")
        return steps, [plan], f"block_total(40,1) KS_NT=1, K ranges {info['ksplit']}, {copies} replicas in rotation"

    def layer_steps():
        plans = {}
        for k, (m, n) in bt.C5_SHAPES.items():
            row, col, val = ds.pruned_weight(m, n, args.sparsity, bt.shape_seed(0, k))
            p = build_candidate(m, n, row, col, val, ("block_total", 112, 1, {}), N, "f16")
            assert p.info()["device_kernel"] == "k_mfma_ks" and p.epilogue_fused(N) == 1, p.info()
            for _ in range(bt.C5_SLOTS.count(k) - 1):
                p.add_replica()
            plans[k] = p
            say(f"layer {k}: K ranges {p.info()['ksplit']}")
            del row, col, val
        entries, ops = [], []
        for slot, k in enumerate(bt.C5_SLOTS):
            m, n = bt.C5_SHAPES[k]
            o = operands(m, n)
            ops.append(o)
            entries.append((plans[k], bt.C5_SLOTS[:slot].count(k), o[0], o[1]))
        step = Step(entries, ops)
        assert step.epi.launches() == [6], step.epi.launches()
        return [step], list(plans.values()), "block_total(112,1) x 6 entries, one k_mfma_ks_group launch per step"

    def fuse_for(variant):
        gsa.set_config("EPILOGUE_FUSE", 0 if variant == "postpass" else 1)

    def agree(steps):
        """b, c and d compute one thing: each against the fp32 evaluation of a's output"""
        st = steps[0]
        st.run("plain")
        torch.cuda.synchronize(dev)
        want = [torch.relu(C.float() + bias[:, None]) + res.float() for _, C, bias, _, res in st.ops]
        worst = {}
        for v in VARIANTS[1:]:
            fuse_for(v)
            st.run(v)
            torch.cuda.synchronize(dev)
            worst[v] = max(((C.float() - w).abs() / w.abs().clamp(min=1.0)).max().item() for (_, C, _, _, _), w in zip(st.ops, want))
            # three fp16 roundings in b, two in c, the SpMM's own rounding in `want`: 2^-8 of max(1, |.|) holds all
            assert worst[v] <= 2.0 ** -8, (v, worst[v])
        fuse_for("fused")
        return {v: round(x, 6) for v, x in worst.items()}

    def measure(name, steps):
        n = len(steps)
        for v in VARIANTS:
            fuse_for(v)
            for i in range(max(args.warmup, n)):
                steps[i % n].run(v)
            torch.cuda.synchronize(dev)
        dev_us = {v: [] for v in VARIANTS}
        host_us = {v: [] for v in VARIANTS}
        for r in range(args.rounds):
            for v in VARIANTS:
                fuse_for(v)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    steps[i % n].run(v)
                t1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize(dev)
                dev_us[v].append(e0.elapsed_time(e1) / args.steps * 1e3)
                host_us[v].append((t1 - t0) / args.steps * 1e6)
            say(f"{name} round {r}: " + ", ".join(f"{v} {dev_us[v][-1]:.2f} us (host {host_us[v][-1]:.2f})" for v in VARIANTS))
        fuse_for("fused")
        med = {v: statistics.median(dev_us[v]) for v in VARIANTS}
        return {"unit": "us per step: device events around the round's steps; host = the enqueue loop's wall time",
                "rounds": {v: [round(x, 3) for x in dev_us[v]] for v in VARIANTS},
                "host_rounds": {v: [round(x, 3) for x in host_us[v]] for v in VARIANTS},
                "median": {v: round(med[v], 3) for v in VARIANTS},
                "plain_min_to_max_spread": round(max(dev_us["plain"]) - min(dev_us["plain"]), 3),
                "fused_minus_plain": round(med["fused"] - med["plain"], 3),
                "postpass_minus_fused": round(med["postpass"] - med["fused"], 3),
                "torch_minus_fused": round(med["torch"] - med["fused"], 3),
                "fused_le_postpass_lt_torch": bool(med["fused"] <= med["postpass"] < med["torch"])}

    result = {"what": "relu(A @ B + bias) + residual four ways (scripts/epilogue_ab.py): plain SpMM, SpMM + three torch "
                      "kernels, SpMM + k_epilogue (EPILOGUE_FUSE=0), fused into k_mfma_ks",
              "device": torch.cuda.get_device_name(0), "N": N, "sparsity": args.sparsity, "rounds": args.rounds,
              "steps_per_round": args.steps, "warmup_steps": args.warmup}
    for name, make in (("c2", c2_steps), ("layer", layer_steps)):
        if args.only and args.only != name:
            continue
        steps, plans, what = make()
        result[name] = {"plan": what, "max_rel_err_against_fp32_stages": agree(steps)}
        result[name].update(measure(name, steps))
        for p in plans:
            p.device_status()
            p.free()
        del steps, plans
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
