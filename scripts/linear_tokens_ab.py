#!/usr/bin/env python3
"""The token-major linear (Plan.linear / gs_linear) at token counts other than the plan's width: a
layer built for 32 tokens, called with n tokens, timed in one process two ways.

  b  linear  fused: k_mfma_ks_tm on ceil(n / 32) token tiles, one launch
  d  three   LINEAR_FUSE = 0: k_tm_in, the plan's SpMM at width n, k_tm_out -- for n != 32 what every
             call ran before the kernel took token tiles (the SpMM is then a gather-family kernel on a
             CSR copy of A)

Workloads, rotation past the Infinity Cache and the timing are scripts/linear_ab.py's: fp16, 70%
pruned weights, c2 = 5120^2 on block_total(40,1) with KS_NT = 1, attn / fc1 / fc2 = the OPT-30B
layer's shapes on block_total(112,1); after the warm-up the variants alternate, each round timing
`steps` steps between two device events.  b's output is compared bit for bit with the 32-token calls
of the same rows (zero-padded last slice) before the timing.  --variants linear times b alone: run
it under GS_LIBRARY with two builds of the library, the processes alternating, to compare builds
(the experiments build with and without -DGS_KS_TM_TILE_MAJOR: the order of the tiles in the grid).
Written to --out (default profiles/linear_tokens_ab.json).

    python scripts/linear_tokens_ab.py [--tokens 8,24,32,64,128,256] [--rounds 5] [--steps 100]
                                       [--only c2,attn,fc1,fc2] [--variants linear,three] [--out FILE]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="8,24,32,64,128,256")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotation-mb", type=float, default=640.0)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--only", default="c2,attn,fc1,fc2")
    ap.add_argument("--variants", default="linear,three")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_tokens_ab.json"))
    args = ap.parse_args()
    tokens = [int(t) for t in args.tokens.split(",")]
    variants = tuple(args.variants.split(","))
    assert set(variants) <= {"linear", "three"} and tokens and min(tokens) >= 1

    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import batch as bt
    from generalsparse_amd import datasets as ds
    from generalsparse_amd.autotune import build_candidate

    if not torch.cuda.is_available():
        raise SystemExit("linear_tokens_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    W = 32
    nmax = max(tokens)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    class Step:
        """one replica's operands: x (nmax x K) and y (nmax x M); a call takes the first n rows"""

        def __init__(self, plan, replica, M, K):
            self.plan, self.replica = plan, replica
            self.x = torch.rand((nmax, K), device=dev, generator=gen).mul_(2).sub_(1).half()
            self.y = torch.empty((nmax, M), device=dev, dtype=torch.float16)
            self.h, self.L = plan._h, plan._L
            self.px, self.py = ctypes.c_void_p(self.x.data_ptr()), ctypes.c_void_p(self.y.data_ptr())

        def run(self, n):
            rc = self.L.gs_linear(self.h, self.replica, self.px, self.py, n, None, stream)
            assert rc == 0, (n, rc, self.L.gs_last_error().decode())

    def make(name):
        if name == "c2":
            M = K = 5120
            seed, cand = 13, ("block_total", 40, 1, {"KS_NT": 1})
        else:
            M, K = bt.C5_SHAPES[name]
            seed, cand = bt.shape_seed(0, name), ("block_total", 112, 1, {})
        row, col, val = ds.pruned_weight(M, K, args.sparsity, seed)
        plan = build_candidate(M, K, row, col, val, cand, W, "f16")
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and all(plan.linear_fused(n) == 1 for n in tokens), info
        copies = max(2, int(math.ceil(args.rotation_mb * 1e6 / (info["device_bytes_A"] + 2 * (K + M) * nmax * 2))))
        for _ in range(copies - 1):
            plan.add_replica()
        say(f"{name}: {M} x {K}, {cand[0]}({cand[1]},{cand[2]}), K ranges {info['ksplit']}, {copies} replicas")
        return plan, [Step(plan, r, M, K) for r in range(copies)], \
            f"{M} x {K} {cand[0]}({cand[1]},{cand[2]}) {cand[3]}, K ranges {info['ksplit']}, {copies} replicas in rotation"

    def fuse_for(v):
        gsa.set_config("LINEAR_FUSE", 0 if v == "three" else 1)

    def agree(st, n):
        """b at n tokens against the 32-token calls on the same rows, bit for bit"""
        fuse_for("linear")
        pad = torch.zeros(((n + W - 1) // W * W, st.x.shape[1]), dtype=st.x.dtype, device=dev)
        pad[:n] = st.x[:n]
        want = torch.cat([st.plan.linear(pad[i:i + W], replica=st.replica) for i in range(0, pad.shape[0], W)])[:n]
        st.y.fill_(float("nan"))
        st.run(n)
        torch.cuda.synchronize(dev)
        same = bool((st.y[:n].view(torch.int16) == want.view(torch.int16)).all())
        assert same, n
        return same

    def measure(name, steps, n):
        k = len(steps)
        for v in variants:
            fuse_for(v)
            for i in range(max(args.warmup, k)):  # (scratch and K-split state are allocated here, once per replica)
                steps[i % k].run(n)
            torch.cuda.synchronize(dev)
        dev_us = {v: [] for v in variants}
        host_us = {v: [] for v in variants}
        for r in range(args.rounds):
            for v in variants:
                fuse_for(v)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                e0.record()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    steps[i % k].run(n)
                t1 = time.perf_counter()
                e1.record()
                torch.cuda.synchronize(dev)
                dev_us[v].append(e0.elapsed_time(e1) / args.steps * 1e3)
                host_us[v].append((t1 - t0) / args.steps * 1e6)
        fuse_for("linear")
        med = {v: statistics.median(dev_us[v]) for v in variants}
        say(f"{name} n={n}: " + ", ".join(f"{v} {med[v]:.2f} us [{min(dev_us[v]):.2f} .. {max(dev_us[v]):.2f}]" for v in variants))
        out = {"rounds": {v: [round(x, 3) for x in dev_us[v]] for v in variants},
               "host_rounds": {v: [round(x, 3) for x in host_us[v]] for v in variants},
               "median": {v: round(med[v], 3) for v in variants},
               "min_to_max_spread": {v: round(max(dev_us[v]) - min(dev_us[v]), 3) for v in variants},
               "launches": steps[0].plan.linear_launches(n)}
        if len(variants) == 2:
            out["three_minus_linear"] = round(med["three"] - med["linear"], 3)
        return out

    result = {"what": "a pruned layer built for 32 tokens called with n tokens (scripts/linear_tokens_ab.py): linear fused "
                      "(k_mfma_ks_tm on ceil(n / 32) token tiles) and linear with LINEAR_FUSE=0 (k_tm_in + spmm at width n "
                      "+ k_tm_out)",
              "unit": "us per call: device events around the round's calls; host = the enqueue loop's wall time",
              "device": torch.cuda.get_device_name(0), "library": os.path.basename(gsa._lib.LIB_PATH),
              "experiments_build": int(gsa.get_config("GS_EXPERIMENTS")), "tokens": tokens, "variants": list(variants),
              "sparsity": args.sparsity, "rounds": args.rounds, "steps_per_round": args.steps, "warmup_steps": args.warmup}
    for name in args.only.split(","):
        plan, steps, what = make(name)
        result[name] = {"plan": what}
        for n in tokens:
            result[name][f"n={n}"] = dict(measure(name, steps, n), bit_identical_to_32_token_calls=agree(steps[0], n))
        plan.device_status()
        plan.free()
        del steps, plan
        torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
