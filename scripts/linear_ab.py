#!/usr/bin/env python3
"""What the token-major linear (Plan.linear / gs_linear) buys: four ways to run a pruned layer on
activations held as (tokens, features), timed in one process.

  a  spmm        plan.spmm on a pre-transposed operand (B: K x N -> C: M x N): the floor, what the
                 engine ran before; a caller with token-major activations cannot use it as it is
  b  linear      plan.linear, fused: k_mfma_ks_tm on x (N x K) -> y (N x M), one launch
  c  transposes  what such a caller ran before: B.copy_(x.t()), plan.spmm, y.copy_(C.t()) -- two
                 extra torch kernels and two extra round trips through HBM
  d  three       plan.linear with LINEAR_FUSE = 0: k_tm_in, the plan's SpMM, k_tm_out

Workloads (fp16, 32 tokens, 70% pruned weights, seeded): c2 = 5120^2 on block_total(40,1) with
KS_NT = 1; attn / fc1 / fc2 = the OPT-30B layer's shapes (its six matrices are 4 x attn, fc1, fc2) on
block_total(112,1).  Every plan rotates over replicas (and their operand buffers) past the Infinity
Cache.  After the warm-up the variants alternate (a, b, c, d, a, ...), each round timing `steps`
steps between two device events; the enqueue loop's host time is recorded next to it.  The outputs
of b, c and d are compared with a's once before the timing (b and c bit for bit).
Written to profiles/linear_ab.json.

    python scripts/linear_ab.py [--rounds 5] [--steps 100] [--warmup 10] [--only c2,attn] [--out FILE]
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
VARIANTS = ("spmm", "linear", "transposes", "three")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rotation-mb", type=float, default=640.0)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--only", default="c2,attn,fc1,fc2")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_ab.json"))
    args = ap.parse_args()

    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import batch as bt
    from generalsparse_amd import datasets as ds
    from generalsparse_amd.autotune import build_candidate

    if not torch.cuda.is_available():
        raise SystemExit("linear_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    N = 32
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    class Step:
        """one replica's operands: x (N x K) and its transpose B, C (M x N), y (N x M)"""

        def __init__(self, plan, replica, M, K):
            self.plan, self.replica = plan, replica
            self.x = torch.rand((N, K), device=dev, generator=gen).mul_(2).sub_(1).half()
            self.B = self.x.t().contiguous()
            self.B2 = torch.empty_like(self.B)
            self.C = torch.empty((M, N), device=dev, dtype=torch.float16)
            self.y = torch.empty((N, M), device=dev, dtype=torch.float16)
            self.h, self.L = plan._h, plan._L
            self.p = {k: ctypes.c_void_p(getattr(self, k).data_ptr()) for k in ("x", "B", "B2", "C", "y")}

        def run(self, v):
            p = self.p
            if v == "spmm":
                rc = self.L.gs_spmm_replica(self.h, self.replica, p["B"], p["C"], N, stream)
            elif v == "transposes":
                self.B2.copy_(self.x.t())
                rc = self.L.gs_spmm_replica(self.h, self.replica, p["B2"], p["C"], N, stream)
                self.y.copy_(self.C.t())
            else:
                rc = self.L.gs_linear(self.h, self.replica, p["x"], p["y"], N, None, stream)
            assert rc == 0, (v, rc)

    def make(name):
        if name == "c2":
            M = K = 5120
            seed, cand = 13, ("block_total", 40, 1, {"KS_NT": 1})
        else:
            M, K = bt.C5_SHAPES[name]
            seed, cand = bt.shape_seed(0, name), ("block_total", 112, 1, {})
        row, col, val = ds.pruned_weight(M, K, args.sparsity, seed)
        plan = build_candidate(M, K, row, col, val, cand, N, "f16")
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks" and plan.linear_fused(N) == 1, info
        copies = max(2, int(math.ceil(args.rotation_mb * 1e6 / (info["device_bytes_A"] + 2 * (K + M) * N * 2))))
        for _ in range(copies - 1):
            plan.add_replica()
        say(f"{name}: {M} x {K}, {cand[0]}({cand[1]},{cand[2]}), K ranges {info['ksplit']}, {copies} replicas")
        return plan, [Step(plan, r, M, K) for r in range(copies)], \
            f"{M} x {K} {cand[0]}({cand[1]},{cand[2]}) {cand[3]}, K ranges {info['ksplit']}, {copies} replicas in rotation"

    def fuse_for(v):
        gsa.set_config("LINEAR_FUSE", 0 if v == "three" else 1)

    def agree(steps):
        st = steps[0]
        st.run("spmm")
        torch.cuda.synchronize(dev)
        want = st.C.t().contiguous()
        same = {}
        for v in VARIANTS[1:]:
            fuse_for(v)
            st.y.fill_(float("nan"))
            st.run(v)
            torch.cuda.synchronize(dev)
            same[v] = bool((st.y.view(torch.int16) == want.view(torch.int16)).all())
            assert same[v], v  # (no epilogue: d's second rounding is of an fp16 value, exact)
        fuse_for("linear")
        return same

    def measure(name, steps):
        n = len(steps)
        for v in VARIANTS:
            fuse_for(v)
            for i in range(max(args.warmup, n)):  # (d's scratch is allocated here, once per replica)
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
        fuse_for("linear")
        med = {v: statistics.median(dev_us[v]) for v in VARIANTS}
        return {"unit": "us per step: device events around the round's steps; host = the enqueue loop's wall time",
                "rounds": {v: [round(x, 3) for x in dev_us[v]] for v in VARIANTS},
                "host_rounds": {v: [round(x, 3) for x in host_us[v]] for v in VARIANTS},
                "median": {v: round(med[v], 3) for v in VARIANTS},
                "spmm_min_to_max_spread": round(max(dev_us["spmm"]) - min(dev_us["spmm"]), 3),
                "linear_minus_spmm": round(med["linear"] - med["spmm"], 3),
                "transposes_minus_linear": round(med["transposes"] - med["linear"], 3),
                "three_minus_linear": round(med["three"] - med["linear"], 3)}

    result = {"what": "a pruned layer on (tokens, features) activations four ways (scripts/linear_ab.py): spmm on a "
                      "pre-transposed operand, linear fused (k_mfma_ks_tm), torch transposes around spmm, linear with "
                      "LINEAR_FUSE=0 (k_tm_in + spmm + k_tm_out)",
              "device": torch.cuda.get_device_name(0), "tokens": N, "sparsity": args.sparsity, "rounds": args.rounds,
              "steps_per_round": args.steps, "warmup_steps": args.warmup}
    for name in args.only.split(","):
        plan, steps, what = make(name)
        result[name] = {"plan": what, "bit_identical_to_spmm": agree(steps)}
        result[name].update(measure(name, steps))
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
