#!/usr/bin/env python3
"""What the grouped token-major linear (LinearBatch / gs_linear_batch, k_mfma_ks_tm_group) buys three layers that
share one x -- the Q/K/V shape -- against the three single calls, timed in one process.

  batch    LinearBatch.run(): one gs_linear_batch call, ONE k_mfma_ks_tm_group launch for the three layers
  singles  three Plan.linear calls on the same stream: three k_mfma_ks_tm launches
  batch_c / singles_c  the same two through ctypes on argument arrays built once (gs_linear_batch against three
           gs_linear calls): next to no host work per call, so the device events see the launches and not Python

The layers (f16, seeded): three 5120 x 5120 weights at 70% sparsity on block_total(40,1), built for 32 tokens,
every one a k_mfma_ks plan; x is (tokens, 5120), shared.  Measured at 8, 32 and 128 tokens.  At each token count
every way is warmed up, then the ways are timed over `steps` calls each in `rounds` alternating rounds, twice:
between two device events, and by the host clock around the calls and a device synchronise.  Back-to-back calls
re-read the same three weights (3 x ~31 MB of tiles), which the Infinity Cache holds: both sides of the comparison
run warm, as a decode loop over few layers would, not behind a model's other traffic.
Reported per way: the rounds, their median and their spread (max - min).  not_slower: the grouped call's median is
at most the singles' median plus the larger of the two spreads.  Before the timing the grouped outputs are compared
bit for bit with the single calls'.
Written to profiles/linear_batch_ab.json.

    python scripts/linear_batch_ab.py [--rounds 7] [--steps 200] [--warmup 20] [--size 5120] [--out FILE]
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
TOKENS = (8, 32, 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--size", type=int, default=5120)
    ap.add_argument("--sparsity", type=float, default=0.7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_batch_ab.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least 5 rounds: the spread is part of the result")

    import torch
    import generalsparse_amd as gsa
    from generalsparse_amd import _lib
    from generalsparse_amd import datasets as ds

    if not torch.cuda.is_available():
        raise SystemExit("linear_batch_ab.py times kernels: it needs the GPU")
    dev = torch.device("cuda:0")
    M = K = args.size

    def say(msg):
        print(f"[{time.strftime('%H:%M:%S')}] {msg}", flush=True)

    plans = []
    for seed in (13, 14, 15):
        row, col, val = ds.pruned_weight(M, K, args.sparsity, seed)
        plan = gsa.Plan.from_coo(M, K, row, col, val).run_pipeline("block_total", 32, 40, 1).compile().upload("f16", 0)
        info = plan.info()
        assert info["device_kernel"] == "k_mfma_ks", info
        plans.append(plan)
        say(f"layer {len(plans)}: {M} x {K}, {info['nnz']} non-zeros, {info['ksplit']} K ranges, tile bytes {info['tile_bytes']}")
    L = plans[0]._L
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)

    per_tokens = {}
    for n in TOKENS:
        x = torch.rand((n, K), device=dev, generator=gen).mul_(2).sub_(1).half()
        ys = [torch.empty((n, M), dtype=torch.float16, device=dev) for _ in plans]
        ref = [torch.empty_like(y) for y in ys]
        batch = gsa.LinearBatch([(p, 0, x, y) for p, y in zip(plans, ys)])
        assert batch.launches() == [3], batch.launches()
        assert all(p.linear_launches(n) == [(n + 31) // 32] for p in plans)

        def singles(out=ys):
            for p, y in zip(plans, out):
                p.linear(x, out=y)

        def singles_c():
            for p, y in zip(plans, ys):
                rc = L.gs_linear(p._h, 0, ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(y.data_ptr()), n, None, stream)
                assert rc == 0, rc

        def batch_c():
            _lib.check(L.gs_linear_batch(batch._p, batch._r, batch._x, batch._y, batch._t, None, 3, stream))

        # the same bits first
        singles(ref)
        for y in ys:
            y.fill_(float("nan"))
        batch.run()
        torch.cuda.synchronize(dev)
        same = all(bool((y.view(torch.int16) == r.view(torch.int16)).all()) for y, r in zip(ys, ref))
        assert same, f"{n} tokens: the grouped outputs differ from the single calls'"

        ways = {"batch": batch.run, "singles": singles, "batch_c": batch_c, "singles_c": singles_c}
        for fn in ways.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize(dev)
        us = {k: [] for k in ways}
        wall_us = {k: [] for k in ways}
        for r in range(args.rounds):
            for name, fn in ways.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.steps):
                    fn()
                e1.record()
                torch.cuda.synchronize(dev)
                wall_us[name].append((time.perf_counter() - t0) / args.steps * 1e6)
                us[name].append(e0.elapsed_time(e1) / args.steps * 1e3)
            say(f"{n} tokens, round {r}: " + ", ".join(f"{k} {us[k][-1]:.2f} us (wall {wall_us[k][-1]:.2f})" for k in ways))
        for p in plans:
            p.device_status()

        def stats(v):
            return {"rounds": [round(t, 2) for t in v], "median": round(statistics.median(v), 2), "spread": round(max(v) - min(v), 2)}

        res = {"same_bits_as_the_single_calls": same, "us": {k: stats(v) for k, v in us.items()},
               "wall_us": {k: stats(v) for k, v in wall_us.items()}}
        for a, b in (("batch", "singles"), ("batch_c", "singles_c")):
            for kind in ("us", "wall_us"):
                A, B = res[kind][a], res[kind][b]
                res[f"{a}_over_{b}_{kind}"] = round(A["median"] / B["median"], 4)
                res[f"{a}_not_slower_{kind}"] = A["median"] <= B["median"] + max(A["spread"], B["spread"])
        per_tokens[str(n)] = res

    result = {
        "what": "three layers on one x: LinearBatch.run() (one k_mfma_ks_tm_group launch) against three Plan.linear calls "
                "(three k_mfma_ks_tm launches), and the same through ctypes (scripts/linear_batch_ab.py)",
        "device": torch.cuda.get_device_name(0),
        "layers": f"3 x ({M} x {K}, {args.sparsity:.0%} sparse, f16, block_total(40,1) at 32 tokens), one shared x",
        "rounds": args.rounds, "steps_per_round": args.steps, "warmup_calls": args.warmup,
        "unit": "us per call of all three layers: device events around the round's calls; wall: the host clock around the "
                "calls and a synchronise.  spread: max - min over the rounds.  not_slower: median <= the other median + "
                "the larger spread",
        "tokens": per_tokens,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
