#!/usr/bin/env python3
"""Causal against non-causal fused attention (csrc/kernels/attn.hip), forward and
forward+backward per call at a fixed token count: B * S = 16384, H = 12, D = 64, attention
dropout 0.1, S in 128, 256, 512, 1024, 2048.

    python bench/attn_causal.py
    python bench/attn_causal.py --seqs 256,1024 --repeats 7

Both modes run in the same process on the same tensors.  Beside the measured causal /
non-causal ratio the script prints the block-count ideal: of the n x n 64 x 64 score blocks
(n = ceil(S / 64)) the causal kernels visit n (n + 1) / 2, so (n + 1) / 2n of the work.

Timing as in bench/attn_shapes.py: device events around ``--iters`` back-to-back calls on one
stream, after a warm-up of every shape; ``--repeats`` such windows per shape.  Reported per
call: the median window and the spread (min .. max) of the windows, in microseconds.  One
JSON line per shape, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="128,256,512,1024,2048")
    ap.add_argument("--tokens", type=int, default=16384)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    return ap.parse_args()


def main():
    args = parse()
    import torch

    from cloud_amd.ops import raw

    if not torch.cuda.is_available():
        sys.exit("attn_causal: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    H, p, seed = args.heads, args.p, 1234
    C = H * 64

    def windows(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / args.iters)
        out.sort()
        return {"median_us": round(out[len(out) // 2], 2), "min_us": round(out[0], 2), "max_us": round(out[-1], 2)}

    def measure(qkv, dctx, B, S, causal):
        def fwd():
            return raw.attn_fwd(qkv, B, S, H, None, p, seed, causal=causal)

        def fwd_bwd():
            ctx, lse = raw.attn_fwd(qkv, B, S, H, None, p, seed, causal=causal)
            return raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, None, p, seed, causal=causal)

        return {"fwd": windows(fwd), "fwd_bwd": windows(fwd_bwd)}

    results = []
    for S in [int(s) for s in args.seqs.split(",") if s]:
        B = max(1, args.tokens // S)
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = (torch.randn(B * S, 3 * C, device=dev, generator=g) * 0.5).to(torch.bfloat16)
        dctx = torch.randn(B * S, C, device=dev, generator=g).to(torch.bfloat16)
        n = (S + 63) // 64
        row = {"S": S, "B": B, "H": H, "p": p,
               "full": measure(qkv, dctx, B, S, False), "causal": measure(qkv, dctx, B, S, True)}
        row["causal_over_full"] = {k: round(row["causal"][k]["median_us"] / row["full"][k]["median_us"], 3)
                                   for k in ("fwd", "fwd_bwd")}
        row["block_ideal"] = round((n + 1) / (2 * n), 3)
        print(json.dumps(row), flush=True)
        results.append(row)
    print(json.dumps({"metric": "causal / non-causal attention time by sequence length", "unit": "ratio",
                      "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                      "shapes": {str(r["S"]): dict(r["causal_over_full"], ideal=r["block_ideal"]) for r in results}}),
          flush=True)


if __name__ == "__main__":
    main()
