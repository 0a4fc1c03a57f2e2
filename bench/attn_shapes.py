#!/usr/bin/env python3
"""Fused attention (csrc/kernels/attn.hip) forward and forward+backward times per sequence
length, BERT-base heads: B = 64, H = 12, D = 64, attention dropout 0.1.

    python bench/attn_shapes.py                          # S in 100,128,192,200,256,384,400
    python bench/attn_shapes.py --seqs 128,192,256,384 --repeats 7

For every S that is no multiple of 64 the same data is also timed zero-padded to the next
multiple of 64 with key_len = S -- what a caller had to do before the kernels took any S.

Timing: device events around ``--iters`` back-to-back calls on one stream, after a warm-up
of every shape; ``--repeats`` such windows per shape.  Reported per call: the median window,
and the spread (min .. max) of the windows, in microseconds.  The calls go through
``ops.raw`` (pointer level, buffers allocated per call from the caching allocator), so the
script runs unchanged on a tree whose kernels take only S % 64 == 0 (pass such ``--seqs``).
One JSON line per shape, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seqs", default="100,128,192,200,256,384,400")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    return ap.parse_args()


def main():
    args = parse()
    import torch

    from cloud_amd.ops import raw

    if not torch.cuda.is_available():
        sys.exit("attn_shapes: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    B, H, p, seed = args.batch, args.heads, args.p, 1234
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

    def measure(qkv, dctx, S, key_len):
        def fwd():
            return raw.attn_fwd(qkv, B, S, H, key_len, p, seed)

        def fwd_bwd():
            ctx, lse = raw.attn_fwd(qkv, B, S, H, key_len, p, seed)
            return raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, key_len, p, seed)

        return {"fwd": windows(fwd), "fwd_bwd": windows(fwd_bwd)}

    results = []
    for S in [int(s) for s in args.seqs.split(",") if s]:
        g = torch.Generator(device=dev).manual_seed(S)
        qkv = (torch.randn(B, S, 3 * C, device=dev, generator=g) * 0.5).to(torch.bfloat16)
        dctx = torch.randn(B, S, C, device=dev, generator=g).to(torch.bfloat16)
        row = {"S": S, "B": B, "H": H, "p": p, "native": measure(qkv.view(B * S, -1), dctx.view(B * S, -1), S, None)}
        if S % 64:
            SP = (S + 63) // 64 * 64
            qkv_p = torch.zeros(B, SP, 3 * C, dtype=torch.bfloat16, device=dev)
            dctx_p = torch.zeros(B, SP, C, dtype=torch.bfloat16, device=dev)
            qkv_p[:, :S] = qkv
            dctx_p[:, :S] = dctx
            kl = torch.full((B,), S, dtype=torch.int32, device=dev)
            row["padded_to"] = SP
            row["padded"] = measure(qkv_p.view(B * SP, -1), dctx_p.view(B * SP, -1), SP, kl)
            row["native_over_padded"] = {k: round(row["native"][k]["median_us"] / row["padded"][k]["median_us"], 3)
                                         for k in ("fwd", "fwd_bwd")}
        print(json.dumps(row), flush=True)
        results.append(row)
    print(json.dumps({"metric": "attention us per call by sequence length", "unit": "us", "iters": args.iters,
                      "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                      "shapes": {str(r["S"]): {k: r["native"][k]["median_us"] for k in ("fwd", "fwd_bwd")}
                                 for r in results}}), flush=True)


if __name__ == "__main__":
    main()
