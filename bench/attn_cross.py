#!/usr/bin/env python3
"""Cross-attention: ``ops.cross_attention`` (csrc/kernels/attn.hip) against the PyTorch
expression the Keras ``MultiHeadAttention`` layer ran for ``layer(decoder, encoder)`` before the
kernels existed, forward and forward+backward per call, attention dropout 0.1, on
B=32 H=12 T=128 S=512 and B=8 H=12 T=512 S=2048 (D = 64).

    python bench/attn_cross.py
    python bench/attn_cross.py --shapes 32x12x128x512 --repeats 7

Both routes run in the same process on the same bf16 projections ``q [B, T, H*64]`` and
``kv [B, S, 2*H*64]``; the projections themselves are outside the timed region (they are the
same GEMMs on both routes).  The PyTorch route is copied from the layer as it was: fp32 head
split, ``torch.matmul`` scores ``[B, H, T, S]``, softmax, ``F.dropout``, ``torch.matmul`` with V,
cast back -- library GEMMs and a materialised score tensor.

Timing as in bench/attn_causal.py: device events around ``--iters`` back-to-back calls on one
stream, after a warm-up of every shape; ``--repeats`` such windows per shape.  Reported per
call: the median window and the spread (min .. max) of the windows, in microseconds.  One
JSON line per shape, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32x12x128x512,8x12x512x2048", help="BxHxTxS, comma separated")
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=10)
    return ap.parse_args()


def main():
    args = parse()
    import torch
    import torch.nn.functional as F

    from cloud_amd.ops import cross_attention

    if not torch.cuda.is_available():
        sys.exit("attn_cross: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    p, D = args.p, 64

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

    def torch_route(q, kv, H):
        """The layer's cross-attention core before ops.cross_attention (its PyTorch path)."""
        hd = H * D

        def heads(y):
            return y.float().reshape(y.shape[0], y.shape[1], H, D).transpose(1, 2)  # [B, H, len, D]

        qh, k, v = heads(q), heads(kv[..., :hd]), heads(kv[..., hd:])
        att = (qh @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
        scores = att.softmax(-1)
        pd = F.dropout(scores, p, training=True) if p > 0 else scores
        return (pd @ v).transpose(1, 2).reshape(q.shape[0], q.shape[1], hd).to(q.dtype)

    def measure(route, q, kv, dctx):
        def fwd():
            with torch.no_grad():
                return route(q, kv)

        def fwd_bwd():
            q.grad = kv.grad = None
            route(q, kv).backward(dctx)

        return {"fwd": windows(fwd), "fwd_bwd": windows(fwd_bwd)}

    results = []
    for shape in [s for s in args.shapes.split(",") if s]:
        B, H, T, S = (int(v) for v in shape.split("x"))
        C = H * D
        g = torch.Generator(device=dev).manual_seed(T + S)
        q = (torch.randn(B, T, C, device=dev, generator=g) * 0.5).to(torch.bfloat16).requires_grad_()
        kv = (torch.randn(B, S, 2 * C, device=dev, generator=g) * 0.5).to(torch.bfloat16).requires_grad_()
        dctx = torch.randn(B, T, C, device=dev, generator=g).to(torch.bfloat16)
        row = {"B": B, "H": H, "T": T, "S": S, "p": p,
               "kernels": measure(lambda a, b: cross_attention(a, b, H, None, p, True, seed=1234), q, kv, dctx),
               "pytorch": measure(lambda a, b: torch_route(a, b, H), q, kv, dctx)}
        row["pytorch_over_kernels"] = {k: round(row["pytorch"][k]["median_us"] / row["kernels"][k]["median_us"], 2)
                                       for k in ("fwd", "fwd_bwd")}
        print(json.dumps(row), flush=True)
        results.append(row)
    print(json.dumps({"metric": "cross-attention time per call, in-tree kernels and the PyTorch route", "unit": "us",
                      "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                      "shapes": {f"{r['B']}x{r['H']}x{r['T']}x{r['S']}":
                                 {"kernels": {k: r["kernels"][k]["median_us"] for k in ("fwd", "fwd_bwd")},
                                  "pytorch": {k: r["pytorch"][k]["median_us"] for k in ("fwd", "fwd_bwd")}}
                                 for r in results}}), flush=True)


if __name__ == "__main__":
    main()
