#!/usr/bin/env python3
"""Attention masks: ``ops.cross_attention(mask=)`` on the masked cross-attention kernels
(csrc/kernels/attn.hip) against the same call without a mask and against the PyTorch expression
the Keras ``MultiHeadAttention`` layer runs for an ``attention_mask`` where the kernels do not
apply, forward and forward+backward per call, attention dropout 0.1, on B=32 H=12 T=128 S=512
and B=8 H=12 T=512 S=2048 (D = 64), each with two masks of density 0.5:

    padding   random boolean [B, 1, S]  (one byte row per batch entry, broadcast over queries)
    dense     random boolean [B, T, S]  (a byte per score and batch entry, broadcast over heads)

    python bench/attn_mask.py
    python bench/attn_mask.py --shapes 32x12x128x512 --repeats 7

All routes run in the same process on the same bf16 projections ``q [B, T, H*64]`` and
``kv [B, S, 2*H*64]``; the projections are outside the timed region.  The PyTorch route is the
layer's: fp32 head split, ``torch.matmul`` scores ``[B, H, T, S]``, ``masked_fill`` with
``finfo.min``, softmax, ``F.dropout``, ``torch.matmul`` with V, cast back.

Timing as in bench/attn_cross.py: device events around ``--iters`` back-to-back calls on one
stream, after a warm-up; ``--repeats`` such windows.  Reported per call: the median window and
the spread (min .. max) of the windows, in microseconds.  One JSON line per shape and mask, then
one summary line.
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
        sys.exit("attn_mask: needs a GPU (a CPU run measures nothing)")
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

    def torch_route(q, kv, H, allowed):
        """The layer's masked attention core on its PyTorch branch; ``allowed`` is [B, 1, T|1, S]."""
        hd = H * D

        def heads(y):
            return y.float().reshape(y.shape[0], y.shape[1], H, D).transpose(1, 2)  # [B, H, len, D]

        qh, k, v = heads(q), heads(kv[..., :hd]), heads(kv[..., hd:])
        att = (qh @ k.transpose(-1, -2)) * (1.0 / math.sqrt(D))
        att = att.masked_fill(~allowed, torch.finfo(att.dtype).min)
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
        unmasked = measure(lambda a, b: cross_attention(a, b, H, None, p, True, seed=1234), q, kv, dctx)
        for kind, mshape in (("padding", (B, 1, S)), ("dense", (B, T, S))):
            mask = torch.rand(*mshape, device=dev, generator=g) < 0.5
            row = {"B": B, "H": H, "T": T, "S": S, "p": p, "mask": kind, "mask_shape": list(mshape),
                   "masked": measure(lambda a, b: cross_attention(a, b, H, None, p, True, seed=1234, mask=mask),
                                     q, kv, dctx),
                   "unmasked": unmasked,
                   "pytorch": measure(lambda a, b: torch_route(a, b, H, mask[:, None]), q, kv, dctx)}
            for name, num, den in (("masked_over_unmasked", "masked", "unmasked"),
                                   ("pytorch_over_masked", "pytorch", "masked")):
                row[name] = {k: round(row[num][k]["median_us"] / row[den][k]["median_us"], 2)
                             for k in ("fwd", "fwd_bwd")}
            print(json.dumps(row), flush=True)
            results.append(row)
    print(json.dumps({"metric": "masked cross-attention time per call: masked kernels, unmasked kernels, "
                                "the PyTorch masked route", "unit": "us",
                      "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                      "shapes": {f"{r['B']}x{r['H']}x{r['T']}x{r['S']}/{r['mask']}":
                                 {n: {k: r[n][k]["median_us"] for k in ("fwd", "fwd_bwd")}
                                  for n in ("masked", "unmasked", "pytorch")}
                                 for r in results}}), flush=True)


if __name__ == "__main__":
    main()
