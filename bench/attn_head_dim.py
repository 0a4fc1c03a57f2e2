#!/usr/bin/env python3
"""Attention head dimensions: ``ops.attention`` on the kernels of csrc/kernels/attn.hip at
D = 32, 64 and 128 against the route it replaces for a head dimension without kernels, the
``_reference`` expression of cloud_amd/ops/attention.py (fp32 head split, ``[B, H, S, S]`` scores
from library GEMMs, softmax, ``F.dropout``, GEMM with V).  Equal width H*D = 768 (H = 24 / 12 / 6),
B = 8, S = 512 and 2048, self-attention non-causal and causal, attention dropout 0.1, forward and
forward+backward per call.  D = 64 is the control: its kernels predate the other two.

    python bench/attn_head_dim.py
    python bench/attn_head_dim.py --dims 128 --seqs 2048 --repeats 7

Both routes run in the same process on the same bf16 projection ``qkv [B, S, 3*H*D]``; the
projection itself is outside the timed region.  The reference route is timed twice per shape, in
two separate sets of windows (A/A): the relative difference of the two medians is the noise a
ratio has to exceed.  ``native_wins`` of a shape says that the reference median (the faster of the
two) divided by the native median is above 1 + that A/A spread, forward and forward+backward; a
head dimension stays routed to the kernels (``raw.ATTN_HEAD_DIMS``) only if every shape says so.

Timing as in bench/attn_cross.py: device events around ``--iters`` back-to-back calls on one
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
    ap.add_argument("--dims", default="32,64,128", help="head dimensions, comma separated")
    ap.add_argument("--seqs", default="512,2048", help="sequence lengths, comma separated")
    ap.add_argument("--width", type=int, default=768, help="H * D")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    return ap.parse_args()


def main():
    args = parse()
    import torch

    from cloud_amd.ops import raw
    from cloud_amd.ops.attention import _AttentionFn, _reference

    if not torch.cuda.is_available():
        sys.exit("attn_head_dim: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    p, B = args.p, args.batch

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

    def measure(route, qkv, dctx):
        def fwd():
            with torch.no_grad():
                return route(qkv)

        def fwd_bwd():
            qkv.grad = None
            route(qkv).backward(dctx)

        return {"fwd": windows(fwd), "fwd_bwd": windows(fwd_bwd)}

    results = []
    for D in [int(v) for v in args.dims.split(",") if v]:
        H = args.width // D
        scale = 1.0 / math.sqrt(D)
        for S in [int(v) for v in args.seqs.split(",") if v]:
            for causal in (False, True):
                g = torch.Generator(device=dev).manual_seed(D + S)
                qkv = (torch.randn(B, S, 3 * H * D, device=dev, generator=g) * 0.5).to(torch.bfloat16).requires_grad_()
                dctx = torch.randn(B, S, H * D, device=dev, generator=g).to(torch.bfloat16)

                def native(x):
                    # what ops.attention runs for a routed head dim; called directly, so that a head dim
                    # taken out of raw.ATTN_HEAD_DIMS stays measurable
                    return _AttentionFn.apply(x, None, H, scale, p, 1234, causal)

                def reference(x):
                    return _reference(x, H, None, scale, p, causal)

                routed = D in raw.ATTN_HEAD_DIMS
                row = {"D": D, "H": H, "B": B, "S": S, "causal": causal, "p": p, "routed_to_kernels": bool(routed),
                       "kernels": measure(native, qkv, dctx), "reference": measure(reference, qkv, dctx),
                       "reference_again": measure(reference, qkv, dctx)}
                row["aa_spread"], row["reference_over_kernels"] = {}, {}
                wins = True
                for k in ("fwd", "fwd_bwd"):
                    a, b = row["reference"][k]["median_us"], row["reference_again"][k]["median_us"]
                    aa = max(a, b) / min(a, b) - 1.0
                    ratio = min(a, b) / row["kernels"][k]["median_us"]
                    row["aa_spread"][k] = round(aa, 4)
                    row["reference_over_kernels"][k] = round(ratio, 2)
                    wins = wins and ratio > 1.0 + aa
                row["native_wins"] = wins
                print(json.dumps(row), flush=True)
                results.append(row)
                del qkv, dctx
                torch.cuda.empty_cache()
    verdict = {}
    for r in results:
        verdict[r["D"]] = verdict.get(r["D"], True) and r["native_wins"]
    print(json.dumps({"metric": "self-attention time per call by head dimension, in-tree kernels and the PyTorch "
                                "reference route", "unit": "us", "iters": args.iters, "repeats": args.repeats,
                      "device": torch.cuda.get_device_name(0),
                      "native_wins_every_shape": {str(d): v for d, v in verdict.items()},
                      "shapes": {f"D{r['D']}xS{r['S']}x{'causal' if r['causal'] else 'full'}":
                                 {"kernels": {k: r["kernels"][k]["median_us"] for k in ("fwd", "fwd_bwd")},
                                  "reference": {k: r["reference"][k]["median_us"] for k in ("fwd", "fwd_bwd")},
                                  "reference_over_kernels": r["reference_over_kernels"], "aa_spread": r["aa_spread"]}
                                 for r in results}}), flush=True)


if __name__ == "__main__":
    main()
