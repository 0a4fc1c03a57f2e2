#!/usr/bin/env python3
"""Max / average pooling on the any-window kernels (csrc/kernels/pool2d.hip) against the routes
the Keras layers took before them, at real layer shapes, NHWC bf16:

    python bench/pool_shapes.py
    python bench/pool_shapes.py --cases inception-3x3s1-same,lenet-c6 --out rows.jsonl

Cases (name: N x H x W x C, window / stride, padding -- and the earlier route):

    mnist-2x2           128x26x26x32   max 2x2 / 2 valid   pool.hip's square max pool.  ops still sends this
                                                           form there; pool2d.hip is timed through its raw
                                                           launchers and an autograd node of this file
    inception-3x3s1     32x28x28x192   max 3x3 / 1 same    F.pad(-inf) copy, then pool.hip
    densenet-avg        32x56x56x128   avg 2x2 / 2 valid   permute, F.avg_pool2d, permute + contiguous
    lenet-c6            128x28x28x6    max 2x2 / 2 valid   C % 8 != 0: permute, F.max_pool2d, permute + contiguous
    rgb-halve           64x224x224x3   avg 2x2 / 2 valid   C % 8 != 0 at a size the GPU, not the host, bounds:
                                                           permute, F.avg_pool2d, permute + contiguous
    rect-2x3            32x28x28x64    max 2x3 / 2x3 valid no earlier route computed it (absolute figures only)
    inception-avg-same  32x35x35x288   avg 3x3 / 1 same    no earlier route computed it (absolute figures only)

Per case, forward (under no_grad) and forward + backward (``torch.autograd.grad`` of the output
against a fixed dy) are timed apart, both routes in the same process on the same tensors.  The
outputs and input gradients of the two routes are compared first (``same``: max pools bitwise,
average pools within one bf16 rounding).

Timing: device events around ``--iters`` back-to-back calls on one stream after ``--warmup`` calls;
``--repeats`` rounds, each timing new, earlier, new again, so the two new series (A/A) bracket the
earlier one and their disagreement is the noise floor.  These are times per call as a training step
sees them: where the kernels take a few microseconds, the window measures the host's dispatch (the
ops' Python against one ATen call) and not the GPU.  Kernel durations come from a run of this
script under ``rocprofv3 --kernel-trace --stats`` (a run of its own: tracing slows the host).

Bytes are the least each pass must move, from the shapes: forward reads x and writes y (2 B per
element) plus, for max, the argmax byte per output element; the backward reads dy (and the argmax
bytes) and writes dx.  ``gbps`` = those bytes over the new route's median.  Tensors up to the
256 MiB last-level cache are served from it in part in back-to-back calls: the rates are those of
this loop, not HBM figures.  One JSON line per case, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

#         name                  kind   N    H   W   C    k       s       padding  earlier route
CASES = [("mnist-2x2",          "max", 128, 26, 26, 32,  (2, 2), (2, 2), "valid", "pool.hip"),
         ("inception-3x3s1",    "max", 32,  28, 28, 192, (3, 3), (1, 1), "same",  "pad+pool.hip"),
         ("densenet-avg",       "avg", 32,  56, 56, 128, (2, 2), (2, 2), "valid", "permute+F.avg_pool2d"),
         ("lenet-c6",           "max", 128, 28, 28, 6,   (2, 2), (2, 2), "valid", "permute+F.max_pool2d"),
         ("rgb-halve",          "avg", 64,  224, 224, 3, (2, 2), (2, 2), "valid", "permute+F.avg_pool2d"),
         ("rect-2x3",           "max", 32,  28, 28, 64,  (2, 3), (2, 3), "valid", None),
         ("inception-avg-same", "avg", 32,  35, 35, 288, (3, 3), (1, 1), "same",  None)]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(c[0] for c in CASES), help="case names, comma separated")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    return ap.parse_args()


def main():
    args = parse()
    import torch
    import torch.nn.functional as F

    from cloud_amd import ops
    from cloud_amd.ops import raw

    if not torch.cuda.is_available():
        sys.exit("pool_shapes: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.iters

    def stats(w):
        w = sorted(w)
        return {"median_us": round(w[len(w) // 2], 2), "min_us": round(w[0], 2), "max_us": round(w[-1], 2)}

    def measure(new, earlier, nbytes):
        for fn in (new, earlier):
            if fn is not None:
                for _ in range(args.warmup):
                    fn()
        torch.cuda.synchronize()
        a1, old, a2 = [], [], []
        for _ in range(args.repeats):
            a1.append(window(new))
            if earlier is not None:
                old.append(window(earlier))
            a2.append(window(new))
        s1, s2, sa = stats(a1), stats(a2), stats(a1 + a2)
        row = {"new": sa, "aa_spread": round(abs(s1["median_us"] - s2["median_us"]) /
                                             min(s1["median_us"], s2["median_us"]), 4),
               "bytes": nbytes, "gbps": round(nbytes / sa["median_us"] / 1e3, 1)}
        if earlier is not None:
            row["earlier"] = stats(old)
            row["new_over_earlier"] = round(sa["median_us"] / row["earlier"]["median_us"], 3)
        return row

    class RawMax(torch.autograd.Function):
        """pool2d.hip's max pool as an autograd node, for the one case ops keeps on pool.hip."""

        @staticmethod
        def forward(ctx, x, k, s, pads, out_hw):
            y, idx = raw.pool2d_max_fwd(x, k, s, pads, out_hw)
            ctx.save_for_backward(idx)
            ctx.cfg = (tuple(x.shape), k, s, pads)
            return y

        @staticmethod
        def backward(ctx, dy):
            return raw.pool2d_max_bwd(dy.contiguous(), *ctx.saved_tensors, *ctx.cfg), None, None, None, None

    results = []
    wanted = [c for c in args.cases.split(",") if c]
    for name, kind, N, H, W, C, k, s, padding, earlier_name in CASES:
        if name not in wanted:
            continue
        if padding == "same":
            out_hw = (math.ceil(H / s[0]), math.ceil(W / s[1]))
            tot = [max((o - 1) * st + kk - n, 0) for o, st, kk, n in zip(out_hw, s, k, (H, W))]
            pads = ((tot[0] // 2, tot[0] - tot[0] // 2), (tot[1] // 2, tot[1] - tot[1] // 2))
        else:
            out_hw = ((H - k[0]) // s[0] + 1, (W - k[1]) // s[1] + 1)
            pads = ((0, 0), (0, 0))
        g = torch.Generator(device=dev).manual_seed(H * C + k[0])
        x = torch.randn(N, H, W, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
        dy = torch.randn(N, *out_hw, C, device=dev, generator=g).to(torch.bfloat16)
        top_left = (pads[0][0], pads[1][0])

        if name == "mnist-2x2":  # ops sends this form to pool.hip: reach pool2d.hip directly
            def new(t):
                return RawMax.apply(t, k, s, top_left, out_hw)
        elif kind == "max":
            def new(t):
                return ops.max_pool2d_nhwc(t, k, s, pads, out_hw=out_hw)
        else:
            def new(t):
                return ops.avg_pool2d_nhwc(t, k, s, pads, out_hw=out_hw)

        earlier = None
        if earlier_name == "pool.hip":
            def earlier(t):
                return ops.max_pool2d_nhwc(t, k[0], s[0], 0)
        elif earlier_name == "pad+pool.hip":
            def earlier(t):
                (pt, pb), (pl, pr) = pads
                return ops.max_pool2d_nhwc(F.pad(t, (0, 0, pl, pr, pt, pb), value=float("-inf")).contiguous(),
                                           k[0], s[0], 0)
        elif earlier_name == "permute+F.avg_pool2d":
            def earlier(t):
                return F.avg_pool2d(t.permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1).contiguous()
        elif earlier_name == "permute+F.max_pool2d":
            def earlier(t):
                return F.max_pool2d(t.permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1).contiguous()

        def fwd(route):
            def f():
                with torch.no_grad():
                    route(x)
            return f

        def fwd_bwd(route):
            return lambda: torch.autograd.grad(route(x), x, dy)

        same = None
        if earlier is not None:  # faster and different is not faster
            yn, yo = new(x), earlier(x)
            (dn,), (do,) = torch.autograd.grad(yn, x, dy), torch.autograd.grad(yo, x, dy)
            if kind == "max":
                same = bool(torch.equal(yn, yo) and torch.equal(dn, do))
            else:
                same = bool(((yn.float() - yo.float()).abs() <= 2.0 ** -7 * yo.float().abs()).all()
                            and ((dn.float() - do.float()).abs() <= 2.0 ** -7 * do.float().abs()).all())
        side = 1 if kind == "max" else 0  # the argmax byte per output element
        nb_f = 2 * (x.numel() + dy.numel()) + side * dy.numel()
        nb_fb = nb_f + 2 * (x.numel() + dy.numel()) + side * dy.numel()
        row = {"case": name, "kind": kind, "N": N, "H": H, "W": W, "C": C, "window": list(k), "stride": list(s),
               "padding": padding, "earlier_route": earlier_name, "same": same,
               "fwd": measure(fwd(new), fwd(earlier) if earlier else None, nb_f),
               "fwd_bwd": measure(fwd_bwd(new), fwd_bwd(earlier) if earlier else None, nb_fb)}
        emit(row)
        results.append(row)
    emit({"metric": "pooling time per call: pool2d.hip against the earlier route of each Keras layer, NHWC bf16",
          "unit": "us", "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
          "cases": {r["case"]: {p: {"new": r[p]["new"]["median_us"],
                                    "earlier": r[p].get("earlier", {}).get("median_us"),
                                    "new_over_earlier": r[p].get("new_over_earlier"), "gbps": r[p]["gbps"],
                                    "aa_spread": r[p]["aa_spread"]} for p in ("fwd", "fwd_bwd")}
                    for r in results}})


if __name__ == "__main__":
    main()
