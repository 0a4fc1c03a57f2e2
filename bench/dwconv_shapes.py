#!/usr/bin/env python3
"""Depthwise convolution on the in-tree kernels (csrc/kernels/dwconv.hip) against the library
route, ``F.conv2d(groups=C)`` on channels-last bf16 (MIOpen), at the depthwise layers of
MobileNet, batch 64, 3x3:

    python bench/dwconv_shapes.py
    python bench/dwconv_shapes.py --shapes 56x128x1,14x512x1 --batch 32 --out rows.jsonl

A shape is ``HxCxstride`` (square image, "same" padding as TF splits it).  Per shape the three
passes are timed apart: forward, input gradient, weight gradient -- native through the raw
launchers (``ops.raw.dwconv_fwd / dwconv_dgrad / dwconv_wgrad``, the weight gradient with its
workspace allocation and both launches), library through ``F.conv2d`` and
``aten.convolution_backward`` with one output requested.  Both routes run in the same process on
the same tensors.

Timing: device events around ``--iters`` back-to-back calls on one stream after ``--warmup``
calls; ``--repeats`` rounds, each timing native, library, native again, so the two native series
(A/A) bracket the library one and their disagreement is the noise floor.  The library's first call
of every pass (algorithm search / kernel compilation) is timed on the host clock around a
synchronise and reported apart as ``library_first_call_ms``; it is not part of any window.

Bytes are the least each pass must move, from the shape: forward reads x and writes y, the input
gradient reads dy and writes dx, the weight gradient reads dy and x (2 B per element; weights and
partials left out).  ``gbps`` = those bytes over the native median.  ``elementwise_gbps`` is the
same figure for this tree's elementwise ``act_grad`` kernel (reads two tensors of y's size, writes
one) in the same loop -- the yardstick for "what a streaming kernel reaches here".  Tensors up to
the 256 MiB last-level cache are served from it in part in back-to-back calls: the rates are those
of this loop, not HBM figures.  One JSON line per shape, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "112x32x1,112x64x2,56x128x1,56x128x2,28x256x1,14x512x1,7x1024x1"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="HxCxstride, comma separated")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    return ap.parse_args()


def main():
    args = parse()
    import torch
    import torch.nn.functional as F

    from cloud_amd.ops import raw
    from cloud_amd.ops.dense import _act_grad_dev

    if not torch.cuda.is_available():
        sys.exit("dwconv_shapes: needs a GPU (a CPU run measures nothing)")
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

    def first_call_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 1)

    def compare(native, library, nbytes):
        first = first_call_ms(library)
        for fn in (native, library):
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        a1, lib, a2 = [], [], []
        for _ in range(args.repeats):
            a1.append(window(native))
            lib.append(window(library))
            a2.append(window(native))
        s1, s2, sl, sa = stats(a1), stats(a2), stats(lib), stats(a1 + a2)
        return {"native": sa, "library": sl, "library_first_call_ms": first,
                "aa_spread": round(abs(s1["median_us"] - s2["median_us"]) / min(s1["median_us"], s2["median_us"]), 4),
                "native_over_library": round(sa["median_us"] / sl["median_us"], 3),
                "bytes": nbytes, "gbps": round(nbytes / sa["median_us"] / 1e3, 1)}

    results = []
    for shape in [s for s in args.shapes.split(",") if s]:
        H, C, s = (int(v) for v in shape.split("x"))
        N, K = args.batch, 3
        OH = -(-H // s)
        tot = max((OH - 1) * s + K - H, 0)
        pt, pb = tot // 2, tot - tot // 2
        g = torch.Generator(device=dev).manual_seed(H * C + s)
        x = torch.randn(N, H, H, C, device=dev, generator=g).to(torch.bfloat16)
        w = (torch.randn(K, K, C, 1, device=dev, generator=g) / K).to(torch.bfloat16)
        dy = torch.randn(N, OH, OH, C, device=dev, generator=g).to(torch.bfloat16)
        y = torch.empty_like(dy)
        dx = torch.empty_like(x)
        dw = torch.empty(K, K, C, 1, device=dev)
        # library operands: NCHW views with channels-last strides; TF's split as an explicit pad
        # only where it is asymmetric (stride 2 on an even image), as a caller of F.conv2d must
        xl = x.permute(0, 3, 1, 2)
        if pt != pb:
            xl = F.pad(xl, (pt, pb, pt, pb)).contiguous(memory_format=torch.channels_last)
        lpad = 0 if pt != pb else pt
        wl = w.permute(2, 3, 0, 1).reshape(C, 1, K, K).contiguous(memory_format=torch.channels_last)
        dyl = dy.permute(0, 3, 1, 2)

        def lib_bwd(mask):
            return lambda: torch.ops.aten.convolution_backward(dyl, xl, wl, None, [s, s], [lpad, lpad], [1, 1], False,
                                                               [0, 0], C, mask)

        nb = 2 * (x.numel() + dy.numel())
        row = {"N": N, "H": H, "W": H, "C": C, "kernel": K, "stride": s, "pads": [pt, pb],
               "fwd": compare(lambda: raw.dwconv_fwd(x, w, (s, s), (pt, pt), (OH, OH), out=y),
                              lambda: F.conv2d(xl, wl, None, s, lpad, 1, C), nb),
               "dgrad": compare(lambda: raw.dwconv_dgrad(dy, w, x.shape, (s, s), (pt, pt), out=dx),
                                lib_bwd([True, False, False]), nb),
               "wgrad": compare(lambda: raw.dwconv_wgrad(dy, x, w.shape, (s, s), (pt, pt), out=dw),
                                lib_bwd([False, True, False]), nb)}
        # the elementwise yardstick on y's size: 3 tensors x 2 B per element
        dy2, y2 = dy.view(-1, C), y.view(-1, C)
        for _ in range(args.warmup):
            _act_grad_dev(dy2, y2, C, C, "relu")
        ew = stats([window(lambda: _act_grad_dev(dy2, y2, C, C, "relu")) for _ in range(args.repeats)])
        row["elementwise_us"] = ew["median_us"]
        row["elementwise_gbps"] = round(6 * dy.numel() / ew["median_us"] / 1e3, 1)
        emit(row)
        results.append(row)
    emit({"metric": "depthwise 3x3 convolution time per call: dwconv.hip against F.conv2d(groups=C) channels-last bf16",
          "unit": "us", "batch": args.batch, "iters": args.iters, "repeats": args.repeats,
          "device": torch.cuda.get_device_name(0),
          "shapes": {f"{r['H']}x{r['C']}s{r['stride']}": {
              k: {"native": r[k]["native"]["median_us"], "library": r[k]["library"]["median_us"],
                  "native_over_library": r[k]["native_over_library"], "gbps": r[k]["gbps"],
                  "library_first_call_ms": r[k]["library_first_call_ms"]} for k in ("fwd", "dgrad", "wgrad")}
              for r in results}})


if __name__ == "__main__":
    main()
