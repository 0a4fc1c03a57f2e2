#!/usr/bin/env python3
"""LayerNorm at any width: ``ops.layer_norm`` on the HIP kernels (csrc/kernels/layernorm.hip;
rowops.hip for ``C % 4 == 0``, ``C <= 1344``) against the route ``keras.layers.
LayerNormalization`` ran before it, ``F.layer_norm(x.float(), (C,), gamma, beta, eps).to(bf16)``
with autograd, forward and forward + backward per call, on bf16 ``x [M, C]`` with fp32
``gamma`` / ``beta`` that take gradients:

    python bench/layer_norm.py
    python bench/layer_norm.py --shapes 8192x768,8192x1001 --repeats 9

Both routes run in the same process on the same tensors.  Timing: device events around
``--iters`` back-to-back calls on one stream, after a warm-up; ``--repeats`` rounds, each round
timing native, library, native again, so the two native series (A/A) bracket the library one and
their disagreement is the noise floor of the comparison.  Reported per call: the median window and
the spread (min .. max) of each series in microseconds, ``aa_spread`` = |median A1 - median A2| /
min of the two, and ``native_over_library`` = median of all native windows / library median.

Bytes are what the algorithm needs, from the shape: forward reads x and writes y (4 B per
element), backward reads dy and the saved x and writes dx (6 B per element); gamma, beta, the row
statistics and the gradient partials are left out.  ``gbps`` = those bytes over the native median
(forward: 4 B; forward + backward: 10 B per element).  The tensors of every listed shape fit the
256 MiB last-level cache, so back-to-back calls are served from it in part: the rate is that of
this loop, not an HBM figure.  One JSON line per shape, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "8192x768,8192x1024,8192x2048,4096x4096,2048x8192,1024x16384,8192x1001"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="MxC, comma separated")
    ap.add_argument("--eps", type=float, default=1e-3)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    return ap.parse_args()


def main():
    args = parse()
    import torch
    import torch.nn.functional as F

    from cloud_amd.ops import layer_norm

    if not torch.cuda.is_available():
        sys.exit("layer_norm: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    eps = args.eps

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

    def compare(native, library):
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
        return {"native": sa, "native_a1": s1, "native_a2": s2, "library": sl,
                "aa_spread": round(abs(s1["median_us"] - s2["median_us"]) / min(s1["median_us"], s2["median_us"]), 4),
                "native_over_library": round(sa["median_us"] / sl["median_us"], 3)}

    results = []
    for shape in [s for s in args.shapes.split(",") if s]:
        M, C = (int(v) for v in shape.split("x"))
        g = torch.Generator(device=dev).manual_seed(M + C)
        x = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16).requires_grad_()
        dy = torch.randn(M, C, device=dev, generator=g).to(torch.bfloat16)
        gamma = (torch.randn(C, device=dev, generator=g) * 0.5 + 1).requires_grad_()
        beta = (torch.randn(C, device=dev, generator=g) * 0.1).requires_grad_()

        def native():
            return layer_norm(x, gamma, beta, eps)

        def library():
            return F.layer_norm(x.float(), (C,), gamma, beta, eps).to(x.dtype)

        def fwd(route):
            def f():
                with torch.no_grad():
                    route()
            return f

        def fwd_bwd(route):
            def f():
                x.grad = gamma.grad = beta.grad = None
                route().backward(dy)
            return f

        row = {"M": M, "C": C, "bytes_fwd": 4 * M * C, "bytes_bwd": 6 * M * C,
               "fwd": compare(fwd(native), fwd(library)), "fwd_bwd": compare(fwd_bwd(native), fwd_bwd(library))}
        row["fwd"]["gbps"] = round(row["bytes_fwd"] / row["fwd"]["native"]["median_us"] / 1e3, 1)
        row["fwd_bwd"]["gbps"] = round((row["bytes_fwd"] + row["bytes_bwd"]) / row["fwd_bwd"]["native"]["median_us"] / 1e3, 1)
        print(json.dumps(row), flush=True)
        results.append(row)
    print(json.dumps({"metric": "LayerNorm time per call: ops.layer_norm on the HIP kernels against "
                                "F.layer_norm(x.float()).to(bf16) with autograd", "unit": "us",
                      "iters": args.iters, "repeats": args.repeats, "device": torch.cuda.get_device_name(0),
                      "shapes": {f"{r['M']}x{r['C']}": {k: {"native": r[k]["native"]["median_us"],
                                                            "library": r[k]["library"]["median_us"],
                                                            "native_over_library": r[k]["native_over_library"],
                                                            "aa_spread": r[k]["aa_spread"], "gbps": r[k]["gbps"]}
                                                        for k in ("fwd", "fwd_bwd")} for r in results}}), flush=True)


if __name__ == "__main__":
    main()
