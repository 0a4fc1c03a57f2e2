#!/usr/bin/env python3
"""Softmax cross-entropy at vocabulary width: ``ops.softmax_cross_entropy`` on the
one-row-per-workgroup kernels (csrc/kernels/xent_vocab.hip) against the route the same call
took before them -- the one-wave-per-row kernel of xent.hip with its sum / divide kernels,
reached by putting ``CLOUD_AMD_XENT_VOCAB_MIN_C`` out of reach -- and against
``F.cross_entropy(z.float(), y)`` with autograd.  Forward + backward per call (unit-seed backward
on the two native routes: the stored gradient is handed on), bf16 logits ``[N, C]`` that take a
gradient, int64 labels:

    python bench/xent_vocab.py
    python bench/xent_vocab.py --shapes 8192x32768,4096x50257p7 --repeats 9

A shape ``NxCpP`` is the ``[:, :C]`` view of a ``C + P`` wide buffer (a padded head): the new
route reads it in place, the other two copy it (``.contiguous()`` / ``.float()``), and all three
pay the zero-filled copy of the slice's backward.

All routes run in the same process on the same tensors.  Timing: device events around ``--iters``
back-to-back calls on one stream, after a warm-up; ``--repeats`` rounds, each round timing new,
parent, library, new again, so the two new-route series (A/A) bracket the others and their
disagreement is the noise floor of the comparison.  Reported per call: the median window and the
spread (min .. max) of each series in microseconds, ``aa_spread`` = |median A1 - median A2| / min
of the two, ``new_over_parent`` and ``new_over_library`` = median of all new-route windows over
the other route's median.

Bytes are what the algorithm needs, from the shape: one read and one write of the logits (4 B per
bf16 element); labels and the per-row outputs are left out.  ``gbps`` = those bytes over the
median.  A shape whose logits and gradient fit the 256 MiB last-level cache is served from it in
part between back-to-back calls: the rate is that of this loop, not an HBM figure.  One JSON line
per shape, then one summary line.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = "8192x4096,8192x8192,8192x32768,4096x50257,4096x50257p7,2048x131072,1024x1000"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="NxC or NxCpP (P padding columns), comma separated")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    return ap.parse_args()


def main():
    args = parse()
    import torch
    import torch.nn.functional as F

    from cloud_amd.ops import losses

    if not torch.cuda.is_available():
        sys.exit("xent_vocab: needs a GPU (a CPU run measures nothing)")
    dev = torch.device("cuda", 0)
    seed = losses.unit_seed(dev)
    out_of_reach = 1 << 31

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

    results = []
    for shape in [s for s in args.shapes.split(",") if s]:
        N, rest = shape.split("x")
        C, _, pad = rest.partition("p")
        N, C, pad = int(N), int(C), int(pad or 0)
        g = torch.Generator(device=dev).manual_seed(N + C)
        leaf = (torch.randn(N, C + pad, device=dev, generator=g) * 3).to(torch.bfloat16).requires_grad_()
        y = torch.randint(0, C, (N,), device=dev, generator=g)

        def logits():
            return leaf[:, :C] if pad else leaf

        def native(min_c):
            def f():
                leaf.grad = None
                losses._VOCAB_MIN_C = min_c
                loss, _ = losses.softmax_cross_entropy(logits(), y)
                losses.backward_with_seed(loss, seed)
            return f

        def library():
            leaf.grad = None
            F.cross_entropy(logits().float(), y).backward()

        default = losses._VOCAB_MIN_C
        new, parent = native(1), native(out_of_reach)
        try:
            # the two native routes agree (same formula; sums in another order)
            new()
            g_new, l_new = leaf.grad.clone(), losses.softmax_cross_entropy(logits(), y)[0].item()
            parent()
            g_par, l_par = leaf.grad.clone(), losses.softmax_cross_entropy(logits(), y)[0].item()
            same = bool(abs(l_new - l_par) <= 1e-4 * abs(l_par)
                        and torch.allclose(g_new.float(), g_par.float(), rtol=2e-2, atol=2e-2 / N))
            del g_new, g_par
            for fn in (new, parent, library):
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            a1, par, lib, a2 = [], [], [], []
            for _ in range(args.repeats):
                a1.append(window(new))
                par.append(window(parent))
                lib.append(window(library))
                a2.append(window(new))
        finally:
            losses._VOCAB_MIN_C = default
        s1, s2, sp, sl, sa = stats(a1), stats(a2), stats(par), stats(lib), stats(a1 + a2)
        nbytes = 4 * N * C
        row = {"N": N, "C": C, "pad": pad, "bytes": nbytes, "new": sa, "new_a1": s1, "new_a2": s2, "parent": sp,
               "library": sl, "routes_agree": same,
               "aa_spread": round(abs(s1["median_us"] - s2["median_us"]) / min(s1["median_us"], s2["median_us"]), 4),
               "new_over_parent": round(sa["median_us"] / sp["median_us"], 3),
               "new_over_library": round(sa["median_us"] / sl["median_us"], 3),
               "gbps": {k: round(nbytes / v["median_us"] / 1e3, 1) for k, v in (("new", sa), ("parent", sp), ("library", sl))}}
        print(json.dumps(row), flush=True)
        results.append(row)
        del leaf, y
        torch.cuda.empty_cache()
    print(json.dumps({"metric": "softmax cross-entropy forward + backward per call: the xent_vocab.hip route against "
                                "the one-wave-per-row route and F.cross_entropy(z.float(), y) with autograd",
                      "unit": "us", "iters": args.iters, "repeats": args.repeats,
                      "device": torch.cuda.get_device_name(0),
                      "shapes": {f"{r['N']}x{r['C']}" + (f"p{r['pad']}" if r["pad"] else ""):
                                 {"new": r["new"]["median_us"], "parent": r["parent"]["median_us"],
                                  "library": r["library"]["median_us"], "new_over_parent": r["new_over_parent"],
                                  "new_over_library": r["new_over_library"], "aa_spread": r["aa_spread"],
                                  "gbps": r["gbps"], "routes_agree": r["routes_agree"]} for r in results}}), flush=True)


if __name__ == "__main__":
    main()
