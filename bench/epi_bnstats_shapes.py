"""Input-gradient GEMMs / convolutions that end in the BN-backward statistics epilogue, at the
ResNet-50 shapes (one JSON line per shape and epilogue form, times in us).

    python bench/epi_bnstats_shapes.py [batch] [tag]

1x1 input gradients dx[M, N] = dy[M, K] w[K, N] of the four stages' conv1 (N = 4K), forms
  bn       statistics only, beta 0                     (EPI_BF16_BN)
  bn_beta  statistics, dx += old dx                    (EPI_BF16_BN)
  res      statistics, dx += relu'(mask) * src         (EPI_BF16_BNR)
  res_z2   the same with a second BN's statistics      (EPI_BF16_BNR2)
and the stride-1 3x3 input gradients of stages 2-4 with statistics.  CLOUD_AMD_EPI_PIPE=0
selects the one-batch-at-a-time row pass (A/B runs, one process per value).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cloud_amd.ops import raw  # noqa: E402

BF = torch.bfloat16


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1000.0


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    tag = sys.argv[2] if len(sys.argv) > 2 else ""
    dev = "cuda"
    torch.manual_seed(0)
    for stage, (hw, k) in enumerate(((56, 64), (28, 128), (14, 256), (7, 512)), 1):
        n = 4 * k
        shape = (batch, hw, hw, n)
        m = batch * hw * hw
        dy = torch.randn(batch, hw, hw, k, device=dev).to(BF)
        w = (torch.randn(k, 1, 1, n, device=dev) * 0.05).to(BF)
        z, z2, src = (torch.randn(shape, device=dev).to(BF) for _ in range(3))
        mask = torch.randint(0, 256, (m, n // 8), device=dev, dtype=torch.uint8)
        rmask = torch.randint(0, 256, (m, n // 8), device=dev, dtype=torch.uint8)
        out = torch.zeros(shape, device=dev, dtype=BF)
        forms = {
            "bn": lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out, beta=0.0, bn=(z, mask)),
            "bn_beta": lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out, beta=1.0, bn=(z, mask)),
            "res": lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out, beta=1.0, bn=(z, mask), res=(src, rmask)),
            "res_z2": lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out, beta=1.0, bn=(z, mask, z2),
                                             res=(src, rmask)),
        }
        r = {"tag": tag, "kind": "dgrad1x1", "stage": stage, "M": m, "N": n, "K": k}
        for name, fn in forms.items():
            r[name] = round(timeit(fn), 1)
        print(json.dumps(r), flush=True)
        del dy, w, z, z2, src, mask, rmask, out
    for name, hw, c in (("l2_c2", 28, 128), ("l3_c2", 14, 256), ("l4_c2", 7, 512)):
        shape = (batch, hw, hw, c)
        dy = torch.randn(shape, device=dev).to(BF)
        w = (torch.randn(c, 3, 3, c, device=dev) * 0.05).to(BF)
        z = torch.randn(shape, device=dev).to(BF)
        mask = torch.randint(0, 256, (batch * hw * hw, c // 8), device=dev, dtype=torch.uint8)
        t = timeit(lambda: raw.conv_dgrad(dy, w, shape, 1, 1, bn=(z, mask)), iters=10)
        print(json.dumps({"tag": tag, "kind": "dgrad3x3_bn", "shape": name, "us": round(t, 1)}), flush=True)
        del dy, w, z, mask


if __name__ == "__main__":
    main()
