#!/usr/bin/env python3
"""ResNet-50 inference paths on one MI355X, fused against the per-layer route.

Two workloads, bf16, 224 x 224, batch 256 by default, timed with device events after warmup:

* ``eval_forward``: ``ResNet-50.eval()`` forward under ``torch.no_grad()``;
* ``frozen_fit_step``: one ``fit`` step of a Keras model with a frozen ``ResNet50`` base and a
  trainable GlobalAveragePooling -> Dense(10) head (base forward in inference mode, head forward,
  loss, head backward, optimizer).

Each is measured with ``CLOUD_AMD_INFER_FUSE=1`` (every BatchNorm in the epilogue of its
convolution) and ``=0`` (convolution with statistics partials, then ``bn_apply``: the route
before the switch existed), in fresh child processes, alternated ``--rounds`` times (>= 3) in one
call, so the two settings see the same box state.  One JSON line per child measurement, then one
summary line per workload: medians, the A/A spread of each setting ((max - min) / median over
its rounds) and the speedup of the medians.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time_ms(fn, steps, warmup):
    import torch

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(steps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / steps


def child(a):
    import torch

    from cloud_amd import config
    from cloud_amd.ops import _ext

    _ext.load(required=True)
    dev = torch.device("cuda", 0)
    fuse = int(bool(config.get("CLOUD_AMD_INFER_FUSE")))
    torch.manual_seed(0)
    B, S = a.batch, a.image

    if a.what in ("all", "eval_forward"):
        from cloud_amd.models import resnet50

        model = resnet50(num_classes=1000, dtype=torch.bfloat16, device=dev).eval()
        x = torch.randn(B, S, S, 3, device=dev).to(torch.bfloat16)

        def fwd():
            with torch.no_grad():
                return model(x)

        ms = _time_ms(fwd, a.steps, a.warmup)
        print(json.dumps({"workload": "eval_forward", "infer_fuse": fuse, "batch": B, "image": S, "ms": round(ms, 3),
                          "img_per_s": round(B / ms * 1e3, 1)}), flush=True)
        del model, x
        torch.cuda.empty_cache()

    if a.what in ("all", "frozen_fit_step"):
        from cloud_amd import tf
        from cloud_amd.keras import engine

        engine.set_global_policy("mixed_bfloat16")
        base = tf.keras.applications.ResNet50(include_top=False, weights=None, input_shape=(S, S, 3))
        base.trainable = False
        model = tf.keras.Sequential([base, tf.keras.layers.GlobalAveragePooling2D(), tf.keras.layers.Dense(10)])
        model.compile(optimizer=tf.keras.optimizers.SGD(learning_rate=0.01, momentum=0.9),
                      loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True))
        x = torch.randn(B, S, S, 3).to(torch.bfloat16)
        y = torch.randint(0, 10, (B,))
        model.train_on_batch(x, y)  # builds, binds the optimizer, moves the model to the device
        xd, yd = x.to(dev), y.to(dev)
        assert len(model.trainable_weights) == 2

        def step():
            model.train_step(xd, yd)

        ms = _time_ms(step, a.steps, a.warmup)
        print(json.dumps({"workload": "frozen_fit_step", "infer_fuse": fuse, "batch": B, "image": S,
                          "ms": round(ms, 3), "img_per_s": round(B / ms * 1e3, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--image", type=int, default=224)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternations of the two settings (>= 3)")
    ap.add_argument("--what", default="all", choices=["all", "eval_forward", "frozen_fit_step"])
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    rows = []
    for r in range(a.rounds):
        for fuse in ((1, 0) if r % 2 == 0 else (0, 1)):  # ABBA order
            env = dict(os.environ, CLOUD_AMD_INFER_FUSE=str(fuse))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--batch", str(a.batch),
                   "--image", str(a.image), "--steps", str(a.steps), "--warmup", str(a.warmup), "--what", a.what]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"child (CLOUD_AMD_INFER_FUSE={fuse}) failed with status {p.returncode}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    row = dict(json.loads(line), round=r)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
    for wl in sorted({r["workload"] for r in rows}):
        t = {f: [r["ms"] for r in rows if r["workload"] == wl and r["infer_fuse"] == f] for f in (0, 1)}
        med = {f: statistics.median(v) for f, v in t.items()}
        spread = {f: (max(v) - min(v)) / med[f] for f, v in t.items()}
        print(json.dumps({"summary": wl, "batch": a.batch, "rounds": a.rounds,
                          "fused_ms": round(med[1], 3), "per_layer_ms": round(med[0], 3),
                          "fused_spread": round(spread[1], 4), "per_layer_spread": round(spread[0], 4),
                          "speedup": round(med[0] / med[1], 4)}), flush=True)


if __name__ == "__main__":
    main()
