"""Pooling at any window on the PyTorch route (CPU): ``ops.max_pool2d_nhwc`` / ``ops.avg_pool2d_nhwc``
argument forms, the Keras 2D layers' rectangular windows and "same" geometry, the four 1D layers
and the example workload.

Every reference is a float64 loop over windows and taps (no library pooling): the maximum over the
in-image taps, and the mean over the in-image taps -- padding is excluded from the divisor, as
TF's ``AveragePooling2D`` does.  float32 outputs are compared at 1e-6 (a mean of <= 15 float32
values; maxima are exact).
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cloud_amd import keras, ops, tf
from cloud_amd.keras import layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(n, k, s):
    """(pad before, output size) of TF's "same" on one axis."""
    o = math.ceil(n / s)
    return max((o - 1) * s + k - n, 0) // 2, o


def _ref(x, kind, k, s, pads, out_hw):
    """float64 pooling of x [N, H, W, C] window by window: ``pads`` = (top, left), taps outside the
    image are skipped.  Differentiable (built from indexing, max and mean)."""
    N, H, W, C = x.shape
    rows = []
    for oh in range(out_hw[0]):
        cols = []
        for ow in range(out_hw[1]):
            taps = [x[:, h, w] for h in range(oh * s[0] - pads[0], oh * s[0] - pads[0] + k[0]) if 0 <= h < H
                    for w in range(ow * s[1] - pads[1], ow * s[1] - pads[1] + k[1]) if 0 <= w < W]
            t = torch.stack(taps)
            cols.append(t.amax(0) if kind == "max" else t.sum(0) / len(taps))
        rows.append(torch.stack(cols, 1))
    return torch.stack(rows, 1)


def test_max_pooling2d_rectangular_window():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 7, 10, 4, generator=g)
    y = layers.MaxPooling2D((2, 3))(x)
    assert tuple(y.shape) == (2, 3, 3, 4)
    assert torch.equal(y.double(), _ref(x.double(), "max", (2, 3), (2, 3), (0, 0), (3, 3)))
    # "same": H 7 -> 4 with 2 / 2 pads 0 | 1 (asymmetric), W 10 -> 4 with 3 / 3 pads 1 | 1
    y = layers.MaxPooling2D((2, 3), strides=(2, 3), padding="same")(x)
    assert tuple(y.shape) == (2, 4, 4, 4)
    assert torch.equal(y.double(), _ref(x.double(), "max", (2, 3), (2, 3), (0, 1), (4, 4)))


def test_average_pooling2d_same_divides_by_the_in_image_taps():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 5, 4, 3, generator=g)
    y = layers.AveragePooling2D(3, 2, "same")(x)
    assert tuple(y.shape) == (1, 3, 2, 3)
    # H: 5 -> 3, pads 1 | 1; W: 4 -> 2, pads 0 | 1
    assert (_same(5, 3, 2), _same(4, 3, 2)) == ((1, 3), (0, 2))
    ref = _ref(x.double(), "avg", (3, 3), (2, 2), (1, 0), (3, 2))
    assert (y.double() - ref).abs().max() < 1e-6
    # the corners by hand: top-left reads rows 0..1 x columns 0..2 (6 taps), bottom-right rows 3..4 x column 2..3 (4)
    assert abs(y[0, 0, 0, 0].item() - x[0, 0:2, 0:3, 0].double().mean().item()) < 1e-6
    assert abs(y[0, 2, 1, 0].item() - x[0, 3:5, 2:4, 0].double().mean().item()) < 1e-6
    # "valid" differs (the parent ignored `padding`)
    assert tuple(layers.AveragePooling2D(3, 2, "valid")(x).shape) == (1, 2, 1, 3)


@pytest.mark.parametrize("padding,pads,out_hw", [(1, (1, 1), (3, 3)), ((1, 0), (1, 0), (3, 2)),
                                                 (((0, 1), (1, 0)), (0, 1), (3, 3))])
def test_avg_pool2d_nhwc_padding_forms_and_gradient(padding, pads, out_hw):
    g = torch.Generator().manual_seed(2)
    x = torch.randn(2, 6, 5, 3, generator=g, dtype=torch.float64).requires_grad_()
    dy = torch.randn(2, *out_hw, 3, generator=g, dtype=torch.float64)
    y = ops.avg_pool2d_nhwc(x, (3, 2), (2, 2), padding)
    assert tuple(y.shape) == (2, *out_hw, 3)
    (dx,) = torch.autograd.grad(y, x, dy)
    xr = x.detach().clone().requires_grad_()
    ref = _ref(xr, "avg", (3, 2), (2, 2), pads, out_hw)
    (dxr,) = torch.autograd.grad(ref, xr, dy)
    assert (y.detach() - ref.detach()).abs().max() < 1e-12
    assert (dx - dxr).abs().max() < 1e-12


def test_pool_ops_out_hw_and_pairs():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 8, 3, generator=g)
    for kind, op in (("max", ops.max_pool2d_nhwc), ("avg", ops.avg_pool2d_nhwc)):
        y = op(x, 3, 2, ((0, 1), (0, 1)), out_hw=(4, 4))
        assert tuple(y.shape) == (2, 4, 4, 3)
        assert (y.double() - _ref(x.double(), kind, (3, 3), (2, 2), (0, 0), (4, 4))).abs().max() < 1e-6
        y = op(x, (2, 3))  # the stride defaults to the window
        assert (y.double() - _ref(x.double(), kind, (2, 3), (2, 3), (0, 0), (4, 2))).abs().max() < 1e-6
    # today's form keeps today's expression
    assert torch.equal(ops.max_pool2d_nhwc(x, 3, 2, 1),
                       torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1))


def test_pooling1d_layers():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 11, 5, generator=g)
    x4 = x.double()[:, None]
    y = layers.MaxPooling1D()(x)
    assert tuple(y.shape) == (3, 5, 5)
    assert torch.equal(y.double(), _ref(x4, "max", (1, 2), (1, 2), (0, 0), (1, 5))[:, 0])
    y = layers.MaxPooling1D(3, 2, "same")(x)  # 11 -> 6, pads 1 | 1
    assert tuple(y.shape) == (3, 6, 5)
    assert torch.equal(y.double(), _ref(x4, "max", (1, 3), (1, 2), (0, 1), (1, 6))[:, 0])
    y = layers.AveragePooling1D(4, 3, "same")(x)  # 11 -> 4, total pad 2: 1 | 1
    assert tuple(y.shape) == (3, 4, 5)
    assert (y.double() - _ref(x4, "avg", (1, 4), (1, 3), (0, 1), (1, 4))[:, 0]).abs().max() < 1e-6
    y = layers.AveragePooling1D(3, strides=1)(x)
    assert tuple(y.shape) == (3, 9, 5)
    assert (y.double() - _ref(x4, "avg", (1, 3), (1, 1), (0, 0), (1, 9))[:, 0]).abs().max() < 1e-6
    y = layers.GlobalAveragePooling1D()(x)
    assert tuple(y.shape) == (3, 5) and (y.double() - x.double().mean(1)).abs().max() < 1e-6
    y = layers.GlobalMaxPooling1D()(x)
    assert tuple(y.shape) == (3, 5) and torch.equal(y, x.amax(1))
    for layer in (layers.GlobalAveragePooling1D(), layers.GlobalMaxPooling1D()):
        with pytest.raises(ValueError):
            layer(x, mask=torch.ones(3, 11, dtype=torch.bool))
    with pytest.raises(ValueError):
        layers.MaxPooling1D(2, padding="causal")


def test_pooling1d_configs_aliases_and_registry():
    for cls, kw in ((layers.MaxPooling1D, dict(pool_size=3, strides=2, padding="same")),
                    (layers.AveragePooling1D, dict(pool_size=4)),
                    (layers.GlobalAveragePooling1D, {}), (layers.GlobalMaxPooling1D, {}),
                    (layers.MaxPooling2D, dict(pool_size=(2, 3), strides=(1, 2), padding="same")),
                    (layers.AveragePooling2D, dict(pool_size=3, strides=2, padding="same"))):
        layer = cls(name="p", **kw)
        cfg = layer.get_config()
        assert cls.from_config(cfg).get_config() == cfg
        assert layers.LAYERS[cls.__name__] is cls
    cfg = layers.MaxPooling1D(3, 2, "same").get_config()
    assert (cfg["pool_size"], cfg["strides"], cfg["padding"]) == ([3], [2], "same")
    assert layers.AveragePooling1D(4).get_config()["strides"] == [4]
    assert layers.MaxPooling2D((2, 3)).get_config()["strides"] == [2, 3]
    assert layers.MaxPool1D is layers.MaxPooling1D and layers.AvgPool1D is layers.AveragePooling1D
    assert layers.GlobalAvgPool1D is layers.GlobalAveragePooling1D
    assert layers.GlobalMaxPool1D is layers.GlobalMaxPooling1D
    assert tf.keras.layers.GlobalAveragePooling1D is layers.GlobalAveragePooling1D
    assert tf.keras.layers.MaxPooling1D is layers.MaxPooling1D


def test_pooled_text_model_saves_and_loads(tmp_path):
    model = keras.Sequential([layers.Embedding(50, 8, input_shape=(12,)), layers.MaxPooling1D(2),
                              layers.AveragePooling1D(3, 1, "same"), layers.GlobalMaxPooling1D(), layers.Dense(3)])
    x = np.random.default_rng(0).integers(0, 50, (4, 12))
    y = model(x)
    assert tuple(y.shape) == (4, 3)
    model.save(str(tmp_path / "m"))
    loaded = keras.models.load_model(str(tmp_path / "m"), compile=False)
    assert [type(l).__name__ for l in loaded.layers] == [type(l).__name__ for l in model.layers]
    assert torch.equal(loaded(x), y)


def test_text_avgpool_example_runs_and_learns(tmp_path):
    """examples/workloads/text_avgpool.py at its small sizes with CLOUD_AMD_OPS=torch on the CPU:
    it prints its RESULT line and the loss falls."""
    env = dict(os.environ)
    env.update({"CLOUD_AMD_EXAMPLE_SMALL": "1", "CLOUD_AMD_OPS": "torch", "CLOUD_AMD_DEVICE": "cpu",
                "CLOUD_AMD_NUM_GPUS": "0",
                "CLOUD_AMD_JOBS_DIR": str(tmp_path / "jobs"), "PYTHONPATH": ROOT})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "workloads", "text_avgpool.py")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1]
    res = dict(kv.split("=") for kv in line.split()[2:])
    assert float(res["loss"]) < float(res["first_loss"]), line
    assert np.isfinite(float(res["eval_acc"]))
