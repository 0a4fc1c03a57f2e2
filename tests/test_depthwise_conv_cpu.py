"""``ops.depthwise_conv2d`` on its PyTorch reference route and the Keras ``DepthwiseConv2D`` /
``SeparableConv2D`` layers on the CPU (float32 policy).

The reference route (``F.conv2d(groups=Cin)``) is checked against an independent formulation: a
DENSE ``F.conv2d`` in float64 whose weight is the block-diagonal expansion of the depthwise
weight, ``Wd[c*DM + m, c, ky, kx] = w[ky, kx, c, m]`` and zero elsewhere -- which pins the
``o = c*DM + m`` channel order without leaning on ``groups=``.  With float64 operands both are
exact up to summation order, so outputs and gradients must agree to 1e-12 of their scale.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cloud_amd import keras, ops
from cloud_amd.keras import layers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _float32_policy():
    from cloud_amd.keras import engine

    old = engine._POLICY
    engine.set_global_policy("float32")
    yield
    engine._POLICY = old


def _dense_expansion(x, w, bias, stride, pads, dilation=(1, 1)):
    """act-free depthwise convolution as a dense convolution over a block-diagonal weight."""
    KH, KW, C, DM = w.shape
    wd = torch.zeros(C * DM, C, KH, KW, dtype=x.dtype)
    for c in range(C):
        for m in range(DM):
            wd[c * DM + m, c] = w[:, :, c, m]
    (pt, pb), (pl, pr) = pads
    xc = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    y = F.conv2d(xc, wd, None, stride, 0, dilation).permute(0, 2, 3, 1)
    return y if bias is None else y + bias


#        N  H  W  C  KH KW  stride   pads                DM  dilation  act     bias
CASES = [(2, 7, 5, 3, 3, 3, (1, 1), ((1, 1), (1, 1)), 1, (1, 1), None, False),
         (2, 8, 8, 4, 3, 3, (2, 2), ((0, 1), (0, 1)), 1, (1, 1), "relu", True),   # TF SAME at stride 2
         (1, 9, 6, 5, 3, 3, (2, 2), ((1, 1), (0, 1)), 3, (1, 1), "tanh", True),   # DM 3, mixed split
         (2, 6, 7, 8, 3, 3, (1, 1), ((1, 1), (1, 1)), 2, (1, 1), "gelu", False),  # DM 2
         (2, 11, 13, 2, 1, 3, (1, 2), ((0, 0), (0, 0)), 1, (1, 1), "elu", True),  # rectangular
         (1, 10, 10, 3, 5, 5, (1, 1), ((2, 2), (2, 2)), 2, (1, 1), "sigmoid", True),  # not fusable
         (1, 9, 9, 3, 3, 3, (1, 1), ((2, 2), (2, 2)), 2, (2, 2), None, True)]     # dilation 2


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c[:6])) + f"-dm{c[8]}-{c[10]}")
def test_reference_route_matches_block_diagonal_dense_conv(case):
    N, H, W, C, KH, KW, stride, pads, DM, dil, act, has_b = case
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64).requires_grad_()
    w = torch.randn(KH, KW, C, DM, generator=g, dtype=torch.float64).requires_grad_()
    b = torch.randn(C * DM, generator=g, dtype=torch.float64).requires_grad_() if has_b else None
    fn = {None: lambda t: t, "relu": torch.relu, "tanh": torch.tanh, "gelu": F.gelu, "elu": F.elu,
          "sigmoid": torch.sigmoid}[act]
    if act == "sigmoid":  # not an epilogue activation: the op refuses nothing, the caller applies it
        y = torch.sigmoid(ops.depthwise_conv2d(x, w, b, stride, pads, None, dilation=dil))
    else:
        y = ops.depthwise_conv2d(x, w, b, stride, pads, act, dilation=dil)
    ref = fn(_dense_expansion(x, w, b, stride, pads, dil))
    assert y.shape == ref.shape and y.shape[-1] == C * DM
    dy = torch.randn(ref.shape, generator=g, dtype=torch.float64)
    ins = [x, w] + ([b] if has_b else [])
    got = torch.autograd.grad(y, ins, dy)
    want = torch.autograd.grad(ref, ins, dy)
    for a, r in zip((y,) + got, (ref,) + want):
        assert (a - r).abs().max() <= 1e-12 * max(1.0, r.abs().max().item())


def test_out_hw_and_padding_forms():
    """``padding`` as an int, an (h, w) pair and ((t, b), (l, r)); ``out_hw`` with top / left pads
    alone gives what the full pads give (rows / columns past the edge read as zero)."""
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 8, 7, 3, generator=g, dtype=torch.float64)
    w = torch.randn(3, 3, 3, 2, generator=g, dtype=torch.float64)
    a = ops.depthwise_conv2d(x, w, None, 1, 1)
    assert torch.equal(a, ops.depthwise_conv2d(x, w, None, (1, 1), (1, 1)))
    assert torch.equal(a, ops.depthwise_conv2d(x, w, None, 1, ((1, 1), (1, 1))))
    full = ops.depthwise_conv2d(x, w, None, 2, ((0, 1), (1, 1)))  # TF SAME of 8x7 at stride 2
    assert full.shape == (2, 4, 4, 6)
    assert torch.equal(full, ops.depthwise_conv2d(x, w, None, 2, ((0, 0), (1, 0)), out_hw=(4, 4)))
    with pytest.raises(ValueError):
        ops.depthwise_conv2d(x, w[:, :, :2], None)


def _tf_same(n, k, s):
    """TF's SAME rule for one axis: output size and (before, after) pads."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, (total // 2, total - total // 2)


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("s", [1, 2, 3])
def test_same_padding_shapes_and_pads(k, s):
    g = torch.Generator().manual_seed(5)
    for H in range(1, 10):
        for W in range(1, 10):
            (oh, ph), (ow, pw) = _tf_same(H, k, s), _tf_same(W, k, s)
            assert layers._same_pads((H, W), (k, k), (s, s)) == [ph, pw]
            assert layers.Conv2D(1, k, strides=s)._same_pads(H, W) == [ph, pw]  # the formula it mirrors
            if (H + W) % 4:  # values on a quarter of the sizes: the shapes above cover all
                continue
            layer = layers.DepthwiseConv2D(k, strides=s, padding="same", use_bias=False)
            x = torch.randn(1, H, W, 2, generator=g)
            y = layer(x)
            assert tuple(y.shape) == (1, oh, ow, 2)
            ref = _dense_expansion(x, layer.depthwise_kernel.detach(), None, (s, s), (ph, pw))
            assert torch.allclose(y, ref, atol=1e-5)


def test_layer_shapes_params_and_glorot_fans():
    x = torch.randn(2, 9, 8, 6)
    dw = layers.DepthwiseConv2D((3, 5), depth_multiplier=2)
    assert tuple(dw(x).shape) == (2, 7, 4, 12)
    assert [tuple(p.shape) for p in dw.parameters()] == [(3, 5, 6, 2), (12,)]
    assert dw.count_params() == 3 * 5 * 6 * 2 + 12
    sep = layers.SeparableConv2D(10, 3, strides=2, padding="same", depth_multiplier=3)
    assert tuple(sep(x).shape) == (2, 5, 4, 10)
    assert [n for n, _ in sep.named_parameters()] == ["depthwise_kernel", "pointwise_kernel", "bias"]
    assert [tuple(p.shape) for p in sep.parameters()] == [(3, 3, 6, 3), (10, 1, 1, 18), (10,)]
    assert sep.count_params() == 3 * 3 * 6 * 3 + 18 * 10 + 10
    nb = layers.SeparableConv2D(4, 3, use_bias=False)
    nb(x)
    assert nb.count_params() == 3 * 3 * 6 + 6 * 4 and nb.bias is None
    # Keras's fans of [kh, kw, cin, dm]: fan_in = kh*kw*cin, fan_out = kh*kw*dm
    big = layers.DepthwiseConv2D(3, depth_multiplier=2, use_bias=False)
    big(torch.zeros(1, 3, 3, 512))
    lim = math.sqrt(6.0 / (9 * 512 + 9 * 2))
    m = big.depthwise_kernel.detach().abs().max().item()
    assert 0.98 * lim < m <= lim
    assert layers.SeparableConvolution2D is layers.SeparableConv2D
    assert layers.LAYERS["DepthwiseConv2D"] is layers.DepthwiseConv2D
    assert layers.LAYERS["SeparableConv2D"] is layers.SeparableConv2D
    from cloud_amd import tf

    assert tf.keras.layers.SeparableConv2D is layers.SeparableConv2D
    assert tf.keras.layers.DepthwiseConv2D is layers.DepthwiseConv2D
    with pytest.raises(ValueError):
        layers.DepthwiseConv2D(3, data_format="channels_first")


def test_config_round_trip_and_weight_order():
    sep = layers.SeparableConv2D(8, (3, 2), strides=(2, 1), padding="same", depth_multiplier=2, activation="relu",
                                 dilation_rate=1, depthwise_regularizer=keras.regularizers.l2(0.01),
                                 pointwise_regularizer=keras.regularizers.l1(0.02), name="sep")
    cfg = sep.get_config()
    assert cfg["filters"] == 8 and cfg["kernel_size"] == [3, 2] and cfg["strides"] == [2, 1]
    assert cfg["depth_multiplier"] == 2 and cfg["padding"] == "same" and cfg["activation"] == "relu"
    again = layers.SeparableConv2D.from_config(cfg)
    assert again.get_config() == cfg
    dw = layers.DepthwiseConv2D(3, depth_multiplier=2, activation="tanh", bias_regularizer="l2", name="dw")
    assert layers.DepthwiseConv2D.from_config(dw.get_config()).get_config() == dw.get_config()

    x = torch.randn(2, 6, 6, 4)
    sep(x)
    again(x)
    ws = sep.get_weights()
    assert [w.shape for w in ws] == [(3, 2, 4, 2), (8, 1, 1, 8), (8,)]
    again.set_weights(ws)
    assert torch.equal(sep(x), again(x))
    with pytest.raises(ValueError):
        again.set_weights(ws[:2])


def test_separable_is_depthwise_then_pointwise():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 9, 6, 5, generator=g)
    sep = layers.SeparableConv2D(7, 3, strides=2, padding="same", depth_multiplier=2, activation="relu")
    dw = layers.DepthwiseConv2D(3, strides=2, padding="same", depth_multiplier=2, use_bias=False)
    pw = layers.Conv2D(7, 1, activation="relu")
    y = sep(x)
    pw(dw(x))
    with torch.no_grad():
        sep.bias.copy_(torch.randn(7, generator=g))
    dw.set_weights(sep.get_weights()[:1])
    pw.set_weights(sep.get_weights()[1:])
    y = sep(x)
    assert tuple(y.shape) == (2, 5, 3, 7)
    assert torch.equal(y, pw(dw(x)))


def test_regularizers_and_frozen_layers():
    x = torch.randn(1, 5, 5, 3)
    sep = layers.SeparableConv2D(4, 3, depthwise_regularizer=keras.regularizers.l2(0.5),
                                 pointwise_regularizer=keras.regularizers.l1(0.25),
                                 bias_regularizer=keras.regularizers.l2(2.0))
    sep(x)
    with torch.no_grad():
        sep.bias.fill_(0.5)
    want = (0.5 * sep.depthwise_kernel.pow(2).sum() + 0.25 * sep.pointwise_kernel.abs().sum()
            + 2.0 * sep.bias.pow(2).sum())
    assert torch.allclose(sep.regularization_loss(), want)
    model = keras.Sequential([layers.DepthwiseConv2D(3, input_shape=(5, 5, 3), depthwise_regularizer="l2"),
                              layers.GlobalAveragePooling2D(), layers.Dense(2)])
    model(x)
    dwl = model.layers[0]
    assert torch.allclose(model._regularization(), 0.01 * dwl.depthwise_kernel.pow(2).sum())
    sep.trainable = False
    assert sep.regularization_loss() == 0.0
    assert not any(p.requires_grad for p in sep.parameters()) and sep.trainable_weights == []
    frozen = layers.DepthwiseConv2D(3, trainable=False)
    frozen(x)
    assert not any(p.requires_grad for p in frozen.parameters())


def test_save_and_load_reproduce_outputs_bit_for_bit(tmp_path):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(3, 8, 8, 3, generator=g)

    def make():
        return keras.Sequential([
            layers.Conv2D(8, 3, padding="same", activation="relu", input_shape=(8, 8, 3)),
            layers.SeparableConv2D(8, 3, padding="same", strides=2, depth_multiplier=2, activation="relu",
                                   depthwise_regularizer="l2"),
            layers.DepthwiseConv2D(3, padding="same", activation="tanh"),
            layers.GlobalAveragePooling2D(), layers.Dense(4)])

    model = make()
    y = model(x)
    with torch.no_grad():  # biases off zero, so their order matters
        for p in model.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g))
    y = model(x)
    model.save(str(tmp_path / "m"))
    loaded = keras.models.load_model(str(tmp_path / "m"), compile=False)
    assert [type(l).__name__ for l in loaded.layers] == [type(l).__name__ for l in model.layers]
    assert loaded.layers[1].get_config() == model.layers[1].get_config()
    assert torch.equal(loaded(x), y)
    model.save_weights(str(tmp_path / "w.pt"))
    other = make()
    other(x)
    assert not torch.equal(other(x), y)
    other.load_weights(str(tmp_path / "w.pt"))
    assert torch.equal(other(x), y)


def test_example_workload_runs_on_the_reference_route(tmp_path):
    """examples/workloads/separable_cnn.py at its small sizes with CLOUD_AMD_OPS=torch on the CPU:
    it prints its RESULT line and the loss falls."""
    env = dict(os.environ)
    env.update({"CLOUD_AMD_EXAMPLE_SMALL": "1", "CLOUD_AMD_OPS": "torch", "CLOUD_AMD_DEVICE": "cpu",
                "CLOUD_AMD_NUM_GPUS": "0",
                "CLOUD_AMD_JOBS_DIR": str(tmp_path / "jobs"), "PYTHONPATH": ROOT})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "workloads", "separable_cnn.py")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1]
    res = dict(kv.split("=") for kv in line.split()[2:])
    assert float(res["loss"]) < float(res["first_loss"]), line
    assert np.isfinite(float(res["eval_acc"]))
