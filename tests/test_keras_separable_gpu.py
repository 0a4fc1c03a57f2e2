"""Keras ``DepthwiseConv2D`` / ``SeparableConv2D`` under ``mixed_bfloat16`` on the GPU: layer
outputs and parameter gradients against float64 (from the layers' own bf16 weights and the bf16
input), a ``fit`` step of a separable model that reaches no library convolution / GEMM / pad,
and the example workload end to end.

Bounds are those of test_depthwise_conv_gpu.py: outputs per pixel row < 1e-2, bf16 kernel
gradients per tap < 2e-2, bias gradients in relative norm < 1e-2.  Figures observed on an
MI355X are in that module's table.
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
ROW_BOUND, WGBF_BOUND, BIAS_BOUND = 1e-2, 2e-2, 1e-2


def _say(*a):
    print("[separable]", *a, flush=True)


def _row_err(got, ref):
    C = ref.shape[-1]
    g, r = got.detach().double().cpu().reshape(-1, C), ref.detach().reshape(-1, C)
    assert torch.isfinite(g).all()
    n = r.norm(dim=-1)
    return ((g - r).norm(dim=-1) / torch.maximum(n, n.median())).max().item()


def _tap_err(got, ref):
    """kernel gradients [KH, KW, ...] (or [filters, 1, 1, cin]: one tap) per tap over the rest."""
    taps = ref.shape[0] * ref.shape[1] if ref.shape[1:3] != (1, 1) else 1
    g, r = got.detach().double().cpu().reshape(taps, -1), ref.detach().reshape(taps, -1)
    assert torch.isfinite(g).all()
    return ((g - r).norm(dim=-1) / r.norm(dim=-1)).max().item()


def _dw64(x, w, stride, pads):
    """float64 depthwise convolution, NHWC x, [KH, KW, C, DM] w, explicit ((t, b), (l, r)) pads."""
    KH, KW, C, DM = w.shape
    (pt, pb), (pl, pr) = pads
    xc = F.pad(x.permute(0, 3, 1, 2), (pl, pr, pt, pb))
    return F.conv2d(xc, w.permute(2, 3, 0, 1).reshape(C * DM, 1, KH, KW), None, stride, 0, 1, C).permute(0, 2, 3, 1)


@pytest.mark.parametrize("kind", ["depthwise", "separable"])
def test_layer_outputs_and_parameter_gradients_vs_fp64(kind):
    """2x9x6x16, 3x3, SAME, stride 2 (symmetric pads in H, the extra column on the right in W),
    bias and ReLU in the epilogue of the depthwise kernel / of the pointwise GEMM."""
    from cloud_amd.keras import layers

    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 9, 6, 16, generator=g).to(BF16)
    if kind == "depthwise":
        layer = layers.DepthwiseConv2D(3, strides=2, padding="same", activation="relu", dtype="mixed_bfloat16")
    else:
        layer = layers.SeparableConv2D(24, 3, strides=2, padding="same", activation="relu", dtype="mixed_bfloat16")
    xd = x.to("cuda").requires_grad_()
    y = layer(xd)
    with torch.no_grad():  # a bias off zero (the initializer's zeros would hide a misplaced add)
        layer.bias.copy_(0.3 * torch.randn(layer.bias.shape, generator=g))
    y = layer(xd)
    assert y.dtype == BF16 and layer.depthwise_kernel.dtype == BF16 and layer.bias.dtype == torch.float32
    assert tuple(y.shape) == (2, 5, 3, 16 if kind == "depthwise" else 24)
    dy = torch.randn(y.shape, generator=g).to(BF16)
    y.backward(dy.to("cuda"))
    torch.cuda.synchronize()

    x64 = x.double().requires_grad_()
    p64 = {n: p.detach().double().cpu().requires_grad_() for n, p in layer.named_parameters()}
    pads = ((1, 1), (0, 1))
    z = _dw64(x64, p64["depthwise_kernel"], 2, pads)
    if kind == "separable":
        z = z @ p64["pointwise_kernel"].reshape(24, 16).t()
    ref = torch.relu(z + p64["bias"])
    ref.backward(dy.double())
    e_y, e_dx = _row_err(y, ref), _row_err(xd.grad, x64.grad)
    e_dk = _tap_err(layer.depthwise_kernel.grad, p64["depthwise_kernel"].grad)
    e_b = ((layer.bias.grad.double().cpu() - p64["bias"].grad).norm() / p64["bias"].grad.norm()).item()
    msg = f"{kind}: y/row {e_y:.3e} dx/row {e_dx:.3e} depthwise_kernel/tap {e_dk:.3e} bias {e_b:.3e}"
    e_pk = 0.0
    if kind == "separable":
        e_pk = _tap_err(layer.pointwise_kernel.grad, p64["pointwise_kernel"].grad)
        msg += f" pointwise_kernel {e_pk:.3e}"
    _say(msg)
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND
    assert e_dk < WGBF_BOUND and e_pk < WGBF_BOUND and e_b < BIAS_BOUND


@contextlib.contextmanager
def counted(monkeypatch):
    from cloud_amd.ops import raw

    calls = {}

    def wrap(owner, name, tag):
        orig = getattr(owner, name)

        def f(*a, **k):
            calls[tag] = calls.get(tag, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(owner, name, f)

    for name in ("conv2d", "mm"):
        wrap(torch, name, "torch." + name)
    for name in ("conv2d", "pad", "linear"):
        wrap(F, name, "F." + name)
    wrap(raw, "_plain_lib", "raw._plain_lib")
    yield calls


def test_separable_model_fit_step_uses_no_library_path(monkeypatch):
    from cloud_amd import keras
    from cloud_amd.keras import engine
    from cloud_amd.ops import raw

    native = {}
    for name in ("dwconv_fwd", "dwconv_dgrad", "dwconv_wgrad"):
        def f(*a, _orig=getattr(raw, name), _name=name, **k):
            native[_name] = native.get(_name, 0) + 1
            return _orig(*a, **k)

        monkeypatch.setattr(raw, name, f)
    old = engine._POLICY
    engine.set_global_policy("mixed_bfloat16")
    try:
        rng = np.random.default_rng(0)
        x = rng.random((64, 15, 13, 3), dtype=np.float32)
        y = rng.integers(0, 10, (64,))
        L = keras.layers
        model = keras.Sequential([L.SeparableConv2D(16, 3, padding="same", activation="relu", input_shape=(15, 13, 3)),
                                  L.DepthwiseConv2D(3, strides=2, padding="same", activation="relu"),
                                  L.SeparableConv2D(32, 3, strides=2, padding="same", depth_multiplier=2,
                                                    activation="relu"),
                                  L.GlobalAveragePooling2D(), L.Dense(10, activation="softmax")])
        model.compile(optimizer="adam", loss="sparse_categorical_crossentropy", metrics=["accuracy"])
        model.fit(x[:32], y[:32], batch_size=32, epochs=1, verbose=0)  # build + first-step paths outside the count
        native.clear()
        with counted(monkeypatch) as calls:
            hist = model.fit(x[:32], y[:32], batch_size=32, epochs=1, verbose=0)
            torch.cuda.synchronize()
        assert not calls, calls
        # three depthwise forwards and weight gradients; the first layer's input needs no gradient
        assert native == {"dwconv_fwd": 3, "dwconv_dgrad": 2, "dwconv_wgrad": 3}, native
        assert np.isfinite(hist.history["loss"][0])
    finally:
        engine._POLICY = old


def test_separable_cnn_example_gpu(tmp_path):
    env = dict(os.environ)
    env.pop("CLOUD_AMD_DEVICE", None)
    env.update({"CLOUD_AMD_EXAMPLE_SMALL": "1", "CLOUD_AMD_JOBS_DIR": str(tmp_path / "jobs"), "PYTHONPATH": ROOT})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "workloads", "separable_cnn.py")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT fit")]
    assert lines, p.stdout[-2000:]
    res = dict(kv.split("=") for kv in lines[-1].split()[2:])
    _say(lines[-1])
    assert float(res["loss"]) < float(res["first_loss"]), lines[-1]
