"""``keras.layers.MultiHeadAttention`` under ``mixed_bfloat16`` with key_dim 32 (3 heads) and 128
(2 heads): self-attention, causal self-attention, cross-attention and a masked call run on the
in-tree GEMM and attention kernels, as key_dim 64 does.  Outputs and parameter gradients are held to
the same layer's float32 PyTorch path with the bounds of test_keras_mha_gpu (relative norm 3e-2 for
outputs, 8e-2 for parameter gradients); a training step runs with the PyTorch reference
expressions of ``ops.attention`` replaced by functions that raise, and reaches no library GEMM.

Observed on an MI355X over the eight (key_dim, mode) cases: outputs 3.2e-3 .. 3.5e-3, parameter
gradients at most 4.8e-3 (``qkv_kernel``); each test prints its own."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_keras_mha_gpu import counted, rel  # noqa: E402  (the library-GEMM counter and the metric)

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T, S = 2, 70, 100
CONFIGS = [(3, 32), (2, 128)]  # num_heads, key_dim
MODES = ["self", "causal", "cross", "masked"]


def _pair(H, D, causal):
    """The same weights as a mixed_bfloat16 and as a float32 layer (test_keras_mha_gpu._pair)."""
    from cloud_amd.keras import layers

    dim = H * D
    torch.manual_seed(3)
    mixed = layers.MultiHeadAttention(H, D, use_causal_mask=causal, dtype="mixed_bfloat16")
    ref = layers.MultiHeadAttention(H, D, use_causal_mask=causal, dtype="float32")
    for layer in (mixed, ref):
        layer._maybe_build([(None, T, dim), (None, S, dim)], torch.device(DEV))
    w = mixed.get_weights()
    w[1::2] = [torch.randn(*a.shape).mul_(0.1).numpy() for a in w[1::2]]  # non-zero biases
    mixed.set_weights(w)
    ref.set_weights(mixed.get_weights())  # the bf16-rounded kernels
    assert mixed.qkv_kernel.dtype == torch.bfloat16 and ref.qkv_kernel.dtype == torch.float32
    return mixed, ref


def _inputs(H, D, mode):
    """-> query, value (the query itself for self-attention), attention_mask or None"""
    dim = H * D
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, T, dim, generator=g).to(DEV)
    mem = torch.randn(B, S, dim, generator=g).to(DEV)
    if mode in ("self", "causal"):
        return x, x, None
    if mode == "cross":
        return x, mem, None
    mask = torch.rand(B, T, S, generator=g) < 0.5  # every row keeps ~50 of its 100 keys
    assert (mask.sum(-1) >= 8).all()
    return x, mem, mask.to(DEV)


def _call(layer, q, v, mask):
    if v is q:
        return layer(q, q, attention_mask=mask, training=True)
    return layer(q, v, attention_mask=mask, training=True)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,D", CONFIGS)
def test_mha_mixed_matches_float32_path(H, D, mode):
    mixed, ref = _pair(H, D, mode == "causal")
    q, v, mask = _inputs(H, D, mode)
    g = torch.Generator().manual_seed(12)
    dy = torch.randn(B, T, H * D, generator=g).to(DEV)
    y = _call(mixed, q, v, mask)
    assert y.dtype == torch.bfloat16 and y.shape == (B, T, H * D)
    (y.float() * dy).sum().backward()
    qr = q.to(torch.bfloat16).float()  # what the mixed layer's projections read
    vr = qr if v is q else v.to(torch.bfloat16).float()
    y_r = _call(ref, qr, vr, mask)
    (y_r * dy).sum().backward()
    torch.cuda.synchronize()
    e = rel(y, y_r)
    worst = {}
    for (n, p), (_, p_r) in zip(mixed.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        worst[n] = rel(p.grad, p_r.grad)
    print(f"[mha-head-dim] H={H} D={D} {mode}: out {e:.3e} grads {worst}", flush=True)
    assert e < 3e-2, e
    assert all(x < 8e-2 for x in worst.values()), worst
    if mode == "causal":  # the flag reached the kernels: the non-causal layer computes something else
        other, _ = _pair(H, D, False)
        assert rel(other(q, q, training=True), y_r) > 0.1


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("H,D", CONFIGS)
def test_mha_training_step_is_native(monkeypatch, H, D, mode):
    """One SGD step with attention dropout: the PyTorch reference expressions are never entered
    and no library GEMM is called."""
    import importlib

    from cloud_amd.keras import layers

    attn_mod = importlib.import_module("cloud_amd.ops.attention")  # (ops.attention itself is the function)
    def refuse(*a, **k):
        raise AssertionError("the PyTorch reference route was taken")

    monkeypatch.setattr(attn_mod, "_reference", refuse)
    monkeypatch.setattr(attn_mod, "_cross_reference", refuse)
    torch.manual_seed(0)
    layer = layers.MultiHeadAttention(H, D, dropout=0.1, use_causal_mask=mode == "causal", dtype="mixed_bfloat16")
    layer._maybe_build([(None, T, H * D), (None, S, H * D)], torch.device(DEV))
    q, v, mask = _inputs(H, D, mode)
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
    layer.train()
    with counted(monkeypatch) as calls:
        opt.zero_grad()
        loss = _call(layer, q, v, mask).float().square().mean()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    assert not calls, calls
    assert math.isfinite(float(loss.detach()))
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in layer.parameters())
