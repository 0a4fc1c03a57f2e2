"""Cross-attention of ``keras.layers.MultiHeadAttention`` under ``mixed_bfloat16`` on the GPU: with
key_dim = 64, ``layer(decoder_states, encoder_states)`` is the Q projection, one K | V projection
(two and a concatenation for a ``key`` tensor of its own), ``ops.cross_attention`` and the
output projection, all on in-tree kernels.  As in test_keras_mha_gpu it is held to the same
layer's float32 PyTorch path (relative norm 3e-2 for outputs, 8e-2 for gradients, here also
those of both inputs), and a training step of it may not reach a library GEMM.

Observed on an MI355X:

    route               output    qkv_kernel  out_kernel  qkv_bias  out_bias  dquery    dvalue    dkey
    key absent          3.36e-3   4.66e-3     3.99e-3     2.98e-3   2.06e-3   4.85e-3   4.72e-3   -
    distinct key        3.47e-3   4.77e-3     3.87e-3     2.16e-3   1.39e-3   5.11e-3   4.28e-3   4.94e-3
    bounds              3e-2      8e-2        8e-2        8e-2      8e-2      8e-2      8e-2      8e-2
"""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_keras_mha_gpu import counted, rel  # noqa: E402  (the library-GEMM counter and the metric)

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T, S, H, D = 2, 70, 100, 2, 64
DIM = H * D


def _pair():
    """The same weights as a mixed_bfloat16 and as a float32 layer."""
    from cloud_amd.keras import layers

    torch.manual_seed(3)
    mixed = layers.MultiHeadAttention(H, D, dtype="mixed_bfloat16")
    ref = layers.MultiHeadAttention(H, D, dtype="float32")
    for layer in (mixed, ref):
        layer._maybe_build([(None, T, DIM), (None, S, DIM)], torch.device(DEV))
    w = mixed.get_weights()
    w[1::2] = [torch.randn(*a.shape).mul_(0.1).numpy() for a in w[1::2]]  # non-zero biases
    mixed.set_weights(w)
    ref.set_weights(mixed.get_weights())  # the bf16-rounded kernels
    assert mixed.qkv_kernel.dtype == torch.bfloat16 and ref.qkv_kernel.dtype == torch.float32
    return mixed, ref


@pytest.mark.parametrize("with_key", [False, True])
def test_cross_mha_mixed_matches_float32_path(monkeypatch, with_key):
    from cloud_amd.ops import raw

    mixed, ref = _pair()
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, n, DIM, generator=g).to(DEV) for n in ((T, S, S) if with_key else (T, S))]
    dy = torch.randn(B, T, DIM, generator=g).to(DEV)
    native = []
    fwd = raw.attn_cross_fwd
    monkeypatch.setattr(raw, "attn_cross_fwd", lambda *a, **k: (native.append(a[2:5]), fwd(*a, **k))[1])
    ins = [x.clone().requires_grad_() for x in xs]
    y = mixed(*ins, training=True)
    assert native == [(B, T, S)], "the mixed layer must take the cross-attention kernels"
    assert y.dtype == torch.bfloat16 and y.shape == (B, T, DIM)
    (y.float() * dy).sum().backward()
    ins_r = [x.to(torch.bfloat16).float().requires_grad_() for x in xs]  # what the mixed projections read
    y_r = ref(*ins_r, training=True)
    (y_r * dy).sum().backward()
    torch.cuda.synchronize()
    assert native == [(B, T, S)], "the float32 layer takes the PyTorch path"
    e = rel(y, y_r)
    print(f"[mha-cross] key={with_key}: out {e:.3e}", flush=True)
    worst = {}
    for (n, p), (_, p_r) in zip(mixed.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        worst[n] = rel(p.grad, p_r.grad)
    for n, a, b in zip(("query", "value", "key"), ins, ins_r):
        assert a.grad is not None and a.grad.shape == b.grad.shape, n
        worst["d" + n] = rel(a.grad, b.grad)
    print(f"[mha-cross] key={with_key}: grads {worst}", flush=True)
    assert e < 3e-2, e
    assert all(v < 8e-2 for v in worst.values()), worst


def test_cross_mha_training_step_uses_no_library_gemm(monkeypatch):
    from cloud_amd.keras import layers
    from cloud_amd.ops import raw

    torch.manual_seed(0)
    layer = layers.MultiHeadAttention(H, D, dropout=0.1, dtype="mixed_bfloat16")
    x_dec = torch.randn(B, T, DIM, device=DEV)
    x_enc = torch.randn(B, S, DIM, device=DEV)
    layer._maybe_build([(None, T, DIM), (None, S, DIM)], torch.device(DEV))
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
    layer.train()
    native = {}
    for name in ("attn_cross_fwd", "attn_cross_bwd"):
        def f(*a, _orig=getattr(raw, name), _name=name, **k):
            native[_name] = native.get(_name, 0) + 1
            return _orig(*a, **k)

        monkeypatch.setattr(raw, name, f)
    with counted(monkeypatch) as calls:
        opt.zero_grad()
        loss = layer([x_dec, x_enc], training=True).float().square().mean()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    assert not calls, calls
    assert native == {"attn_cross_fwd": 1, "attn_cross_bwd": 1}, native
    assert math.isfinite(float(loss.detach()))
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in layer.parameters())
    assert all(float(p.grad.float().abs().max()) > 0 for p in layer.parameters())


def test_functional_encoder_decoder_block_fits(monkeypatch):
    """Input(T, dim), Input(S, dim) -> causal self-MHA -> cross-MHA [dec, enc] -> Dense: the list
    form reaches ``call`` with two distinct tensors and takes the native route."""
    from cloud_amd import keras
    from cloud_amd.keras import engine, layers
    from cloud_amd.ops import raw

    native = []
    fwd = raw.attn_cross_fwd
    monkeypatch.setattr(raw, "attn_cross_fwd", lambda *a, **k: (native.append(a[2:5]), fwd(*a, **k))[1])

    old = engine._POLICY
    engine.set_global_policy("mixed_bfloat16")
    try:
        torch.manual_seed(0)
        Tm, Sm = 24, 40
        dec_in, enc_in = keras.Input(shape=(Tm, DIM)), keras.Input(shape=(Sm, DIM))
        a = layers.MultiHeadAttention(H, D, use_causal_mask=True, name="self_mha")([dec_in, dec_in])
        c = layers.MultiHeadAttention(H, D, name="cross_mha")([a, enc_in])
        out = layers.Dense(8)(c)
        model = keras.Model([dec_in, enc_in], out)
        cross = model.get_layer("cross_mha")
        cfg = cross.get_config()
        assert cfg["use_causal_mask"] is False and cfg["num_heads"] == H and cfg["key_dim"] == D
        assert layers.MultiHeadAttention.from_config(cfg).get_config() == cfg

        r = np.random.RandomState(0)
        xd = r.randn(8, Tm, DIM).astype(np.float32)
        xe = r.randn(8, Sm, DIM).astype(np.float32)
        y = r.randn(8, Tm, 8).astype(np.float32)
        model.compile(optimizer="adam", loss="mse")
        before = [p.detach().float().cpu() for p in cross.parameters()]  # fit moves the model to the GPU
        hist = model.fit([xd, xe], y, batch_size=8, epochs=1, verbose=0)
        assert math.isfinite(hist.history["loss"][0])
        assert native and all(n == (8, Tm, Sm) for n in native), native
        assert any(not torch.equal(a_, b_.detach().float().cpu()) for a_, b_ in zip(before, cross.parameters()))
    finally:
        engine._POLICY = old
