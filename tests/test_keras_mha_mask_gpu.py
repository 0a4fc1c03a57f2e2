"""``attention_mask`` (and causal cross-attention) of ``keras.layers.MultiHeadAttention`` under
``mixed_bfloat16`` on the GPU: with key_dim = 64 the layer makes the projections of the unmasked
native routes and hands the mask to ``ops.attention(mask=)`` / ``ops.cross_attention(mask=)``, so
the attention itself runs on the masked cross-attention kernels.  As in test_keras_mha_cross_gpu
it is held to the same layer's float32 PyTorch path (relative norm 3e-2 for outputs, 8e-2 for
gradients, also those of the inputs), and a training step of it may not reach a library GEMM.
No mask here has a row without a visible key, so both layers compute the same function (on
such a row the native route gives zeros, the PyTorch branch the mean of the values).

Observed on an MI355X:

    route                            output    qkv_kernel  out_kernel  qkv_bias  out_bias  dquery    dvalue    dkey
    self [B,S,S]                     3.35e-3   4.55e-3     3.94e-3     2.51e-3   1.53e-3   4.62e-3   -         -
    causal self + padding [B,1,S]    3.30e-3   4.53e-3     3.86e-3     2.88e-3   1.53e-3   4.70e-3   -         -
    cross [B,T,S]                    3.50e-3   4.56e-3     4.10e-3     2.97e-3   2.06e-3   4.73e-3   4.56e-3   -
    cross [B,H,T,S] + key            3.60e-3   4.79e-3     4.02e-3     2.20e-3   1.39e-3   5.09e-3   4.35e-3   5.00e-3
    causal cross                     3.34e-3   4.55e-3     3.89e-3     3.35e-3   2.06e-3   5.03e-3   4.48e-3   -
    cross numpy [T,S]                3.47e-3   4.70e-3     3.97e-3     3.08e-3   2.06e-3   4.84e-3   4.70e-3   -
    bounds                           3e-2      8e-2        8e-2        8e-2      8e-2      8e-2      8e-2      8e-2
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_keras_mha_gpu import counted, rel  # noqa: E402  (the library-GEMM counter and the metric)

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, T, S, H, D = 2, 70, 100, 2, 64
DIM = H * D


def _pair(**kw):
    """The same weights as a mixed_bfloat16 and as a float32 layer."""
    from cloud_amd.keras import layers

    torch.manual_seed(3)
    mixed = layers.MultiHeadAttention(H, D, dtype="mixed_bfloat16", **kw)
    ref = layers.MultiHeadAttention(H, D, dtype="float32", **kw)
    for layer in (mixed, ref):
        layer._maybe_build([(None, T, DIM), (None, S, DIM)], torch.device(DEV))
    w = mixed.get_weights()
    w[1::2] = [torch.randn(*a.shape).mul_(0.1).numpy() for a in w[1::2]]  # non-zero biases
    mixed.set_weights(w)
    ref.set_weights(mixed.get_weights())  # the bf16-rounded kernels
    assert mixed.qkv_kernel.dtype == torch.bfloat16 and ref.qkv_kernel.dtype == torch.float32
    return mixed, ref


def _rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) < 0.5


NAMES = ("self [B,S,S]", "causal self + padding [B,1,S]", "cross [B,T,S]", "cross [B,H,T,S] + key", "causal cross",
         "cross numpy [T,S]")


def _cases():
    pad = torch.arange(S)[None, None, :] < torch.tensor([S, 63])[:, None, None]  # [B, 1, S], key 0 always visible
    return {
        "self [B,S,S]": dict(lens=(S,), kw=dict(attention_mask=_rand((B, S, S), 1).to(DEV))),
        "causal self + padding [B,1,S]": dict(lens=(S,), kw=dict(attention_mask=pad.to(DEV), use_causal_mask=True)),
        "cross [B,T,S]": dict(lens=(T, S), kw=dict(attention_mask=_rand((B, T, S), 2).to(DEV))),
        "cross [B,H,T,S] + key": dict(lens=(T, S, S), kw=dict(attention_mask=_rand((B, H, T, S), 3).to(DEV))),
        "causal cross": dict(lens=(T, S), kw=dict(use_causal_mask=True)),
        "cross numpy [T,S]": dict(lens=(T, S), kw=dict(attention_mask=_rand((T, S), 4).numpy())),
    }


def _expected_mask(name, kw):
    """The [B|1, H|1, T|1, S] mask the kernels must be handed."""
    m = kw.get("attention_mask")
    if m is not None:
        m = torch.as_tensor(m).to(DEV)
        while m.dim() < 3:
            m = m[None]
        if m.dim() == 3:
            m = m[:, None]
    if kw.get("use_causal_mask"):
        n = S if "self" in name else T
        tri = torch.ones(n, S, dtype=torch.bool, device=DEV).tril()
        m = tri[None, None] if m is None else m & tri
    return m


@pytest.mark.parametrize("name", NAMES)
def test_masked_mha_mixed_matches_float32_path(monkeypatch, name):
    from cloud_amd.ops import raw

    assert tuple(_cases()) == NAMES
    case = _cases()[name]
    lens, kw = case["lens"], case["kw"]
    mixed, ref = _pair()
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, n, DIM, generator=g).to(DEV) for n in lens]
    Tq = lens[0]
    dy = torch.randn(B, Tq, DIM, generator=g).to(DEV)
    native = {"attn_cross_fwd": [], "attn_cross_bwd": []}
    for fn in native:
        def f(*a, _orig=getattr(raw, fn), _fn=fn, **k):
            native[_fn].append(k.get("mask"))
            return _orig(*a, **k)

        monkeypatch.setattr(raw, fn, f)

    def call(layer, ins):
        args = (ins[0], ins[0]) if len(ins) == 1 else (ins[0], ins[1])  # self-attention: the same object twice
        return layer(*args, key=ins[2] if len(ins) == 3 else None, training=True, **kw)

    ins = [x.clone().requires_grad_() for x in xs]
    y = call(mixed, ins)
    assert len(native["attn_cross_fwd"]) == 1, "the mixed layer must take the masked cross-attention kernels"
    m = native["attn_cross_fwd"][0]
    want = _expected_mask(name, kw)
    assert m is not None and m.dtype == torch.bool and m.dim() == 4
    assert torch.equal(m.expand(B, H, Tq, S), want.expand(B, H, Tq, S))
    assert (m.expand(B, H, Tq, S).sum(-1) > 0).all(), "no dead rows: both layers compute the same function"
    assert y.dtype == torch.bfloat16 and y.shape == (B, Tq, DIM)
    (y.float() * dy).sum().backward()
    assert len(native["attn_cross_bwd"]) == 1 and native["attn_cross_bwd"][0].data_ptr() == m.data_ptr()
    ins_r = [x.to(torch.bfloat16).float().requires_grad_() for x in xs]  # what the mixed projections read
    y_r = call(ref, ins_r)
    (y_r * dy).sum().backward()
    torch.cuda.synchronize()
    assert len(native["attn_cross_fwd"]) == 1 and len(native["attn_cross_bwd"]) == 1, \
        "the float32 layer takes the PyTorch path"
    e = rel(y, y_r)
    print(f"[mha-mask] {name}: out {e:.3e}", flush=True)
    worst = {}
    for (n, p), (_, p_r) in zip(mixed.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        worst[n] = rel(p.grad, p_r.grad)
    for n, a, b in zip(("query", "value", "key"), ins, ins_r):
        assert a.grad is not None and a.grad.shape == b.grad.shape, n
        worst["d" + n] = rel(a.grad, b.grad)
    print(f"[mha-mask] {name}: grads { {k: f'{v:.2e}' for k, v in worst.items()} }", flush=True)
    assert e < 3e-2, e
    assert all(v < 8e-2 for v in worst.values()), worst


@pytest.mark.parametrize("name", ["causal self + padding [B,1,S]", "cross [B,T,S]", "causal cross"])
def test_masked_mha_training_step_uses_no_library_gemm(monkeypatch, name):
    from cloud_amd.keras import layers
    from cloud_amd.ops import raw

    case = _cases()[name]
    lens, kw = case["lens"], case["kw"]
    torch.manual_seed(0)
    layer = layers.MultiHeadAttention(H, D, dropout=0.1, dtype="mixed_bfloat16")
    xs = [torch.randn(B, n, DIM, device=DEV) for n in lens]
    layer._maybe_build([(None, lens[0], DIM), (None, S, DIM)], torch.device(DEV))
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
    layer.train()
    native = {}
    for fn in ("attn_cross_fwd", "attn_cross_bwd"):
        def f(*a, _orig=getattr(raw, fn), _fn=fn, **k):
            assert k.get("mask") is not None
            native[_fn] = native.get(_fn, 0) + 1
            return _orig(*a, **k)

        monkeypatch.setattr(raw, fn, f)
    args = (xs[0], xs[0]) if len(xs) == 1 else (xs[0], xs[1])
    with counted(monkeypatch) as calls:
        opt.zero_grad()
        loss = layer(*args, training=True, **kw).float().square().mean()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    assert not calls, calls
    assert native == {"attn_cross_fwd": 1, "attn_cross_bwd": 1}, native
    assert math.isfinite(float(loss.detach()))
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in layer.parameters())
    assert all(float(p.grad.float().abs().max()) > 0 for p in layer.parameters())


def test_returned_scores_keep_the_pytorch_branch(monkeypatch):
    from cloud_amd.ops import raw

    mixed, _ = _pair()
    called = []
    fwd = raw.attn_cross_fwd
    monkeypatch.setattr(raw, "attn_cross_fwd", lambda *a, **k: (called.append(1), fwd(*a, **k))[1])
    g = torch.Generator().manual_seed(5)
    x, v = torch.randn(B, T, DIM, generator=g).to(DEV), torch.randn(B, S, DIM, generator=g).to(DEV)
    mask = _rand((B, T, S), 6).to(DEV)
    out, scores = mixed(x, v, attention_mask=mask, return_attention_scores=True)
    assert not called
    assert scores.shape == (B, H, T, S) and out.shape == (B, T, DIM)
    assert (scores[~mask[:, None].expand(B, H, T, S)] == 0).all()
    torch.testing.assert_close(scores.sum(-1), torch.ones(B, H, T, device=DEV), rtol=1e-5, atol=1e-5)
    out_native = mixed(x, v, attention_mask=mask)
    assert called == [1]
    assert rel(out_native, out) < 3e-2
