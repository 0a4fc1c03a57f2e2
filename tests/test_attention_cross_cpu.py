"""``ops.cross_attention`` off the GPU: the PyTorch path (fp32, fp64 for fp64 inputs) against an
explicit einsum formula, its gradients, its argument checks, and the Keras layer's cross call
against the layer's own masked route."""
import math

import pytest
import torch

B, T, S, H, D = 2, 3, 5, 2, 4


@pytest.fixture(autouse=True)
def _float32_policy():
    from cloud_amd.keras import engine

    old = engine._POLICY
    engine.set_global_policy("float32")
    yield
    engine._POLICY = old


def _inputs(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, T, H * D, generator=g, dtype=torch.float64).to(dtype)
    kv = torch.randn(B, S, 2 * H * D, generator=g, dtype=torch.float64).to(dtype)
    return q, kv


def _einsum_ref(q, kv, key_len, scale):
    """float64, one einsum per product; keys >= key_len (clamped to [1, S]) get weight zero."""
    q4 = q.double().view(B, T, H, D)
    k4, v4 = kv.double().view(B, S, 2, H, D).unbind(2)
    sc = torch.einsum("bthd,bshd->bhts", q4, k4) * scale
    if key_len is not None:
        kl = torch.as_tensor(key_len).clamp(1, S)
        sc = sc.masked_fill((torch.arange(S)[None, :] >= kl[:, None])[:, None, None, :], float("-inf"))
    w = torch.exp(sc - sc.amax(-1, keepdim=True))
    w = w / w.sum(-1, keepdim=True)
    return torch.einsum("bhts,bshd->bthd", w, v4).reshape(B, T, H * D)


@pytest.mark.parametrize("dtype,tol", [(torch.float32, 1e-5), (torch.float64, 1e-12)])
@pytest.mark.parametrize("key_len", [None, [5, 2], [0, 9]])
@pytest.mark.parametrize("scale", [None, 0.3])
def test_cross_attention_matches_einsum(dtype, tol, key_len, scale):
    from cloud_amd.ops import cross_attention

    q, kv = _inputs(dtype)
    kl = None if key_len is None else torch.tensor(key_len)
    out = cross_attention(q, kv, H, kl, scale=scale)
    assert out.dtype == dtype and out.shape == (B, T, H * D)
    ref = _einsum_ref(q, kv, key_len, 1.0 / math.sqrt(D) if scale is None else scale)
    e = ((out.double() - ref).norm() / ref.norm()).item()
    assert e < tol, e
    # dropout off: eval mode, whatever dropout_p says
    assert torch.equal(cross_attention(q, kv, H, kl, dropout_p=0.5, training=False, scale=scale), out)


def test_cross_attention_masked_keys_take_no_part():
    from cloud_amd.ops import cross_attention

    q, kv = _inputs(torch.float64)
    kl = torch.tensor([5, 2])
    kv2 = kv.clone()
    kv2[1, 2:] = 123.0
    assert torch.equal(cross_attention(q, kv, H, kl), cross_attention(q, kv2, H, kl))


def test_cross_attention_gradcheck():
    from cloud_amd.ops import cross_attention

    q, kv = _inputs(torch.float64, seed=1)
    q.requires_grad_()
    kv.requires_grad_()
    kl = torch.tensor([5, 3])
    assert torch.autograd.gradcheck(lambda a, b: cross_attention(a, b, H, kl), (q, kv))
    assert torch.autograd.gradcheck(lambda a, b: cross_attention(a, b, H, None, scale=0.7), (q, kv))


def test_cross_attention_dropout_runs_only_in_training():
    from cloud_amd.ops import cross_attention

    q, kv = _inputs(torch.float32)
    torch.manual_seed(0)
    a = cross_attention(q, kv, H, dropout_p=0.5, training=True)
    assert not torch.equal(a, cross_attention(q, kv, H))


@pytest.mark.parametrize("qs,kvs", [
    ((B, T, H * D + 1), (B, S, 2 * H * D)),       # q: last dim is no multiple of H
    ((B, T, H * D), (B, S, 2 * H * D + 2)),       # kv: last dim is no multiple of 2 H
    ((B, T, H * D), (B + 1, S, 2 * H * D)),       # batch
    ((B, T, H * D), (B, S, 2 * H * (D + 1))),     # head dim
    ((B * T, H * D), (B, S, 2 * H * D)),          # rank
])
def test_cross_attention_rejects_mismatched_operands(qs, kvs):
    from cloud_amd.ops import cross_attention

    with pytest.raises(ValueError):
        cross_attention(torch.zeros(*qs), torch.zeros(*kvs), H)


@pytest.mark.parametrize("with_key", [False, True])
def test_keras_cross_call_equals_the_masked_route(with_key):
    """float32 on the CPU: the cross call goes through ``ops.cross_attention``, the call with an
    all-true ``attention_mask`` keeps the layer's PyTorch route -- the same math in another order."""
    from cloud_amd.keras import layers

    dim, Tq, Sk = 12, 7, 5
    torch.manual_seed(0)
    layer = layers.MultiHeadAttention(3, 4)
    layer._maybe_build([(None, Tq, dim), (None, Sk, dim)])
    with torch.no_grad():
        layer.qkv_bias.normal_(0, 0.3)
        layer.out_bias.normal_(0, 0.3)
    layer.eval()
    g = torch.Generator().manual_seed(5)
    x, v, k = (torch.randn(B, n, dim, generator=g) for n in (Tq, Sk, Sk))
    args = (x, v, k) if with_key else (x, v)
    out = layer(*args)
    ref = layer(*args, attention_mask=torch.ones(B, Tq, Sk, dtype=torch.bool))
    assert out.shape == (B, Tq, dim)
    torch.testing.assert_close(out, ref, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(layer([x, v]), layer(x, v, attention_mask=torch.ones(B, Tq, Sk, dtype=torch.bool)),
                               rtol=1e-5, atol=1e-6)


def test_keras_cross_call_reaches_the_op(monkeypatch):
    from cloud_amd import ops
    from cloud_amd.keras import layers

    seen = []
    orig = ops.cross_attention
    monkeypatch.setattr(ops, "cross_attention", lambda *a, **k: (seen.append(a[1].shape), orig(*a, **k))[1])
    layer = layers.MultiHeadAttention(3, 4)
    x, v = torch.randn(B, 7, 12), torch.randn(B, 5, 12)
    layer(x, v)
    assert seen == [(B, 5, 24)]
    layer(x, v, attention_mask=torch.ones(B, 7, 5, dtype=torch.bool))  # masked: the PyTorch route
    layer(x, v, use_causal_mask=True)                                  # causal cross: the PyTorch route
    layer(x, v, return_attention_scores=True)
    layer(x, x)                                                         # self-attention: ops.attention
    assert len(seen) == 1
