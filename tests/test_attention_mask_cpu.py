"""``mask=`` of ``ops.attention`` and ``ops.cross_attention`` on the PyTorch path (CPU, fp64),
against a dense implementation written here with explicit loops over (batch, head, query): the
softmax runs over the list of visible keys of each row, and a row with no visible key is zeros.

Conventions under test: True = the query may see the key; the mask composes with ``key_len`` and
``causal``; accepted ranks ``[S]``, ``[T, S]``, ``[B|1, T|1, S]``, ``[B|1, H|1, T|1, S]``; a dead
row (no visible key) has a zero context row and sends zero gradients, and nothing is NaN.
"""
import math

import pytest
import torch

from cloud_amd import ops

B, T, S, H, D = 2, 5, 7, 2, 4
C = H * D


def _inputs(seed=0, t=T, s=S):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, t, C, generator=g, dtype=torch.float64)
    kv = torch.randn(B, s, 2 * C, generator=g, dtype=torch.float64)
    return q, kv


def _mask(seed=0, t=T, s=S, density=0.6):
    g = torch.Generator().manual_seed(100 + seed)
    return torch.rand(B, H, t, s, generator=g) < density


def _dense(q, kv, allowed, scale=None):
    """Row by row over the visible keys only; ``allowed`` is a full [B, H, T, S] bool tensor."""
    Bq, Tq, _ = q.shape
    Sk = kv.shape[1]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    rows = []
    for b in range(Bq):
        for t in range(Tq):
            heads = []
            for h in range(H):
                keys = allowed[b, h, t].nonzero().flatten()
                if keys.numel() == 0:
                    heads.append(q.new_zeros(D))
                    continue
                k = kv[b, keys, h * D:(h + 1) * D]
                v = kv[b, keys, C + h * D:C + (h + 1) * D]
                w = torch.softmax((k @ q[b, t, h * D:(h + 1) * D]) * scale, 0)
                heads.append(w @ v)
            rows.append(torch.cat(heads))
    return torch.stack(rows).view(Bq, Tq, C)


def _full(mask, t=T, s=S):
    m = torch.as_tensor(mask)
    if m.dim() == 3:
        m = m[:, None]
    while m.dim() < 4:
        m = m[None]
    return m.expand(B, H, t, s)


def _with_key_len(allowed, key_len):
    s = allowed.shape[-1]
    return allowed & (torch.arange(s)[None, :] < key_len.clamp(1, s)[:, None])[:, None, None, :]


def test_cross_attention_mask_matches_dense_forward_and_backward():
    q, kv = _inputs()
    m = _mask()
    m[0, 1, 2] = False                      # a dead row
    key_len = torch.tensor([S, 4])
    m[1, 0, 3, :4] = False                  # dead only through key_len and the mask together
    assert m[1, 0, 3, 4:].any()
    g = torch.randn(B, T, C, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    for kl in (None, key_len):
        allowed = m if kl is None else _with_key_len(m, kl)
        a, b = q.clone().requires_grad_(), kv.clone().requires_grad_()
        out = ops.cross_attention(a, b, H, kl, mask=m)
        out.backward(g)
        a2, b2 = q.clone().requires_grad_(), kv.clone().requires_grad_()
        ref = _dense(a2, b2, allowed)
        ref.backward(g)
        assert out.dtype == torch.float64 and out.shape == (B, T, C)
        torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(a.grad, a2.grad, rtol=1e-11, atol=1e-12)
        torch.testing.assert_close(b.grad, b2.grad, rtol=1e-11, atol=1e-12)
        # dead rows: exactly zero context and dQ, everything finite
        dead = ~allowed.any(-1)             # [B, H, T]
        assert dead[0, 1, 2] and (kl is None or dead[1, 0, 3])
        o4, dq4 = out.detach().view(B, T, H, D).transpose(1, 2), a.grad.view(B, T, H, D).transpose(1, 2)
        assert (o4[dead] == 0).all() and (dq4[dead] == 0).all()
        assert (o4[~dead].abs().sum(-1) > 0).all()
        for t in (out, a.grad, b.grad):
            assert torch.isfinite(t).all()


def test_attention_mask_matches_dense_forward_and_backward():
    g0 = torch.Generator().manual_seed(3)
    qkv = torch.randn(B, S, 3 * C, generator=g0, dtype=torch.float64)
    m = _mask(2, S, S)
    m[1, 0, 4] = False                      # a dead row
    key_len = torch.tensor([5, S])
    g = torch.randn(B, S, C, dtype=torch.float64, generator=g0)
    for kl, causal in ((None, False), (key_len, False), (key_len, True)):
        allowed = m if kl is None else _with_key_len(m, kl)
        if causal:
            allowed = allowed & torch.ones(S, S, dtype=torch.bool).tril()
        x = qkv.clone().requires_grad_()
        out = ops.attention(x, H, kl, causal=causal, mask=m)
        out.backward(g)
        x2 = qkv.clone().requires_grad_()
        ref = _dense(x2[..., :C], x2[..., C:], allowed)
        ref.backward(g)
        torch.testing.assert_close(out, ref, rtol=1e-12, atol=1e-13)
        torch.testing.assert_close(x.grad, x2.grad, rtol=1e-11, atol=1e-12)
        dead = ~allowed.any(-1)
        assert dead[1, 0, 4]
        assert (out.detach().view(B, S, H, D).transpose(1, 2)[dead] == 0).all()
        assert (x.grad[..., :C].view(B, S, H, D).transpose(1, 2)[dead] == 0).all()
        assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()


def test_gradcheck_with_dead_rows():
    q, kv = _inputs(1)
    m = _mask(1)
    m[0, 0, 1] = False                      # dead through the mask
    key_len = torch.tensor([S, 3])
    m[1, 1, 2, :3] = False                  # dead only through key_len and the mask together
    assert m[1, 1, 2, 3:].any()
    q.requires_grad_()
    kv.requires_grad_()
    assert torch.autograd.gradcheck(lambda a, b: ops.cross_attention(a, b, H, key_len, mask=m), (q, kv))
    assert torch.autograd.gradcheck(lambda a, b: ops.cross_attention(a, b, H, None, mask=m[:, :1]), (q, kv))
    qkv = torch.randn(B, S, 3 * C, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    qkv.requires_grad_()
    ms = _mask(3, S, S)
    ms[0, 1, 0] = False
    ms[1, 0, 6, :3] = False
    assert torch.autograd.gradcheck(lambda x: ops.attention(x, H, key_len, mask=ms), (qkv,))
    assert torch.autograd.gradcheck(lambda x: ops.attention(x, H, key_len, causal=True, mask=ms), (qkv,))


def test_prefix_mask_equals_key_len():
    q, kv = _inputs(2)
    key_len = torch.tensor([S, 3])
    prefix = torch.arange(S)[None, :] < key_len[:, None]        # [B, S]
    ref = ops.cross_attention(q, kv, H, key_len)
    out = ops.cross_attention(q, kv, H, None, mask=prefix[:, None, :])
    torch.testing.assert_close(out, ref, rtol=1e-13, atol=1e-14)
    qkv = torch.randn(B, S, 3 * C, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    torch.testing.assert_close(ops.attention(qkv, H, None, mask=prefix[:, None, :]), ops.attention(qkv, H, key_len),
                               rtol=1e-13, atol=1e-14)


def test_tril_mask_equals_causal():
    qkv = torch.randn(B, S, 3 * C, dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    tril = torch.ones(S, S, dtype=torch.bool).tril()
    key_len = torch.tensor([4, S])
    for kl in (None, key_len):
        x, y = qkv.clone().requires_grad_(), qkv.clone().requires_grad_()
        a = ops.attention(x, H, kl, mask=tril)
        b = ops.attention(y, H, kl, causal=True)
        torch.testing.assert_close(a, b, rtol=1e-13, atol=1e-14)
        a.sum().backward()
        b.sum().backward()
        torch.testing.assert_close(x.grad, y.grad, rtol=1e-12, atol=1e-13)
    # the same mask on the cross op, on the column views
    c = ops.cross_attention(qkv[..., :C], qkv[..., C:], H, None, mask=tril)
    torch.testing.assert_close(c, ops.attention(qkv, H, None, causal=True), rtol=1e-13, atol=1e-14)


def test_every_mask_rank_equals_its_4d_form():
    q, kv = _inputs(3)
    g = torch.Generator().manual_seed(9)
    rnd = lambda *shape: torch.rand(*shape, generator=g) < 0.6  # noqa: E731
    masks = [rnd(S), rnd(T, S), rnd(B, T, S), rnd(1, T, S), rnd(B, 1, S), rnd(1, 1, S), rnd(B, H, T, S),
             rnd(1, H, T, S), rnd(B, 1, T, S), rnd(B, H, 1, S), rnd(1, 1, 1, S)]
    masks.append(rnd(B, S, T).transpose(1, 2))                  # key stride != 1
    masks.append(rnd(B, T, S).to(torch.uint8))                  # bytes: non-zero = visible
    masks.append(rnd(T, S).numpy())
    for m in masks:
        full = _full(m).bool().contiguous()
        out = ops.cross_attention(q, kv, H, None, mask=m)
        assert torch.equal(out, ops.cross_attention(q, kv, H, None, mask=full)), tuple(torch.as_tensor(m).shape)
        torch.testing.assert_close(out, _dense(q, kv, full), rtol=1e-12, atol=1e-13)
    qkv = torch.randn(B, S, 3 * C, dtype=torch.float64, generator=g)
    for m in (rnd(S), rnd(S, S), rnd(B, 1, S), rnd(B, S, S), rnd(1, H, S, S)):
        full = _full(m, S, S).contiguous()
        assert torch.equal(ops.attention(qkv, H, None, mask=m), ops.attention(qkv, H, None, mask=full))


def test_wrong_mask_raises_value_error():
    q, kv = _inputs(4)
    qkv = torch.zeros(B, S, 3 * C, dtype=torch.float64)
    ok = torch.ones
    bad = [ok(S + 1, dtype=torch.bool), ok(T + 1, S, dtype=torch.bool), ok(B + 1, T, S, dtype=torch.bool),
           ok(B, H + 1, T, S, dtype=torch.bool), ok(B, T, 1, dtype=torch.bool), ok(1, B, H, T, S, dtype=torch.bool),
           ok(B, T, S), ok(B, T, S, dtype=torch.int64), torch.tensor(True)]
    for m in bad:
        with pytest.raises(ValueError):
            ops.cross_attention(q, kv, H, None, mask=m)
    for m in (ok(S + 1, dtype=torch.bool), ok(T, S, dtype=torch.bool), ok(B, S, S, dtype=torch.float32)):
        with pytest.raises(ValueError):
            ops.attention(qkv, H, None, mask=m)


def test_mask_none_is_the_unmasked_expression():
    """``mask=None`` (and leaving the argument out) runs what ran before the argument existed:
    the expressions of the parent, written out here."""
    q, kv = _inputs(5)
    key_len = torch.tensor([S, 3])
    scale = 1.0 / math.sqrt(D)
    qh = q.reshape(B, T, H, D).transpose(1, 2)
    k, v = kv.reshape(B, S, 2, H, D).permute(2, 0, 3, 1, 4)
    att = (qh @ k.transpose(-1, -2)) * scale
    pad = torch.arange(S)[None, :] >= key_len[:, None]
    att = att.masked_fill(pad[:, None, None, :], float("-inf")).softmax(-1)
    ref = (att @ v).transpose(1, 2).reshape(B, T, C)
    assert torch.equal(ops.cross_attention(q, kv, H, key_len, mask=None), ref)
    assert torch.equal(ops.cross_attention(q, kv, H, key_len), ref)

    qkv = torch.randn(B, S, 3 * C, dtype=torch.float64, generator=torch.Generator().manual_seed(8))
    q3, k3, v3 = qkv.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    att = (q3 @ k3.transpose(-1, -2)) * scale
    att = att.masked_fill(pad[:, None, None, :], float("-inf"))
    att = att.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf")).softmax(-1)
    ref = (att @ v3).permute(0, 2, 1, 3).reshape(B, S, C)
    assert torch.equal(ops.attention(qkv, H, key_len, causal=True, mask=None), ref)
    assert torch.equal(ops.attention(qkv, H, key_len, causal=True), ref)
