"""Head dimensions of the attention kernels, the part that needs no GPU: the supported set lives
in ``raw.ATTN_HEAD_DIMS``, a head dimension outside it is refused before the extension is loaded,
and on the CPU ``ops.attention`` / ``ops.cross_attention`` at D = 32 and 128 are still the PyTorch
reference expression."""
import math

import pytest
import torch


def test_supported_head_dims():
    from cloud_amd.ops import raw

    assert raw.ATTN_HEAD_DIMS == (32, 64, 128)


def test_unsupported_head_dim_raises_before_the_extension_is_loaded(monkeypatch):
    from cloud_amd.ops import _ext, raw

    def no_load(*a, **k):
        raise AssertionError("the extension was asked for")

    monkeypatch.setattr(_ext, "load", no_load)
    B, T, S, H, D = 1, 3, 5, 2, 48
    qkv = torch.zeros(B * S, 3 * H * D, dtype=torch.bfloat16)
    q = torch.zeros(B * T, H * D, dtype=torch.bfloat16)
    kv = torch.zeros(B * S, 2 * H * D, dtype=torch.bfloat16)
    ctx, dctx = torch.zeros_like(q), torch.zeros_like(q)
    with pytest.raises(ValueError, match="head_dim"):
        raw.attn_fwd(qkv, B, S, H, head_dim=D)
    with pytest.raises(ValueError, match="head_dim"):
        raw.attn_bwd(qkv, qkv[:, :H * D], qkv[:, :H * D], torch.zeros(B, H, S), B, S, H, head_dim=D)
    with pytest.raises(ValueError, match="head_dim"):
        raw.attn_cross_fwd(q, kv, B, T, S, H, head_dim=D)
    with pytest.raises(ValueError, match="head_dim"):
        raw.attn_cross_bwd(q, kv, ctx, dctx, torch.zeros(B, H, T), B, T, S, H, head_dim=D)


@pytest.mark.parametrize("D,H", [(32, 3), (128, 2)])
@pytest.mark.parametrize("causal", [False, True])
def test_cpu_attention_is_the_reference_expression(D, H, causal):
    from cloud_amd.ops import attention
    from cloud_amd.ops.attention import _reference

    B, S = 2, 37
    g = torch.Generator().manual_seed(D)
    qkv = torch.randn(B, S, 3 * H * D, generator=g)
    kl = torch.tensor([S, 19])
    x = qkv.clone().requires_grad_()
    y = attention(x, H, kl, causal=causal)
    x_r = qkv.clone().requires_grad_()
    y_r = _reference(x_r, H, kl, 1.0 / math.sqrt(D), 0.0, causal)
    assert torch.equal(y, y_r)
    dy = torch.randn(B, S, H * D, generator=g)
    y.backward(dy)
    y_r.backward(dy)
    assert torch.equal(x.grad, x_r.grad)
    # against the definition, per head
    q, k, v = qkv.double().view(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(D)
    pos = torch.arange(S)
    sc = sc.masked_fill((pos[None, :] >= kl[:, None])[:, None, None, :], float("-inf"))
    if causal:
        sc = sc.masked_fill((pos[None, :] > pos[:, None])[None, None], float("-inf"))
    want = (sc.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, S, H * D)
    assert (y.double() - want).abs().max().item() < 1e-5


@pytest.mark.parametrize("D,H", [(32, 3), (128, 2)])
def test_cpu_cross_attention_is_the_reference_expression(D, H):
    from cloud_amd.ops import cross_attention
    from cloud_amd.ops.attention import _cross_reference

    B, T, S = 2, 11, 37
    g = torch.Generator().manual_seed(D)
    q = torch.randn(B, T, H * D, generator=g)
    kv = torch.randn(B, S, 2 * H * D, generator=g)
    kl = torch.tensor([S, 19])
    a, b = q.clone().requires_grad_(), kv.clone().requires_grad_()
    y = cross_attention(a, b, H, kl)
    a_r, b_r = q.clone().requires_grad_(), kv.clone().requires_grad_()
    y_r = _cross_reference(a_r, b_r, H, kl, 1.0 / math.sqrt(D), 0.0)
    assert torch.equal(y, y_r)
    dy = torch.randn(B, T, H * D, generator=g)
    y.backward(dy)
    y_r.backward(dy)
    assert torch.equal(a.grad, a_r.grad) and torch.equal(b.grad, b_r.grad)
    qh = q.double().view(B, T, H, D).transpose(1, 2)
    k, v = kv.double().view(B, S, 2, H, D).permute(2, 0, 3, 1, 4)
    sc = (qh @ k.transpose(-1, -2)) / math.sqrt(D)
    sc = sc.masked_fill((torch.arange(S)[None, :] >= kl[:, None])[:, None, None, :], float("-inf"))
    want = (sc.softmax(-1) @ v).transpose(1, 2).reshape(B, T, H * D)
    assert (y.double() - want).abs().max().item() < 1e-5
