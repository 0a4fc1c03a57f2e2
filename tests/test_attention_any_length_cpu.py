"""``ops.attention`` on the PyTorch reference path (CPU tensors): against an explicit
softmax(Q K^T * scale + mask) V, its gradient by ``gradcheck``, the key_len clamp and the
``training`` switch."""
import math

import torch

from cloud_amd.ops import attention


def _explicit(qkv, H, key_len, scale=None):
    """softmax(Q K^T * scale + additive -inf key mask) V, head by head."""
    B, S, C3 = qkv.shape
    D = C3 // (3 * H)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    out = torch.zeros(B, S, H * D, dtype=qkv.dtype)
    for b in range(B):
        kl = S if key_len is None else min(max(int(key_len[b]), 1), S)
        mask = torch.zeros(S, dtype=qkv.dtype)
        mask[kl:] = float("-inf")
        for h in range(H):
            q = qkv[b, :, h * D:(h + 1) * D]
            k = qkv[b, :, H * D + h * D:H * D + (h + 1) * D]
            v = qkv[b, :, 2 * H * D + h * D:2 * H * D + (h + 1) * D]
            out[b, :, h * D:(h + 1) * D] = torch.softmax(q @ k.t() * scale + mask[None, :], -1) @ v
    return out


def test_attention_cpu_matches_explicit_formula():
    torch.manual_seed(0)
    B, S, H, D = 2, 5, 2, 32
    qkv = torch.randn(B, S, 3 * H * D)
    key_len = torch.tensor([5, 3])
    out = attention(qkv, H, key_len)
    assert out.shape == (B, S, H * D) and out.dtype == torch.float32
    torch.testing.assert_close(out, _explicit(qkv, H, key_len), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(attention(qkv, H), _explicit(qkv, H, None), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(attention(qkv, H, key_len, scale=0.3), _explicit(qkv, H, key_len, 0.3), atol=1e-5,
                               rtol=1e-5)


def test_attention_cpu_gradcheck_fp64():
    torch.manual_seed(1)
    B, S, H, D = 2, 3, 2, 4
    qkv = torch.randn(B, S, 3 * H * D, dtype=torch.float64, requires_grad=True)
    key_len = torch.tensor([3, 2])
    assert torch.autograd.gradcheck(lambda t: attention(t, H, key_len), (qkv,))
    assert torch.autograd.gradcheck(lambda t: attention(t, H), (qkv,))


def test_attention_cpu_key_len_is_clamped():
    torch.manual_seed(2)
    B, S, H, D = 2, 5, 2, 32
    qkv = torch.randn(B, S, 3 * H * D)
    a = attention(qkv, H, torch.tensor([0, S + 5]))
    b = attention(qkv, H, torch.tensor([1, S]))
    assert torch.equal(a, b)


def test_attention_cpu_eval_ignores_dropout():
    torch.manual_seed(3)
    B, S, H, D = 2, 5, 2, 32
    qkv = torch.randn(B, S, 3 * H * D)
    key_len = torch.tensor([5, 3])
    a = attention(qkv, H, key_len, dropout_p=0.5, training=False)
    b = attention(qkv, H, key_len, dropout_p=0.0)
    assert torch.equal(a, b)
    c = attention(qkv, H, key_len, dropout_p=0.5, training=True)
    assert not torch.equal(c, b)
