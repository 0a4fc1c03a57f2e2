"""``ops.attention(..., causal=True)`` on the PyTorch reference path (CPU tensors, float32 /
float64, head dims 32 and 64) against ``F.scaled_dot_product_attention(is_causal=True)`` and,
with ``key_len``, against an explicit ``-inf`` mask.  float64 agrees to 1e-12 relative (the
explicit mask gave 2e-16), float32 to 1e-5."""
import math

import pytest
import torch
import torch.nn.functional as F

from cloud_amd.ops import attention

B, S, H = 3, 70, 2
KEY_LENS = [None, [70, 1, 33]]
TOL = {torch.float64: 1e-12, torch.float32: 1e-5}


def _inputs(D, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, S, 3 * H * D, generator=g, dtype=torch.float64).to(dtype)
    dout = torch.randn(B, S, H * D, generator=g, dtype=torch.float64).to(dtype)
    return qkv, dout


def _split(qkv, D):
    return qkv.reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)  # 3 x [B, H, S, D]


def _explicit(qkv, D, key_len):
    """softmax(Q K^T / sqrt(D) + mask) V with the mask written out as -inf."""
    q, k, v = _split(qkv, D)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(D)
    pos = torch.arange(S)
    hide = (pos[None, :] > pos[:, None])[None, None].expand(B, 1, S, S).clone()
    if key_len is not None:
        kl = torch.tensor(key_len).clamp(1, S)
        hide |= (pos[None, :] >= kl[:, None])[:, None, None, :]
    sc = sc.masked_fill(hide, float("-inf"))
    return (sc.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, S, H * D)


def _sdpa(qkv, D):
    q, k, v = _split(qkv, D)
    return F.scaled_dot_product_attention(q, k, v, is_causal=True).permute(0, 2, 1, 3).reshape(B, S, H * D)


def _rel(a, b):
    return ((a - b).norm() / b.norm()).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("D", [32, 64])
@pytest.mark.parametrize("key_len", KEY_LENS)
def test_causal_reference_forward_and_gradients(D, dtype, key_len):
    qkv, dout = _inputs(D, dtype)
    kl = None if key_len is None else torch.tensor(key_len)
    x = qkv.clone().requires_grad_()
    out = attention(x, H, kl, causal=True)
    assert out.shape == (B, S, H * D) and out.dtype == dtype
    out.backward(dout)
    refs = [("explicit mask", _explicit)]
    if key_len is None:
        refs.append(("sdpa is_causal", lambda t, d, _k: _sdpa(t, d)))
    for name, fn in refs:
        y = qkv.clone().requires_grad_()
        ref = fn(y, D, key_len)
        ref.backward(dout)
        e_out, e_grad = _rel(out.detach(), ref.detach()), _rel(x.grad, y.grad)
        print(f"[causal-cpu] D={D} {dtype} key_len={key_len} vs {name}: out {e_out:.2e} grad {e_grad:.2e}")
        assert e_out < TOL[dtype], (name, e_out)
        assert e_grad < TOL[dtype], (name, e_grad)


def test_causal_changes_the_result_and_hides_the_future():
    qkv, _ = _inputs(64, torch.float64)
    a = attention(qkv, H, causal=True)
    assert not torch.equal(a, attention(qkv, H))
    q2 = qkv.clone()
    q2[:, 40:] = torch.randn(B, S - 40, qkv.shape[2], dtype=torch.float64)
    assert torch.equal(a[:, :40], attention(q2, H, causal=True)[:, :40])
    v0 = qkv.reshape(B, S, 3, H * 64)[:, 0, 2]
    assert torch.allclose(a[:, 0], v0, rtol=0, atol=1e-15)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_causal_false_is_the_call_without_the_argument(dtype):
    qkv, _ = _inputs(64, dtype)
    kl = torch.tensor([70, 1, 33])
    assert torch.equal(attention(qkv, H, kl, causal=False), attention(qkv, H, kl))
    assert torch.equal(attention(qkv, H, causal=False), attention(qkv, H))
