"""Fused multi-head attention (K13): self-attention over a packed QKV projection, and
cross-attention of a query projection against a packed K | V projection.

``attention(qkv, num_heads, key_len, causal=...)`` computes, per batch entry and head,
``softmax(Q K^T * scale + key mask [+ causal mask]) (dropout) V`` for ``qkv: [B, S, 3*H*D]`` packed
``Q | K | V`` with head ``h`` at columns ``h*D`` of each third -- the layout the QKV
projection produces and the kernels of ``csrc/kernels/attn.hip`` read in place.  The
result is ``[B, S, H*D]``.

On MI355X (contiguous bf16 CUDA tensors, ``D == 64``) forward and backward run on the
gfx950 MFMA kernels at any sequence length (S = 64 / 128 on the one-workgroup kernels);
with ``causal=True`` they skip the 64x64 score blocks that lie entirely in the future.  The
backward recomputes the probabilities from the saved log-sum-exp and regenerates the
dropout mask from the saved seed.  CPU tensors, other dtypes and other head dimensions run
the same math in fp32 PyTorch.

``cross_attention(q, kv, num_heads, key_len)`` is the same computation for queries and keys /
values of different sources and lengths: ``q: [B, T, H*D]``, ``kv: [B, S, 2*H*D]`` packed
``K | V``, result ``[B, T, H*D]``; it runs on the cross-attention kernels of the same file at
any ``T`` and ``S`` under the same conditions.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from . import _ext, raw
from .dropout import next_seed


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, key_len, H, scale, p, seed, causal):
        B, S, _ = qkv.shape
        q2 = qkv.view(B * S, -1)
        out, lse = raw.attn_fwd(q2, B, S, H, key_len, p, seed, scale=scale, causal=causal)
        ctx.save_for_backward(q2, out, lse, key_len)
        ctx.cfg = (B, S, H, scale, p, seed, causal)
        return out.view(B, S, -1)

    @staticmethod
    def backward(ctx, dout):
        q2, out, lse, key_len = ctx.saved_tensors
        B, S, H, scale, p, seed, causal = ctx.cfg
        dout = dout.contiguous().view(B * S, -1)
        dqkv = raw.attn_bwd(q2, out, dout, lse, B, S, H, key_len, p, seed, scale=scale, causal=causal)
        return dqkv.view(B, S, -1), None, None, None, None, None, None


def _reference(qkv, H, key_len, scale, p, causal=False):
    B, S, C3 = qkv.shape
    D = C3 // (3 * H)
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    q, k, v = qkv.to(ct).reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    att = (q @ k.transpose(-1, -2)) * scale
    if key_len is not None:
        kl = key_len.to(device=qkv.device, dtype=torch.long).clamp(1, S)
        pad = torch.arange(S, device=qkv.device)[None, :] >= kl[:, None]
        att = att.masked_fill(pad[:, None, None, :], float("-inf"))
    if causal:
        future = torch.ones(S, S, dtype=torch.bool, device=qkv.device).triu(1)  # [q, key]: key > q
        att = att.masked_fill(future, float("-inf"))
    att = att.softmax(-1)
    if p > 0:
        att = F.dropout(att, p, training=True)
    return (att @ v).permute(0, 2, 1, 3).reshape(B, S, H * D).to(qkv.dtype)


def attention(qkv, num_heads, key_len=None, dropout_p=0.0, training=True, scale=None, seed=None, causal=False):
    """Multi-head self-attention of a packed projection ``qkv [B, S, 3*H*D]`` -> ``[B, S, H*D]``.

    ``key_len``: int tensor ``[B]``, the number of valid (leading) keys of each batch entry,
    clamped to ``[1, S]``; ``None`` = all keys.  ``causal``: query ``i`` sees key ``j`` only if
    ``j <= i`` (and ``j < key_len``); key 0 is visible to every query, so no row is fully masked.
    ``scale`` defaults to ``1 / sqrt(D)``.
    Dropout acts on the attention probabilities, only when ``training``; ``seed`` (an int)
    fixes the mask of the native path and defaults to ``ops.dropout.next_seed()``.

    The two paths draw different dropout masks: the HIP kernels hash ``(seed, element
    index)`` (``raw.dropout_mask`` reproduces it), the PyTorch reference uses ``F.dropout``
    and the torch generator, and ignores ``seed``.
    """
    if qkv.dim() != 3 or qkv.shape[2] % (3 * num_heads):
        raise ValueError(f"attention: qkv must be [B, S, 3*H*D] with H = {num_heads}, got {tuple(qkv.shape)}")
    D = qkv.shape[2] // (3 * num_heads)
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    p = float(dropout_p) if training else 0.0
    if (qkv.dtype == torch.bfloat16 and D == 64 and qkv.shape[0] > 0 and qkv.shape[1] > 0 and qkv.is_contiguous()
            and _ext.use_native(qkv)):
        kl = None if key_len is None else key_len.to(device=qkv.device, dtype=torch.int32).contiguous()
        if p > 0 and seed is None:
            seed = next_seed()
        return _AttentionFn.apply(qkv, kl, num_heads, scale, p, int(seed) if p > 0 else 0, bool(causal))
    return _reference(qkv, num_heads, key_len, scale, p, bool(causal))


class _CrossAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, key_len, H, scale, p, seed):
        B, T, _ = q.shape
        S = kv.shape[1]
        q2, kv2 = q.view(B * T, -1), kv.view(B * S, -1)
        out, lse = raw.attn_cross_fwd(q2, kv2, B, T, S, H, key_len, p, seed, scale=scale)
        ctx.save_for_backward(q2, kv2, out, lse, key_len)
        ctx.cfg = (B, T, S, H, scale, p, seed)
        return out.view(B, T, -1)

    @staticmethod
    def backward(ctx, dout):
        q2, kv2, out, lse, key_len = ctx.saved_tensors
        B, T, S, H, scale, p, seed = ctx.cfg
        dout = dout.contiguous().view(B * T, -1)
        dq, dkv = raw.attn_cross_bwd(q2, kv2, out, dout, lse, B, T, S, H, key_len, p, seed, scale=scale)
        return dq.view(B, T, -1), dkv.view(B, S, -1), None, None, None, None, None


def _cross_reference(q, kv, H, key_len, scale, p):
    B, T, C = q.shape
    S, D = kv.shape[1], C // H
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    qh = q.to(ct).reshape(B, T, H, D).transpose(1, 2)  # [B, H, T, D]
    k, v = kv.to(ct).reshape(B, S, 2, H, D).permute(2, 0, 3, 1, 4)  # [B, H, S, D] each
    att = (qh @ k.transpose(-1, -2)) * scale
    if key_len is not None:
        kl = key_len.to(device=q.device, dtype=torch.long).clamp(1, S)
        pad = torch.arange(S, device=q.device)[None, :] >= kl[:, None]
        att = att.masked_fill(pad[:, None, None, :], float("-inf"))
    att = att.softmax(-1)
    if p > 0:
        att = F.dropout(att, p, training=True)
    return (att @ v).transpose(1, 2).reshape(B, T, C).to(q.dtype)


def cross_attention(q, kv, num_heads, key_len=None, dropout_p=0.0, training=True, scale=None, seed=None):
    """Multi-head cross-attention: queries ``q [B, T, H*D]`` against the packed key / value
    projection ``kv [B, S, 2*H*D]`` (``K | V``, head ``h`` at columns ``h*D`` of each half) ->
    ``[B, T, H*D]``.  ``T`` and ``S`` are independent.

    ``key_len``: int tensor ``[B]``, a prefix mask: the number of valid (leading) keys of each
    batch entry, clamped to ``[1, S]``; ``None`` = all keys.  ``scale`` defaults to
    ``1 / sqrt(D)``.  Dropout acts on the attention probabilities, only when ``training``;
    ``seed`` (an int) fixes the mask of the native path and defaults to
    ``ops.dropout.next_seed()``.

    There is no ``causal`` argument: how a causal mask is aligned when ``T != S`` (top-left or
    bottom-right) is a convention this op does not choose.  Causal self-attention is
    ``attention(..., causal=True)``.

    bf16 CUDA tensors with ``D == 64`` run on the gfx950 kernels, forward and backward
    (non-contiguous inputs are made contiguous first); everything else (CPU, other dtypes,
    other head dimensions) runs the same math in fp32 PyTorch (fp64 for fp64 inputs).  The two
    paths draw different dropout masks: the HIP kernels hash ``(seed, element index)`` with
    the index ``(b*H + h)*T*S + q*S + key`` (``raw.dropout_mask`` reproduces it), the PyTorch
    reference uses ``F.dropout`` and the torch generator, and ignores ``seed``.
    """
    H = int(num_heads)
    if q.dim() != 3 or H < 1 or q.shape[2] % H:
        raise ValueError(f"cross_attention: q must be [B, T, H*D] with H = {num_heads}, got {tuple(q.shape)}")
    if kv.dim() != 3 or kv.shape[2] % (2 * H):
        raise ValueError(f"cross_attention: kv must be [B, S, 2*H*D] with H = {num_heads}, got {tuple(kv.shape)}")
    if kv.shape[0] != q.shape[0]:
        raise ValueError(f"cross_attention: q and kv differ in batch size: {tuple(q.shape)}, {tuple(kv.shape)}")
    if kv.shape[2] != 2 * q.shape[2]:
        raise ValueError("cross_attention: q and kv differ in head dimension: "
                         f"{q.shape[2] // H} and {kv.shape[2] // (2 * H)}")
    if kv.dtype != q.dtype:
        raise ValueError(f"cross_attention: q and kv differ in dtype: {q.dtype}, {kv.dtype}")
    D = q.shape[2] // H
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    p = float(dropout_p) if training else 0.0
    if q.dtype == torch.bfloat16 and D == 64 and q.numel() > 0 and kv.numel() > 0 and _ext.use_native(q, kv):
        kl = None if key_len is None else key_len.to(device=q.device, dtype=torch.int32).contiguous()
        if p > 0 and seed is None:
            seed = next_seed()
        return _CrossAttentionFn.apply(q.contiguous(), kv.contiguous(), kl, H, scale, p, int(seed) if p > 0 else 0)
    return _cross_reference(q, kv, H, key_len, scale, p)
