"""Fused multi-head attention (K13): self-attention over a packed QKV projection, and
cross-attention of a query projection against a packed K | V projection.

``attention(qkv, num_heads, key_len, causal=...)`` computes, per batch entry and head,
``softmax(Q K^T * scale + key mask [+ causal mask]) (dropout) V`` for ``qkv: [B, S, 3*H*D]`` packed
``Q | K | V`` with head ``h`` at columns ``h*D`` of each third -- the layout the QKV
projection produces and the kernels of ``csrc/kernels/attn.hip`` read in place.  The
result is ``[B, S, H*D]``.

On MI355X (contiguous bf16 CUDA tensors, ``D`` in ``raw.ATTN_HEAD_DIMS`` = 32, 64, 128) forward
and backward run on the gfx950 MFMA kernels at any sequence length (D = 64 at S = 64 / 128 on the
one-workgroup kernels);
with ``causal=True`` they skip the 64x64 score blocks that lie entirely in the future.  The
backward recomputes the probabilities from the saved log-sum-exp and regenerates the
dropout mask from the saved seed.  CPU tensors, other dtypes and other head dimensions run
the same math in fp32 PyTorch.

``cross_attention(q, kv, num_heads, key_len)`` is the same computation for queries and keys /
values of different sources and lengths: ``q: [B, T, H*D]``, ``kv: [B, S, 2*H*D]`` packed
``K | V``, result ``[B, T, H*D]``; it runs on the cross-attention kernels of the same file at
any ``T`` and ``S`` under the same conditions.

Both take ``mask=``, a boolean attention mask (True = the query may see the key) of shape
``[S]``, ``[T, S]``, ``[B|1, T|1, S]`` or ``[B|1, H|1, T|1, S]``, which composes with ``key_len``
(and ``causal``).  Natively the mask is read by the cross-attention kernels as bytes through
broadcast strides, nothing is expanded; masked self-attention runs on them through the views
``qkv[..., :C]`` and ``qkv[..., C:]``.  A query row that may see no key at all has a zero
context row and sends zero gradients, on both paths.
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
        out, lse = raw.attn_fwd(q2, B, S, H, key_len, p, seed, scale=scale, causal=causal,
                                head_dim=q2.shape[1] // (3 * H))
        ctx.save_for_backward(q2, out, lse, key_len)
        ctx.cfg = (B, S, H, scale, p, seed, causal)
        return out.view(B, S, -1)

    @staticmethod
    def backward(ctx, dout):
        q2, out, lse, key_len = ctx.saved_tensors
        B, S, H, scale, p, seed, causal = ctx.cfg
        dout = dout.contiguous().view(B * S, -1)
        dqkv = raw.attn_bwd(q2, out, dout, lse, B, S, H, key_len, p, seed, scale=scale, causal=causal,
                            head_dim=q2.shape[1] // (3 * H))
        return dqkv.view(B, S, -1), None, None, None, None, None, None


class _MaskedAttentionFn(torch.autograd.Function):
    """Self-attention under a mask: the cross-attention kernels on the Q and K | V column views of
    the packed projection (row pitch 3C), dqkv = dq | dkv."""

    @staticmethod
    def forward(ctx, qkv, key_len, mask, H, scale, p, seed):
        B, S, C3 = qkv.shape
        q2 = qkv.view(B * S, C3)
        C = C3 // 3
        out, lse = raw.attn_cross_fwd(q2[:, :C], q2[:, C:], B, S, S, H, key_len, p, seed, scale=scale, mask=mask,
                                      head_dim=C // H)
        ctx.save_for_backward(q2, out, lse, key_len, mask)
        ctx.cfg = (B, S, H, scale, p, seed)
        return out.view(B, S, -1)

    @staticmethod
    def backward(ctx, dout):
        q2, out, lse, key_len, mask = ctx.saved_tensors
        B, S, H, scale, p, seed = ctx.cfg
        C = q2.shape[1] // 3
        dout = dout.contiguous().view(B * S, -1)
        dq, dkv = raw.attn_cross_bwd(q2[:, :C], q2[:, C:], out, dout, lse, B, S, S, H, key_len, p, seed, scale=scale,
                                     mask=mask, head_dim=C // H)
        return torch.cat([dq, dkv], dim=1).view(B, S, -1), None, None, None, None, None, None


def _mask4(mask, B, H, T, S, device, who):
    """``mask`` ([S], [T, S], [B|1, T|1, S] or [B|1, H|1, T|1, S]; bool, True = visible) as a 4-D
    ``[B|1, H|1, T|1, S]`` view with unit key stride.  Nothing is expanded: only a mask whose key
    stride is not 1 is copied, in its own (unexpanded) shape."""
    m = torch.as_tensor(mask)
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError(f"{who}: mask must be boolean (True = the query may see the key), got {m.dtype}")
    if not 1 <= m.dim() <= 4:
        raise ValueError(f"{who}: mask must be [S], [T, S], [B|1, T|1, S] or [B|1, H|1, T|1, S], got {tuple(m.shape)}")
    if m.dim() == 3:
        m = m[:, None]  # heads
    while m.dim() < 4:
        m = m[None]
    if m.shape[3] != S or any(n not in (1, full) for n, full in zip(m.shape, (B, H, T))):
        raise ValueError(f"{who}: mask {tuple(torch.as_tensor(mask).shape)} does not broadcast to "
                         f"[B, H, T, S] = {[B, H, T, S]} (the key axis is never broadcast)")
    m = m.to(device)
    if S > 1 and m.stride(3) != 1:
        m = m.contiguous()
    return m if m.dtype == torch.bool else m != 0


def _masked_softmax(att, allowed):
    """softmax over the allowed keys; a row with none is all zeros and sends no gradient (its
    scores stay finite, so neither the softmax nor its backward sees a NaN)."""
    live = allowed.any(-1, keepdim=True)
    att = att.masked_fill(~allowed & live, float("-inf"))
    return att.softmax(-1) * (allowed & live)


def _reference(qkv, H, key_len, scale, p, causal=False, mask=None):
    B, S, C3 = qkv.shape
    D = C3 // (3 * H)
    ct = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    q, k, v = qkv.to(ct).reshape(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    att = (q @ k.transpose(-1, -2)) * scale
    if mask is not None:
        allowed = mask  # [B|1, H|1, S|1, S] bool
        if key_len is not None:
            kl = key_len.to(device=qkv.device, dtype=torch.long).clamp(1, S)
            allowed = allowed & (torch.arange(S, device=qkv.device)[None, :] < kl[:, None])[:, None, None, :]
        if causal:
            allowed = allowed & torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
        att = _masked_softmax(att, allowed)
        if p > 0:
            att = F.dropout(att, p, training=True)
        return (att @ v).permute(0, 2, 1, 3).reshape(B, S, H * D).to(qkv.dtype)
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


def attention(qkv, num_heads, key_len=None, dropout_p=0.0, training=True, scale=None, seed=None, causal=False,
              mask=None):
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

    ``mask``: boolean, True = the query may see the key; ``[S]`` (keys), ``[S, S]`` (query, key),
    ``[B|1, S|1, S]`` or ``[B|1, H|1, S|1, S]``.  It composes with ``key_len`` and ``causal``.  With a
    mask a query row can lose every key: such a row has a zero context row and sends zero
    gradients.  Natively a masked call runs on the cross-attention kernels, which read the views
    ``qkv[..., :C]`` and ``qkv[..., C:]`` in place and the mask through broadcast strides (no
    expansion); at S = 64 / 128 it therefore does not take the one-workgroup kernels (which are
    for D = 64 only; the other head dimensions run the generic kernels at every S).
    ``causal=True`` together with a mask ANDs a lower-triangular ``[S, S]`` into the mask in
    PyTorch: that materialises a byte mask of up to ``[B, H, S, S]`` per call and gives up the
    block skipping of the causal kernels (every 64x64 block is computed).  ``mask=None`` runs
    exactly what it ran before the argument existed.
    """
    if qkv.dim() != 3 or qkv.shape[2] % (3 * num_heads):
        raise ValueError(f"attention: qkv must be [B, S, 3*H*D] with H = {num_heads}, got {tuple(qkv.shape)}")
    D = qkv.shape[2] // (3 * num_heads)
    scale = 1.0 / math.sqrt(D) if scale is None else float(scale)
    p = float(dropout_p) if training else 0.0
    if mask is not None:
        B, S = qkv.shape[0], qkv.shape[1]
        m4 = _mask4(mask, B, num_heads, S, S, qkv.device, "attention")
        if (qkv.dtype == torch.bfloat16 and D in raw.ATTN_HEAD_DIMS and B > 0 and S > 0 and qkv.is_contiguous()
                and _ext.use_native(qkv)):
            if causal:
                m4 = m4 & torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
            kl = None if key_len is None else key_len.to(device=qkv.device, dtype=torch.int32).contiguous()
            if p > 0 and seed is None:
                seed = next_seed()
            return _MaskedAttentionFn.apply(qkv, kl, m4, num_heads, scale, p, int(seed) if p > 0 else 0)
        return _reference(qkv, num_heads, key_len, scale, p, bool(causal), m4)
    if (qkv.dtype == torch.bfloat16 and D in raw.ATTN_HEAD_DIMS and qkv.shape[0] > 0 and qkv.shape[1] > 0
            and qkv.is_contiguous() and _ext.use_native(qkv)):
        kl = None if key_len is None else key_len.to(device=qkv.device, dtype=torch.int32).contiguous()
        if p > 0 and seed is None:
            seed = next_seed()
        return _AttentionFn.apply(qkv, kl, num_heads, scale, p, int(seed) if p > 0 else 0, bool(causal))
    return _reference(qkv, num_heads, key_len, scale, p, bool(causal))


class _CrossAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, kv, key_len, H, scale, p, seed, mask=None):
        B, T, _ = q.shape
        S = kv.shape[1]
        q2, kv2 = q.view(B * T, -1), kv.view(B * S, -1)
        out, lse = raw.attn_cross_fwd(q2, kv2, B, T, S, H, key_len, p, seed, scale=scale, mask=mask,
                                      head_dim=q2.shape[1] // H)
        ctx.save_for_backward(q2, kv2, out, lse, key_len, mask)
        ctx.cfg = (B, T, S, H, scale, p, seed)
        return out.view(B, T, -1)

    @staticmethod
    def backward(ctx, dout):
        q2, kv2, out, lse, key_len, mask = ctx.saved_tensors
        B, T, S, H, scale, p, seed = ctx.cfg
        dout = dout.contiguous().view(B * T, -1)
        dq, dkv = raw.attn_cross_bwd(q2, kv2, out, dout, lse, B, T, S, H, key_len, p, seed, scale=scale, mask=mask,
                                     head_dim=q2.shape[1] // H)
        return dq.view(B, T, -1), dkv.view(B, S, -1), None, None, None, None, None, None


def _cross_reference(q, kv, H, key_len, scale, p, mask=None):
    B, T, C = q.shape
    S, D = kv.shape[1], C // H
    ct = torch.float64 if q.dtype == torch.float64 else torch.float32
    qh = q.to(ct).reshape(B, T, H, D).transpose(1, 2)  # [B, H, T, D]
    k, v = kv.to(ct).reshape(B, S, 2, H, D).permute(2, 0, 3, 1, 4)  # [B, H, S, D] each
    att = (qh @ k.transpose(-1, -2)) * scale
    if mask is not None:
        allowed = mask  # [B|1, H|1, T|1, S] bool
        if key_len is not None:
            kl = key_len.to(device=q.device, dtype=torch.long).clamp(1, S)
            allowed = allowed & (torch.arange(S, device=q.device)[None, :] < kl[:, None])[:, None, None, :]
        att = _masked_softmax(att, allowed)
        if p > 0:
            att = F.dropout(att, p, training=True)
        return (att @ v).transpose(1, 2).reshape(B, T, C).to(q.dtype)
    if key_len is not None:
        kl = key_len.to(device=q.device, dtype=torch.long).clamp(1, S)
        pad = torch.arange(S, device=q.device)[None, :] >= kl[:, None]
        att = att.masked_fill(pad[:, None, None, :], float("-inf"))
    att = att.softmax(-1)
    if p > 0:
        att = F.dropout(att, p, training=True)
    return (att @ v).transpose(1, 2).reshape(B, T, C).to(q.dtype)


def cross_attention(q, kv, num_heads, key_len=None, dropout_p=0.0, training=True, scale=None, seed=None, mask=None):
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
    ``attention(..., causal=True)``; a causal cross-attention is a ``mask``, with the alignment the
    caller builds into it (``torch.ones(T, S, dtype=torch.bool).tril()`` is the top-left one).

    ``mask``: boolean, True = the query may see the key; ``[S]`` (keys), ``[T, S]``,
    ``[B|1, T|1, S]`` or ``[B|1, H|1, T|1, S]``.  A score takes part iff its key is below
    ``key_len`` and the mask allows it.  The kernels read the mask as bytes through broadcast
    strides: size-1 axes are never expanded, and only a mask whose key stride is not 1 is copied
    (in its own shape).  A query row that may see no key has a zero context row and sends zero
    gradients to ``q`` and ``kv`` (a softmax over nothing is defined as all zeros, on both paths);
    a key no query sees gets zero gradients.

    bf16 CUDA tensors with ``D`` in ``raw.ATTN_HEAD_DIMS`` (32, 64, 128) run on the gfx950 kernels,
    forward and backward
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
    m4 = None if mask is None else _mask4(mask, q.shape[0], H, q.shape[1], kv.shape[1], q.device, "cross_attention")
    if (q.dtype == torch.bfloat16 and D in raw.ATTN_HEAD_DIMS and q.numel() > 0 and kv.numel() > 0
            and _ext.use_native(q, kv)):
        kl = None if key_len is None else key_len.to(device=q.device, dtype=torch.int32).contiguous()
        if p > 0 and seed is None:
            seed = next_seed()
        if m4 is None:
            return _CrossAttentionFn.apply(q.contiguous(), kv.contiguous(), kl, H, scale, p, int(seed) if p > 0 else 0)
        return _CrossAttentionFn.apply(q.contiguous(), kv.contiguous(), kl, H, scale, p, int(seed) if p > 0 else 0, m4)
    return _cross_reference(q, kv, H, key_len, scale, p, m4)
