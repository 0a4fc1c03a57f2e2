"""Layer normalisation over the last axis, with an optional fused residual add.

bf16 CUDA tensors run on the HIP kernels: the tuned one-wave-per-row pair of the BERT path
(``csrc/kernels/rowops.hip``) for ``C % 4 == 0``, ``C <= 1344`` and aligned operands (8 bytes
for activations, 16 for ``gamma`` / ``beta``), the any-width kernels
(``csrc/kernels/layernorm.hip``) for every other ``1 <= C <= 16384`` -- see
:func:`cloud_amd.ops.raw.layer_norm_fwd`.  The activation is read
and written in bf16 once; the row statistics are fp32 and two-pass (mean, then centred sum of
squares); the backward saves the bf16 pre-norm sum and the two fp32 statistics per row, not an
fp32 copy of the activation, and its ``gamma`` / ``beta`` gradients are summed in a fixed order
(bitwise reproducible).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _ext, raw

MAX_NATIVE_WIDTH = 16384
_CONST = {}


def _const(value, C, device):
    """ones / zeros [C] (fp32) handed to the kernels for ``gamma=None`` / ``beta=None``."""
    key = (value, C, str(device))
    t = _CONST.get(key)
    if t is None:
        t = _CONST[key] = torch.full((C,), value, dtype=torch.float32, device=device)
    return t


class _LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, residual):
        y, h, mean, rstd = raw.layer_norm_fwd(x, gamma, beta, eps, residual)
        ctx.save_for_backward(x if h is None else h, mean, rstd, gamma)
        ctx.has_residual = residual is not None
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        h, mean, rstd, gamma = ctx.saved_tensors
        dh, dgamma, dbeta = raw.layer_norm_bwd(dy.contiguous(), h, mean, rstd, gamma)
        need = ctx.needs_input_grad
        return (dh if need[0] else None, dgamma if need[1] else None, dbeta if need[2] else None, None,
                dh if ctx.has_residual and need[4] else None)


def layer_norm(x, gamma=None, beta=None, eps=1e-3, residual=None):
    """``LN(x + residual) * gamma + beta`` over the last axis of an N-D ``x`` (autograd).

    ``gamma`` / ``beta``: ``[C]`` vectors, ``None`` for ones / zeros (no gradient is returned
    for a ``None``).  ``residual``: a tensor of ``x``'s shape and dtype, added before the
    normalisation; its gradient equals ``x``'s.

    Routing: bf16 CUDA tensors with ``1 <= C <= 16384`` and at least one element run on the
    HIP kernels (non-contiguous inputs are made contiguous first; ``C`` needs no alignment, and
    a sliced, 2-byte-aligned ``x`` is taken as it is).  Everything else -- CPU, fp32 / fp64,
    wider rows, empty tensors, ``CLOUD_AMD_OPS=torch`` -- runs the reference expression
    ``F.layer_norm(h.float(), (C,), gamma, beta, eps).to(x.dtype)`` with ``h = x + residual``
    (fp64 inputs: ``F.layer_norm(h, ...)`` in fp64).

    Against an fp64 reference the kernels' ``y`` is within 1e-2 and ``dx`` within 2e-2 of a
    row's scale (bf16 outputs), the statistics within 1e-5 also on rows whose mean is far
    larger than their spread, ``dgamma`` / ``dbeta`` within 1e-2 in relative norm
    (tests/test_layer_norm_gpu.py).

    Raises ``ValueError``, before any launch, for a ``gamma`` / ``beta`` that is not ``[C]``
    and for a ``residual`` of another shape or dtype.
    """
    if x.dim() < 1:
        raise ValueError("layer_norm: x needs at least one axis")
    C = x.shape[-1]
    for name, p in (("gamma", gamma), ("beta", beta)):
        if p is not None and tuple(p.shape) != (C,):
            raise ValueError(f"layer_norm: {name} must have shape [{C}], got {tuple(p.shape)}")
    if residual is not None and (residual.shape != x.shape or residual.dtype != x.dtype):
        raise ValueError(f"layer_norm: residual must match x ({tuple(x.shape)}, {x.dtype}), got "
                         f"{tuple(residual.shape)}, {residual.dtype}")
    if (x.dtype == torch.bfloat16 and 1 <= C <= MAX_NATIVE_WIDTH and x.numel() > 0
            and _ext.use_native(x, residual, gamma, beta)):
        g = _const(1.0, C, x.device) if gamma is None else gamma.float().contiguous()
        b = _const(0.0, C, x.device) if beta is None else beta.float().contiguous()
        return _LayerNormFn.apply(x.contiguous(), g, b, float(eps),
                                  None if residual is None else residual.contiguous())
    h = x if residual is None else x + residual
    if x.dtype == torch.float64:
        return F.layer_norm(h, (C,), gamma, beta, eps)
    return F.layer_norm(h.float(), (C,), gamma, beta, eps).to(x.dtype)
