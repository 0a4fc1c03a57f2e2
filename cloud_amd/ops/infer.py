"""Inference form of convolution + BatchNorm (+ residual) (+ ReLU): one kernel launch.

A frozen or eval-mode BatchNorm is the per-channel affine ``z * scale + shift`` with
``scale = gamma / sqrt(running_var + eps)`` and ``shift = beta - running_mean * scale``.
:func:`conv_bn_act_infer` applies it in the convolution's epilogue
(``ca_conv_fwd_bn``, ``csrc/kernels/conv.hip``): fp32 on the accumulators, then the
residual add and the ReLU on the way out -- the convolution output is never written
and re-read, and no BN-statistics partials are computed.

The scale stays an fp32 epilogue multiply; it is never folded into a copy of the bf16
weights, which ``load_weights`` / ``set_weights`` would leave stale.

No autograd node: this is for the forward of a model that has no backward (eval, or
a frozen base under ``torch.no_grad()``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _ext
from .conv import _conv_mode, _native_conv_ok, _out

ACT_NONE, ACT_RELU = 0, 2  # csrc/include/ca_mfma_core.h enum Act


def conv_bn_act_infer(x, w, bn_scale, bn_shift, *, stride=1, padding=0, residual=None, relu=True):
    """y = act(conv(x, w) * bn_scale[c] + bn_shift[c] (+ residual)).

    x: NHWC ``[N, H, W, Cin]``, w: ``[Cout, KH, KW, Cin]``, bn_scale / bn_shift: fp32
    ``[Cout]``, residual: NHWC of the output's shape in x's dtype or None.  bf16 CUDA
    tensors run on the gfx950 kernel; anything else computes the same formula in torch."""
    assert not torch.is_grad_enabled() and not x.requires_grad and not w.requires_grad, \
        "conv_bn_act_infer has no backward: call it under torch.no_grad() on tensors that need no gradient " \
        "(pass a trainable weight as w.detach())"
    N, H, W, Cin = x.shape
    Cout, KH, KW, Cin_w = w.shape
    assert Cin == Cin_w, f"channel mismatch {Cin} vs {Cin_w}"
    OH, OW = _out(H, KH, stride, padding), _out(W, KW, stride, padding)
    if residual is not None:
        assert tuple(residual.shape) == (N, OH, OW, Cout) and residual.dtype == x.dtype, \
            "the residual must have the output's shape and dtype"
    if _conv_mode() == "native" and x.is_cuda and _native_conv_ok(x, w) and _ext.use_native(x, w):
        from . import raw

        return raw.conv_fwd_bn(x, w, bn_scale, bn_shift, stride, padding, residual=residual, relu=relu)
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, stride=stride, padding=padding)
    y = y.permute(0, 2, 3, 1).float() * bn_scale.float() + bn_shift.float()
    if residual is not None:
        y = y + residual.float()
    if relu:
        y = torch.relu(y)
    return y.to(x.dtype).contiguous()
