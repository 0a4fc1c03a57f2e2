"""Depthwise convolution (Keras ``DepthwiseConv2D`` / the first half of ``SeparableConv2D``)
on the streaming kernels of ``csrc/kernels/dwconv.hip`` -- no MIOpen, no per-shape JIT.

* activations NHWC ``[N, H, W, Cin]``; weight ``[KH, KW, Cin, DM]`` (the Keras layout, DM the
  depth multiplier): output channel ``o = c * DM + m`` reads input channel ``c``;
* forward ``y = act(dwconv(x, w) + bias)`` in one launch (fp32 bias and the activation at the
  store).  Padding is carried as top / left pads plus the output size: a tap past the bottom /
  right edge contributes zero, so TF's asymmetric SAME split needs no padded copy;
* backward: ``g = dy * act'(.)`` (one elementwise pass), the gather-form input gradient, the
  two-launch deterministic weight gradient and the native column-sum for the bias.  Gradients
  of parameters that live in an optimizer arena are added there in place and the data-parallel
  engine is notified.

CPU tensors, fp32, activations the epilogue does not have, dilation != 1, kernels wider than
7 or strides above 4 take the PyTorch reference: ``F.conv2d(groups=Cin)`` on channels-last
views, with an explicit ``F.pad`` where the padding is asymmetric.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _ext, conv as _conv, raw
from .dense import _act_grad_dev, _bias_grad, _deliver, _pad2d, _pair2, _rup8, _torch_act, fusable


def _pads(padding):
    """int | (h, w) | ((top, bottom), (left, right)) -> ((top, bottom), (left, right))."""
    if isinstance(padding, int):
        return (padding, padding), (padding, padding)
    ph, pw = padding
    ph = (int(ph), int(ph)) if isinstance(ph, int) else (int(ph[0]), int(ph[1]))
    pw = (int(pw), int(pw)) if isinstance(pw, int) else (int(pw[0]), int(pw[1]))
    return ph, pw


class _DwConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pads, out_hw, act, wparam, bparam):
        bp = b.float().contiguous() if b is not None else None
        pre = None
        if act == "gelu":  # GELU' is taken at the pre-activation
            pre = torch.empty((x.shape[0], out_hw[0], out_hw[1], w.shape[2] * w.shape[3]), dtype=torch.bfloat16,
                              device=x.device)
        y = raw.dwconv_fwd(x, w, stride, pads, out_hw, bias=bp, act=act, pre=pre)
        ctx.save_for_backward(x, w, y, pre)
        ctx.cfg = (stride, pads, act)
        ctx.wparam, ctx.bparam, ctx.has_b = wparam, bparam, b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ext.load(required=True)
        x, w, y, pre = ctx.saved_tensors
        stride, pads, act = ctx.cfg
        Cout = y.shape[-1]
        Mo = y.numel() // Cout
        st = _ext.stream_handle(dy.device)
        if act in (None, "linear"):
            g = dy.contiguous()
        elif Cout % 8 == 0:
            src = pre if act == "gelu" else y
            g = _act_grad_dev(dy.reshape(Mo, Cout), src.reshape(Mo, Cout), Cout, Cout, act).view_as(y)
        else:
            # an odd channel count: the elementwise pass runs on the tensor as one row, padded
            # to the 8 elements its vectors take (one small copy of the saved operand)
            tot = y.numel()
            src = _pad2d((pre if act == "gelu" else y).reshape(1, tot), _rup8(tot))
            g = _act_grad_dev(dy.contiguous().reshape(1, tot), src, tot, _rup8(tot), act)[0, :tot].view_as(y)
        dx = dw = db = dwp = dbp = None
        if ctx.needs_input_grad[0]:
            dx = raw.dwconv_dgrad(g, w, x.shape, stride, pads)
        if ctx.needs_input_grad[1] or ctx.wparam is not None:
            # fp32 [KH*KW, Cout]; _deliver adds it into the (bf16) arena slot and notifies the DP engine
            full = raw.dwconv_wgrad(g, x, w.shape, stride, pads).view(-1, Cout)
            if ctx.wparam is not None:
                dwp = _deliver(ctx.wparam, full, full)
            else:
                dw = full.to(w.dtype).view_as(w)
        if ctx.has_b and (ctx.needs_input_grad[2] or ctx.bparam is not None):
            Np = _rup8(Cout)
            dbp, db = _bias_grad(ext, _pad2d(g.reshape(Mo, Cout), Np), Mo, Np, Cout, ctx.bparam, st)
        return dx, dw, db, None, None, None, None, dwp, dbp


def _reference(x, w, bias, stride, pads, out_hw, act, dilation):
    (pt, pb), (pl, pr) = pads
    KH, KW, Cin, DM = w.shape
    dh, dw_ = dilation
    if out_hw is not None:  # the output size decides how much of the bottom / right edge is read
        pb = (out_hw[0] - 1) * stride[0] + dh * (KH - 1) + 1 - x.shape[1] - pt
        pr = (out_hw[1] - 1) * stride[1] + dw_ * (KW - 1) + 1 - x.shape[2] - pl
    xc = x.permute(0, 3, 1, 2)
    if pt == pb and pl == pr and pt >= 0 and pl >= 0:
        padding = (pt, pl)
    else:
        xc, padding = F.pad(xc, (pl, pr, pt, pb)), (0, 0)
    # [KH, KW, Cin, DM] -> [Cin*DM, 1, KH, KW]: group c holds its DM filters, o = c*DM + m
    wc = w.to(x.dtype).permute(2, 3, 0, 1).reshape(Cin * DM, 1, KH, KW)
    y = F.conv2d(xc, wc, None, stride, padding, dilation, groups=Cin).permute(0, 2, 3, 1).contiguous()
    if bias is not None:
        y = y + bias.to(y.dtype)
    return _torch_act(y, act)


def depthwise_conv2d(x, w, bias=None, stride=1, padding=0, act=None, out_hw=None, dilation=1):
    """``act(depthwise_conv2d_nhwc(x, w) + bias)``: x [N, H, W, Cin], w [KH, KW, Cin, DM], bias
    [Cin*DM] (fp32 or the compute dtype) -> [N, OH, OW, Cin*DM].

    ``stride`` is an int or an (h, w) pair; ``padding`` an int, an (h, w) pair or
    ((top, bottom), (left, right)).  ``out_hw`` = (OH, OW) overrides the output size the pads
    imply (rows / columns past the bottom / right edge read as zero).  The native route runs
    for CUDA bf16 operands, a fusable activation and ``dilation == 1``; the returned tensor is
    bf16.  Otherwise PyTorch computes the same expression."""
    stride, dilation = _pair2(stride), _pair2(dilation)
    pads = _pads(padding)
    KH, KW, Cin, DM = w.shape
    if x.shape[-1] != Cin:
        raise ValueError(f"depthwise_conv2d: channel mismatch {x.shape[-1]} vs {Cin}")
    if out_hw is not None:
        out_hw = (int(out_hw[0]), int(out_hw[1]))
    if (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and fusable(act)
            and dilation == (1, 1) and KH <= 7 and KW <= 7 and max(stride) <= 4 and min(pads[0] + pads[1]) >= 0
            and _conv._conv_mode() == "native" and x.shape[0] > 0 and x.numel() < 2 ** 31
            and _ext.use_native(x, w)):
        if out_hw is None:
            out_hw = ((x.shape[1] + sum(pads[0]) - KH) // stride[0] + 1,
                      (x.shape[2] + sum(pads[1]) - KW) // stride[1] + 1)
        if out_hw[0] < 1 or out_hw[1] < 1:
            raise ValueError(f"depthwise_conv2d: empty output {out_hw}")
        wparam = w if (w.is_leaf and w.requires_grad) else None
        bparam = bias if (bias is not None and bias.is_leaf and bias.requires_grad) else None
        return _DwConvFn.apply(x.contiguous(), (w.detach() if wparam is not None else w).contiguous(),
                               None if bias is None else (bias.detach() if bparam is not None else bias), stride,
                               (pads[0][0], pads[1][0]), out_hw, act, wparam, bparam)
    return _reference(x, w, bias, stride, pads, out_hw, act, dilation)
