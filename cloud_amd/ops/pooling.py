"""NHWC pooling ops (K7): max / average pooling at any window and the global pools.

HIP path: ``csrc/kernels/pool.hip`` (square symmetric max pool with ``C % 8 == 0``, global
pools, the fused ResNet stem tail) and ``csrc/kernels/pool2d.hip`` (max / average at any
window, stride, asymmetric pads and channel count).  CPU / torch-mode path: PyTorch NCHW ops on
permuted views.  Parity: Keras ``MaxPooling2D`` / ``AveragePooling2D`` / ``GlobalAveragePooling2D``
(reference ``core/tests/testdata/mnist_example_using_fit.py:58``,
``core/tests/examples/call_run_within_script_with_keras_fit.py:83``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import config
from . import _ext, raw
from .dense import _pair2
from .depthwise import _pads


def _out(n, k, s, p):
    return (n + 2 * p - k) // s + 1


class _MaxPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, p):
        ext = _ext.load(required=True)
        x = x.contiguous()
        N, H, W, C = x.shape
        OH, OW = _out(H, k, s, p), _out(W, k, s, p)
        y = torch.empty((N, OH, OW, C), dtype=x.dtype, device=x.device)
        idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=x.device)
        ext.maxpool_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, OH, OW, k, s, p,
                        _ext.stream_handle(x.device))
        ctx.save_for_backward(idx)
        ctx.cfg = (N, H, W, C, OH, OW, k, s, p)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ext.load(required=True)
        (idx,) = ctx.saved_tensors
        N, H, W, C, OH, OW, k, s, p = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((N, H, W, C), dtype=dy.dtype, device=dy.device)
        ext.maxpool_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), N, H, W, C, OH, OW, k, s, p,
                        _ext.stream_handle(dy.device))
        return dx, None, None, None


class _MaxPool2dFn(torch.autograd.Function):
    """Max pool at any window on ``pool2d.hip``: the argmax bytes are the only saved state."""

    @staticmethod
    def forward(ctx, x, k, s, pads, out_hw):
        y, idx = raw.pool2d_max_fwd(x, k, s, pads, out_hw)
        ctx.save_for_backward(idx)
        ctx.cfg = (tuple(x.shape), k, s, pads)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        x_shape, k, s, pads = ctx.cfg
        return raw.pool2d_max_bwd(dy.contiguous(), idx, x_shape, k, s, pads), None, None, None, None


class _AvgPool2dFn(torch.autograd.Function):
    """Average pool at any window on ``pool2d.hip`` (divisor: the in-image taps); nothing saved."""

    @staticmethod
    def forward(ctx, x, k, s, pads, out_hw):
        ctx.cfg = (tuple(x.shape), k, s, pads)
        return raw.pool2d_avg_fwd(x, k, s, pads, out_hw)

    @staticmethod
    def backward(ctx, dy):
        x_shape, k, s, pads = ctx.cfg
        return raw.pool2d_avg_bwd(dy.contiguous(), x_shape, k, s, pads), None, None, None, None


def _geometry(x, kernel_size, stride, padding, out_hw):
    """(kernel, stride, ((top, bottom), (left, right)), (OH, OW)) from the ops' argument forms;
    with ``out_hw`` the bottom / right pads are what that output size reads (negative: rows /
    columns the windows never reach)."""
    k = _pair2(kernel_size)
    s = k if stride is None else _pair2(stride)
    (pt, pb), (pl, pr) = _pads(padding)
    H, W = x.shape[1], x.shape[2]
    if out_hw is None:
        out_hw = ((H + pt + pb - k[0]) // s[0] + 1, (W + pl + pr - k[1]) // s[1] + 1)
    else:
        out_hw = (int(out_hw[0]), int(out_hw[1]))
        pb = (out_hw[0] - 1) * s[0] + k[0] - H - pt
        pr = (out_hw[1] - 1) * s[1] + k[1] - W - pl
    return k, s, ((pt, pb), (pl, pr)), out_hw


def _pool2d_native(x, k, s, pads, out_hw):
    """The calls that run on ``pool2d.hip``: CUDA bf16 NHWC, a geometry its launchers accept."""
    return (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4 and x.shape[0] > 0 and x.numel() < 2 ** 31
            and raw.pool2d_geom_ok(x.shape, k, s, (pads[0][0], pads[1][0]), out_hw) and _ext.use_native(x))


def max_pool2d_nhwc(x, kernel_size, stride=None, padding=0, out_hw=None):
    """Max pool of x [N, H, W, C] -> [N, OH, OW, C].  ``kernel_size`` and ``stride`` are ints or
    (h, w) pairs (``stride`` defaults to the window); ``padding`` an int, an (h, w) pair or
    ((top, bottom), (left, right)); padded taps never win.  ``out_hw`` = (OH, OW) overrides the
    output size the pads imply (taps past the bottom / right edge are skipped).

    A square window with one stride, one symmetric pad, no ``out_hw`` and ``C % 8 == 0`` runs on
    the kernels of ``pool.hip`` (the ResNet route); every other CUDA bf16 call whose windows all
    hold an in-image tap runs on ``pool2d.hip``; anything else is the same expression in PyTorch."""
    k, s, pads, ohw = _geometry(x, kernel_size, stride, padding, out_hw)
    (pt, pb), (pl, pr) = pads
    square = out_hw is None and k[0] == k[1] and s[0] == s[1] and pt == pb == pl == pr  # (k, s, p) says it all
    if square and x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0 and _ext.use_native(x):
        return _MaxPoolFn.apply(x, k[0], s[0], pt)
    if _pool2d_native(x, k, s, pads, ohw):
        return _MaxPool2dFn.apply(x.contiguous(), k, s, (pt, pl), ohw)
    xc = x.permute(0, 3, 1, 2)
    if square:
        y = F.max_pool2d(xc, k[0], s[0], pt)
    else:
        y = F.max_pool2d(F.pad(xc, (pl, pr, pt, pb), value=float("-inf")), k, s)
    return y.permute(0, 2, 3, 1).contiguous()


def avg_pool2d_nhwc(x, kernel_size, stride=None, padding=0, out_hw=None):
    """Average pool of x [N, H, W, C] -> [N, OH, OW, C] over the in-image taps of each window:
    padding is excluded from the divisor (TF's ``AveragePooling2D``).  Arguments as
    :func:`max_pool2d_nhwc`.  CUDA bf16 calls whose windows all hold an in-image tap run on
    ``pool2d.hip``; anything else is the same expression in PyTorch: the window sums of the
    zero-padded input over the window sums of a padded map of ones (fp32 sums for 16-bit inputs)."""
    k, s, pads, ohw = _geometry(x, kernel_size, stride, padding, out_hw)
    if _pool2d_native(x, k, s, pads, ohw):
        return _AvgPool2dFn.apply(x.contiguous(), k, s, (pads[0][0], pads[1][0]), ohw)
    (pt, pb), (pl, pr) = pads
    xc = x.permute(0, 3, 1, 2)
    wide = xc.float() if x.dtype in (torch.bfloat16, torch.float16) else xc
    ones = torch.ones((1, 1, x.shape[1], x.shape[2]), dtype=wide.dtype, device=x.device)
    total = F.avg_pool2d(F.pad(wide, (pl, pr, pt, pb)), k, s, divisor_override=1)
    count = F.avg_pool2d(F.pad(ones, (pl, pr, pt, pb)), k, s, divisor_override=1)
    y = total / count.clamp_(min=1)  # a window wholly in the padding: 0
    return y.to(x.dtype).permute(0, 2, 3, 1).contiguous()


class _GapFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = _ext.load(required=True)
        x = x.contiguous()
        N, H, W, C = x.shape
        y = torch.empty((N, C), dtype=x.dtype, device=x.device)
        ext.gap_fwd(x.data_ptr(), y.data_ptr(), 1, N, H * W, C, _ext.stream_handle(x.device))
        ctx.cfg = (N, H, W, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ext.load(required=True)
        N, H, W, C = ctx.cfg
        dy = dy.contiguous()
        dx = torch.empty((N, H, W, C), dtype=torch.bfloat16, device=dy.device)
        ext.gap_bwd(dy.data_ptr(), int(dy.dtype == torch.bfloat16), dx.data_ptr(), N, H * W, C,
                    _ext.stream_handle(dy.device))
        return dx


def global_avg_pool_nhwc(x):
    if x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0 and _ext.use_native(x):
        return _GapFn.apply(x)
    return x.mean(dim=(1, 2))


class _GmpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ext = _ext.load(required=True)
        x = x.contiguous()
        N, H, W, C = x.shape
        y = torch.empty((N, C), dtype=x.dtype, device=x.device)
        cnt = torch.empty((N, C), dtype=torch.float32, device=x.device)
        ext.gmp_fwd(x.data_ptr(), y.data_ptr(), cnt.data_ptr(), N, H * W, C, _ext.stream_handle(x.device))
        ctx.save_for_backward(x, y, cnt)
        ctx.mark_non_differentiable(cnt)
        return y

    @staticmethod
    def backward(ctx, dy):
        ext = _ext.load(required=True)
        x, y, cnt = ctx.saved_tensors
        N, H, W, C = x.shape
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        ext.gmp_bwd(dy.data_ptr(), int(dy.dtype == torch.bfloat16), x.data_ptr(), y.data_ptr(), cnt.data_ptr(),
                    dx.data_ptr(), N, H * W, C, _ext.stream_handle(dy.device))
        return dx


def global_max_pool_nhwc(x):
    """[N, H, W, C] -> [N, C] max over H, W (Keras GlobalMaxPooling2D); ties share the
    gradient evenly, as reduce_max / amax."""
    if x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0 and _ext.use_native(x):
        return _GmpFn.apply(x)
    return x.amax(dim=(1, 2))


class _StemTailFn(torch.autograd.Function):
    """maxpool3x3/2/1(relu(BN(z))) for the ResNet stem in one pass each way.

    Forward: the BN statistics come from the stem convolution's epilogue partials
    (statistics-only finalize), then ``bn_relu_maxpool_s2k3`` applies BN + ReLU while
    pooling -- the 112x112x64 BN output is never written.  Backward: the max-pool
    gradient is gated by ``pooled > 0`` (the ReLU derivative at the argmax pixel) and
    reduced into the BN-backward statistics by the same kernel, so the BN backward
    runs its apply pass only."""

    @staticmethod
    def forward(ctx, z, gamma, beta, running_mean, running_var, eps, momentum, partials):
        from . import raw

        ext = _ext.load(required=True)
        N, H, W, C = z.shape
        OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        stats = raw.bn_fwd_stats(z, gamma, beta, running_mean, running_var, eps, momentum, partials)
        y = torch.empty((N, OH, OW, C), dtype=torch.bfloat16, device=z.device)
        idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=z.device)
        ext.bn_relu_maxpool_s2k3(z.data_ptr(), stats[2 * C:].data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C,
                                 OH, OW, _ext.stream_handle(z.device))
        ctx.save_for_backward(z, stats, y, idx, gamma)
        ctx.has_beta = beta is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        from . import raw

        ext = _ext.load(required=True)
        z, stats, y, idx, gamma = ctx.saved_tensors
        N, H, W, C = z.shape
        OH, OW = y.shape[1], y.shape[2]
        dev = z.device
        dy = dy.contiguous()
        st = _ext.stream_handle(dev)
        parts = torch.empty((ext.maxpool_bnstats_parts(N, H, W, C), 2, C), dtype=torch.float32, device=dev)
        dgamma = torch.empty(C, dtype=torch.float32, device=dev) if gamma is not None else None
        dbeta = torch.empty(C, dtype=torch.float32, device=dev) if ctx.has_beta else None
        if config.get("CLOUD_AMD_STEM_BWD_RECOMPUTE"):
            # statistics pass, then the apply pass recomputes the pooled gradient g per 2x2 block:
            # g (N x H x W x C) is never written or read back
            ext.maxpool_bwd_s2k3_bnstats(dy.data_ptr(), y.data_ptr(), idx.data_ptr(), z.data_ptr(), 0,
                                         parts.data_ptr(), N, H, W, C, OH, OW, st)
            coef = raw.bn_bwd_coef(C, N * H * W, gamma, stats, parts, dgamma=dgamma, dbeta=dbeta)
            dz = torch.empty_like(z)
            ext.maxpool_bwd_s2k3_bnapply(dy.data_ptr(), y.data_ptr(), idx.data_ptr(), z.data_ptr(), coef.data_ptr(),
                                         dz.data_ptr(), N, H, W, C, OH, OW, st)
            return dz, dgamma, dbeta, None, None, None, None, None
        g = torch.empty_like(z)
        ext.maxpool_bwd_s2k3_bnstats(dy.data_ptr(), y.data_ptr(), idx.data_ptr(), z.data_ptr(),
                                     g.data_ptr(), parts.data_ptr(), N, H, W, C, OH, OW, st)
        dz, _ = raw.bn_bwd(g, None, z, gamma, stats, False, dgamma=dgamma, dbeta=dbeta, partials=parts)
        return dz, dgamma, dbeta, None, None, None, None, None


def stem_tail_ok(z, bn, pool, partials):
    return (bn.training and bn.relu and partials is not None and z.is_cuda and z.dtype == torch.bfloat16
            and z.is_contiguous() and z.shape[-1] % 8 == 0 and 256 % (z.shape[-1] // 8) == 0
            and z.shape[0] * z.shape[1] * z.shape[2] < 2 ** 31  # the kernels' 32-bit pixel indices
            and (pool.k, pool.stride, pool.padding) == (3, 2, 1) and _ext.use_native(z))


def stem_bn_relu_maxpool(z, bn, partials):
    """The ResNet stem tail ``maxpool(bn1(z))`` of a training step, fused (see _StemTailFn)."""
    return _StemTailFn.apply(z, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum, partials)


def stem_infer_ok(z, bn, pool):
    """The fused stem tail applies to an inference forward (no statistics, no backward)."""
    return (bn.relu and z.is_cuda and z.dtype == torch.bfloat16 and z.is_contiguous() and z.shape[-1] % 8 == 0
            and z.shape[0] * z.shape[1] * z.shape[2] < 2 ** 31 and not z.requires_grad
            and (pool.k, pool.stride, pool.padding) == (3, 2, 1) and _ext.use_native(z))


def stem_bn_relu_maxpool_infer(z, bn):
    """``maxpool(relu(bn(z)))`` of the ResNet stem with the BatchNorm in inference form: the
    same ``bn_relu_maxpool_s2k3`` pass as the training step, fed the folded running statistics
    (``bn.folded()``).  The argmax bytes it also writes feed a backward that never runs here."""
    ext = _ext.load(required=True)
    N, H, W, C = z.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, OH, OW, C), dtype=torch.bfloat16, device=z.device)
    idx = torch.empty((N, OH, OW, C), dtype=torch.uint8, device=z.device)  # scratch
    ext.bn_relu_maxpool_s2k3(z.data_ptr(), bn.folded().data_ptr(), y.data_ptr(), idx.data_ptr(), N, H, W, C, OH, OW,
                             _ext.stream_handle(z.device))
    return y
