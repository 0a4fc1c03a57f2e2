"""Fused softmax + sparse categorical cross-entropy (K3/K12).

The HIP kernel computes loss rows, the correct-prediction flags AND the logits
gradient in the forward pass (one read of the logits); backward just scales
the stored gradient by the incoming loss-gradient.  Parity target:
``tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True)`` with
``SUM_OVER_BATCH_SIZE`` / ``compute_average_loss(global_batch_size=...)``
(reference ``core/tests/testdata/mnist_example_using_ctl.py:93-101``).

Three kernel routes: one block for a small batch, one wave per row for classifier heads
(xent.hip), one workgroup per row at vocabulary width and for the mean over valid tokens
(xent_vocab.hip: a language model's ``[B, T, V]`` logits, padding left out with
``ignore_index`` / ``denom="valid"``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import config
from . import _ext


# batches up to this many logits take the one-block kernel that also reduces the mean
# loss and the metric sums in place (xent.hip xent_batch_kernel): Keras fit batches, the
# BERT classifier head.  Larger ones (the ResNet-50 head, 1024 x 1000 per GPU) take the
# row-parallel kernel: one workgroup on 1M logits measured 0.98 ms vs 0.013 ms
# (profiles/r3_s14/rn_step_kernels.txt).
_BATCH_KERNEL_MAX = 1 << 17
# past _BATCH_KERNEL_MAX, rows at least this wide take the one-row-per-workgroup kernels of
# xent_vocab.hip (a language model's [tokens, vocab] logits) instead of the one-wave-per-row
# kernel; the default is the measured cross-over (docs/performance.md, "Cross-entropy at
# vocabulary width").  denom="valid" takes them at any size: its scale lives on the device.
_VOCAB_MIN_C = config.get("CLOUD_AMD_XENT_VOCAB_MIN_C")
_UNIT = {}


def unit_seed(device):
    """A persistent 1.0 to pass as ``torch.autograd.backward(loss, grad_tensors=...)``: the
    fused loss recognises it and hands its stored gradient on unscaled (no fill kernel for
    autograd's implicit ones, no multiply)."""
    key = str(device)
    t = _UNIT.get(key)
    if t is None:
        t = _UNIT[key] = torch.ones((), dtype=torch.float32, device=device)
    return t


def backward_with_seed(loss, seed):
    """``torch.autograd.backward(loss, grad_tensors=seed)`` without its Python-side shape
    check: in this torch that check imports ``torch.fx.experimental.symbolic_shapes`` -- and
    with it sympy, 0.86 s cold on the GPU box -- on the first seeded backward of every process
    (every tuner worker's first trial; scripts/debug/cold_trial.py)."""
    if loss.shape != seed.shape:
        raise ValueError(f"seed shape {tuple(seed.shape)} != loss shape {tuple(loss.shape)}")
    try:
        from torch.autograd.graph import _engine_run_backward
    except ImportError:  # pragma: no cover - other torch versions
        return torch.autograd.backward(loss, grad_tensors=seed)
    _engine_run_backward((loss,), (seed,), False, False, (), allow_unreachable=True, accumulate_grad=True)


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, denom, label_smoothing, acc, acc_w):
        # the `correct` output never receives a gradient: no zero tensor materialised for it
        ctx.set_materialize_grads(False)
        ext = _ext.load(required=True)
        B, C = logits.shape
        small = B * C <= _BATCH_KERNEL_MAX
        if isinstance(denom, str) or (not small and C >= _VOCAB_MIN_C):
            out, correct, dz = _vocab_forward(ext, logits, labels, denom, label_smoothing, acc, acc_w)
            ctx.save_for_backward(dz)
            ctx.mark_non_differentiable(correct)
            return out, correct
        # the one-block kernel takes strided rows (a padded head's [:, :C] view: no copy)
        z = logits if (small and logits.stride(1) == 1) else logits.contiguous()
        dev = z.device
        correct = torch.empty(B, dtype=torch.float32, device=dev)
        dz = torch.empty((B, C), dtype=z.dtype, device=dev)
        lab = labels.contiguous()
        if small:
            mean = torch.empty(1, dtype=torch.float32, device=dev)
            ext.softmax_xent_batch(z.data_ptr(), z.stride(0), int(z.dtype == torch.bfloat16), lab.data_ptr(), B, C,
                                   1.0 / float(denom), float(label_smoothing), mean.data_ptr(), correct.data_ptr(),
                                   dz.data_ptr(), _ext.ptr(acc), float(acc_w), _ext.stream_handle(dev))
            out = mean.view(())
        else:
            loss = torch.empty(B, dtype=torch.float32, device=dev)
            ext.softmax_xent(z.data_ptr(), int(z.dtype == torch.bfloat16), lab.data_ptr(), B, C,
                             1.0 / float(denom), float(label_smoothing), loss.data_ptr(), correct.data_ptr(),
                             dz.data_ptr(), _ext.stream_handle(dev))
            if acc is not None:
                acc += torch.stack([loss.sum(), correct.sum(), loss.new_tensor(float(B))]) * float(acc_w)
            out = loss.sum() / float(denom)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(correct)
        return out, correct

    @staticmethod
    def backward(ctx, gloss, _gcorrect):
        (dz,) = ctx.saved_tensors
        if gloss is None:  # (grads are not materialised)
            return None, None, None, None, None, None
        u = _UNIT.get(str(gloss.device))
        if u is not None and gloss.data_ptr() == u.data_ptr():
            return dz, None, None, None, None, None
        return dz * gloss.to(dz.dtype), None, None, None, None, None


def _vocab_forward(ext, logits, labels, denom, label_smoothing, acc, acc_w):
    """The xent_vocab.hip route: [count,] one workgroup per row, one finalising block.  Rows are
    read in place through their pitch (a padded head's [:, :C] view: no copy)."""
    B, C = logits.shape
    z = logits if (logits.stride(1) == 1 and (B == 1 or logits.stride(0) >= C)) else logits.contiguous()
    ldz = z.stride(0) if B > 1 else C
    dev = z.device
    st = _ext.stream_handle(dev)
    lab = labels.contiguous()
    # [row losses | correct flags | mean loss, count, 1 / max(count, 1)]
    ws = torch.empty(2 * B + 3, dtype=torch.float32, device=dev)
    loss, correct, mean, cnt = ws[:B], ws[B:2 * B], ws[2 * B:2 * B + 1], ws[2 * B + 1:]
    dz = torch.empty((B, C), dtype=z.dtype, device=dev)
    cnt_ptr = 0
    scale = 1.0
    if isinstance(denom, str):  # "valid": the scale is computed on the device
        ext.xent_vocab_count(lab.data_ptr(), B, C, cnt.data_ptr(), st)
        cnt_ptr = cnt.data_ptr()
    else:
        scale = 1.0 / float(denom)
    ext.xent_vocab(z.data_ptr(), ldz, int(z.dtype == torch.bfloat16), lab.data_ptr(), B, C, scale, cnt_ptr,
                   float(label_smoothing), loss.data_ptr(), correct.data_ptr(), dz.data_ptr(), st)
    ext.xent_vocab_finalize(loss.data_ptr(), correct.data_ptr(), B, scale, cnt_ptr, mean.data_ptr(), _ext.ptr(acc),
                            float(acc_w), st)
    return mean.view(()), correct, dz


def softmax_cross_entropy(logits, labels, *, denom=None, label_smoothing=0.0, acc=None, acc_weight=1.0,
                          ignore_index=None):
    """Return ``(mean_loss, correct_flags)``.

    ``logits`` is ``[..., C]`` with ``labels`` of the same leading shape (or already flat): the
    leading axes are flattened (as views where the layout allows), ``correct`` comes back flat
    ``[N]``.

    ``denom`` defaults to the local batch size; pass the GLOBAL batch size to get
    the MultiWorkerMirrored ``compute_average_loss`` convention.  ``acc`` (fp32 [3] on the
    device): ``acc += [sum of row losses, sum of correct flags, rows] * acc_weight``
    inside the loss kernel (Keras loss / accuracy metric state without per-step syncs).

    Ignored rows: a label outside ``[0, C)`` (-1, C, ...) marks its row as ignored on both
    engines (HIP kernels and the torch fallback): the row's loss, its ``correct`` flag and its
    logits gradient are 0.  ``ignore_index`` adds one label value (inside ``[0, C)`` or not) that
    marks a row as ignored in the same way.  With a numeric ``denom`` (or ``None``) the row still
    counts in ``denom`` (and in ``acc[2]``): the mean is over all rows.  ``denom="valid"`` makes
    it the mean over the rows that are not ignored (``acc[2]`` then adds their number); with no
    such row the loss and every gradient are 0.  ``correct`` follows the smallest-index rule on
    tied maxima.
    """
    C = logits.shape[-1]
    if logits.dim() != 2:
        logits = logits.reshape(-1, C)
    B = logits.shape[0]
    labels = labels.reshape(-1).long()
    if labels.shape[0] != B:
        raise ValueError(f"labels with {labels.shape[0]} elements for {B} rows of logits")
    if isinstance(denom, str) and denom != "valid":
        raise ValueError(f"denom must be a number, None or 'valid', not {denom!r}")
    denom = B if denom is None else denom
    if ignore_index is not None:
        labels = torch.where(labels == int(ignore_index), torch.full_like(labels, -1), labels)
    if logits.dtype in (torch.bfloat16, torch.float32) and _ext.use_native(logits, labels):
        return _XentFn.apply(logits, labels, denom, label_smoothing, acc, acc_weight)
    lf = logits.float()
    valid = (labels >= 0) & (labels < C)
    safe = torch.where(valid, labels, torch.zeros_like(labels))
    per = F.cross_entropy(lf, safe, reduction="none", label_smoothing=label_smoothing) * valid.to(lf.dtype)
    # first index of the row maximum (the kernels' tie rule), not argmax's unspecified one
    cols = torch.arange(C, device=lf.device).expand_as(lf)
    first = torch.where(lf == lf.max(-1, keepdim=True).values, cols, cols.new_full((), C)).min(-1).values
    correct = ((first == labels) & valid).float()
    by_valid = isinstance(denom, str)
    rows = valid.sum().to(lf.dtype) if by_valid else per.new_tensor(float(B))
    if acc is not None:
        with torch.no_grad():
            acc += torch.stack([per.sum(), correct.sum(), rows]).to(acc.device) * float(acc_weight)
    return per.sum() / (rows.clamp_min(1.0) if by_valid else float(denom)), correct
