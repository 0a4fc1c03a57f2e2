"""Convolution + inference BatchNorm (+ residual) (+ ReLU) in one launch (ext.conv_fwd_bn:
ca_conv_fwd_bn in csrc/kernels/conv.hip, the EPI_BF16_AFF epilogue of csrc/include/ca_mfma_core.h)
against float64.

    y = act(conv(x, w) * scale[c] + shift[c] (+ residual)),   act = ReLU or none

References are float64 on the host, computed from exactly the bf16 operands (and fp32
coefficients) the kernel reads; inputs come from a host ``torch.Generator`` seeded per geometry.
The coefficients are at full scale: scale in [0.5, 1.5] with the sign flipped on a quarter of the
channels, shift ~ 0.75 + 0.5 N(0, 1), residual ~ N(0, 1).  The output is pre-filled with NaN inside
a guarded allocation (test_bn_fold_edges_gpu._Arena): every element must be written, none past the
last row.

Geometries: the smallest that reach each dispatch branch of ca_conv_fwd_bn, with an M tail and an N
tail (CASES below).  Each runs with and without residual, with ReLU and without.

Assertions per case:
  * per-row error <= ROW_BOUND (1e-2, the project's bound for bf16 outputs; metric _row_err of
    test_resnet_kernel_edges_gpu.py);
  * under ReLU no output is negative (nor -0.0), and every element whose float64 pre-activation
    t + r (t = conv * scale + shift, r = residual) lies below -2^-6 (|t| + |r|) is exactly zero:
    the kernel rounds t to bf16, adds r in fp32 and rounds again, two roundings of at most
    2^-8 (|t| + |r|) each, i.e. 2^-7 (|t| + |r|); the factor 2 is the margin;
  * the guard rows keep their bit pattern;
  * the REFERENCE has no all-zero row (so _row_err's zero-row rule never hides a row).

Worst figures observed on an MI355X (each case prints its figures before asserting):

    geometry                 branch                                  worst y / row over the 4 variants
    3x3_9x13                 tap-mask, tall 256 x 64                 3.22e-3
    3x3_13x9_c128            patch-fed core                          2.99e-3
    s2_15x10                 tap-mask 128 x 128, stride 2            2.94e-3
    s2_10x15_c24             general loader, 128 x 64, N tail 8      3.37e-3
    1x1s2_11x7               strided shortcut (tap-mask, 1 tap)      2.73e-3
    rowseg_9x12              row-segment stem loader, tall tile      3.50e-3
    1x1_9x13_c256            dense 1x1, 128 x 128                    2.72e-3
    1x1_7x7_c520             dense 1x1, N = 4 * 128 + 8              2.54e-3
    1x1_9x13_c64             dense 1x1, 64-wide N tile               3.21e-3

(without residual 1.84e-3 .. 2.22e-3; every figure equals a host emulation of the kernel's two
roundings bit for bit; no negative output, no clearly negative pre-activation left non-zero.)
"""
import functools
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bn_fold_edges_gpu as E  # noqa: E402  (guarded allocations)
import test_resnet_kernel_edges_gpu as R  # noqa: E402  (metrics and bounds of the conv edge tests)

_row_err, _say, ROW_BOUND = R._row_err, R._say, R.ROW_BOUND
_Arena = E._Arena
DEV = "cuda"
BF16 = torch.bfloat16

# (N, H, W, Cin, Cout, KH, KW, stride, pad)
CASES = {
    "3x3_9x13": (3, 9, 13, 64, 64, 3, 3, 1, 1),          # tall 256 x 64 tap-mask tile, M = 351
    "3x3_13x9_c128": (3, 13, 9, 128, 192, 3, 3, 1, 1),   # patch-fed core, Cout 128 + 64
    "s2_15x10": (2, 15, 10, 64, 128, 3, 3, 2, 1),        # strided tap-mask, 128 x 128
    "s2_10x15_c24": (2, 10, 15, 24, 40, 3, 3, 2, 1),     # general loader, N tail 8
    "1x1s2_11x7": (3, 11, 7, 128, 256, 1, 1, 2, 0),      # strided shortcut
    "rowseg_9x12": (2, 9, 12, 16, 64, 4, 4, 1, 0),       # row-segment stem loader
    "1x1_9x13_c256": (3, 9, 13, 64, 256, 1, 1, 1, 0),    # dense 1x1 (NT GEMM), M = 351
    "1x1_7x7_c520": (2, 7, 7, 256, 520, 1, 1, 1, 0),     # dense 1x1, N = 4 * 128 + 8
    # beyond the issue's list: the dense GEMM's 64-wide N tile (a bottleneck's conv1, N <= 64)
    "1x1_9x13_c64": (3, 9, 13, 256, 64, 1, 1, 1, 0),
}


def _out_hw(n, k, s, p):
    return (n + 2 * p - k) // s + 1


@functools.lru_cache(maxsize=None)
def _data(name):
    """bf16 operands, fp32 coefficients (host) and the float64 convolution of them; computed once
    per process, shared by the four variants of the geometry, never modified."""
    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    g = torch.Generator().manual_seed(7000 + list(CASES).index(name))
    OH, OW = _out_hw(H, KH, s, p), _out_hw(W, KW, s, p)
    x = torch.randn(N, H, W, Cin, generator=g).to(BF16)
    w = (torch.randn(Cout, KH, KW, Cin, generator=g) / math.sqrt(KH * KW * Cin)).to(BF16)
    scale = 0.5 + torch.rand(Cout, generator=g)
    scale = torch.where(torch.rand(Cout, generator=g) < 0.25, -scale, scale).float().contiguous()
    shift = (0.75 + 0.5 * torch.randn(Cout, generator=g)).float().contiguous()
    res = torch.randn(N, OH, OW, Cout, generator=g).to(BF16)
    z = F.conv2d(x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2), None, s, p).permute(0, 2, 3, 1)
    t = z * scale.double() + shift.double()
    return dict(x=x, w=w, scale=scale, shift=shift, res=res, t=t.contiguous())


def reference(name, with_res, relu):
    """(float64 reference, float64 pre-activation t + r, |t| + |r|)."""
    d = _data(name)
    r = d["res"].double() if with_res else torch.zeros_like(d["t"])
    pre = d["t"] + r
    return (torch.relu(pre) if relu else pre), pre, d["t"].abs() + r.abs()


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "noact"])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("name", list(CASES))
def test_conv_bn_infer_vs_fp64(name, with_res, relu):
    from cloud_amd.ops import raw

    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    d = _data(name)
    ref, pre, mag = reference(name, with_res, relu)
    assert bool((ref.reshape(-1, Cout).norm(dim=-1) > 0).all()), "the reference must have no all-zero row"
    arena = _Arena()
    y = arena.new(ref.shape, BF16, name="y")
    x, w, scale, shift = (d[k].to(DEV) for k in ("x", "w", "scale", "shift"))
    res = d["res"].to(DEV) if with_res else None
    out = raw.conv_fwd_bn(x, w, scale, shift, s, p, residual=res, relu=relu, out=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    got = y.double().cpu()
    e_y, zero_rows = _row_err(y, ref)
    must_zero = pre < -(2.0 ** -6) * mag
    n_neg = int((got < 0).sum()) + int((y.view(torch.int16) == -32768).sum()) if relu else 0
    n_leak = int((got[must_zero] != 0).sum()) if relu else 0
    _say(f"conv_bn_infer {name} {CASES[name]} res={int(with_res)} relu={int(relu)}: y/row {e_y:.3e} "
         f"({zero_rows} zero rows), negative outputs {n_neg}, clearly-negative pre-activations "
         f"{int(must_zero.sum())} of {must_zero.numel()} with {n_leak} not zero")
    assert zero_rows == 0
    assert e_y <= ROW_BOUND, e_y
    if relu:
        assert n_neg == 0, "ReLU output below zero"
        assert n_leak == 0, "pre-activation clearly below zero, output not zero"
    arena.check()


@pytest.mark.gpu
def test_conv_bn_act_infer_op_routes_and_refuses():
    """The public op: native on bf16 CUDA tensors (equal to the raw launcher bit for bit), the torch
    formula otherwise; it refuses to run where a gradient would be expected."""
    from cloud_amd import ops
    from cloud_amd.ops import raw

    name = "s2_15x10"
    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    d = _data(name)
    x, w, scale, shift, res = (d[k].to(DEV) for k in ("x", "w", "scale", "shift", "res"))
    with torch.no_grad():
        a = ops.conv_bn_act_infer(x, w, scale, shift, stride=s, padding=p, residual=res, relu=True)
        b = raw.conv_fwd_bn(x, w, scale, shift, s, p, residual=res, relu=True)
        c = ops.conv_bn_act_infer(x.float(), w.float(), scale, shift, stride=s, padding=p, residual=res.float(),
                                  relu=True)
    assert torch.equal(a, b)
    ref, _, _ = reference(name, True, True)
    assert c.dtype == torch.float32 and _row_err(c, ref)[0] < 1e-4
    with pytest.raises(AssertionError):
        ops.conv_bn_act_infer(x, w, scale, shift, stride=s, padding=p)  # grad mode on
    with torch.no_grad(), pytest.raises(AssertionError):
        ops.conv_bn_act_infer(x, w.clone().requires_grad_(), scale, shift, stride=s, padding=p)
