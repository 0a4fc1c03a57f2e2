"""Reference tests for the depthwise-convolution kernels (csrc/kernels/dwconv.hip), their raw
launchers (ops/raw.py dwconv_*) and ``ops.depthwise_conv2d`` through autograd.

Every reference is computed in float64 on the host from the same bf16 operands the kernels read
(a tap-by-tap shifted sum: no ``groups=``, no library convolution); inputs come from a host
``torch.Generator``.  Metrics and bounds are those of test_resnet_kernel_edges_gpu.py: forward
outputs and input gradients per pixel row over the channel vector against max(row norm, median
row norm) < 1e-2, weight gradients per filter tap over the channel vector < 2e-3 into fp32 and
< 2e-2 delivered into a bf16 gradient, the bias gradient in relative norm < 1e-2.  Rows / taps
whose true value is structurally zero must be exactly zero.

Which shape reaches which branch (VW = 8: 16-byte channel vectors, DM = 1, Cin % 8 == 0, aligned
bases; VW = 1: one channel per lane):

    forward / dgrad VW = 8          every DM = 1 row with Cin in {8, 16, 24, 40, 264, 256, 528}
    forward / dgrad VW = 1          Cin = 3, 12 (12 % 8 != 0), 5, 65; DM = 2, 3; every odd-offset run
    forward strip tail (OW % 4)     OW = 1, 2, 3, 5, 7, 13, 29 ...; a whole strip at 8x8 / 2
    forward halo predicates         1x1 and 2x2 images under a 3x3 filter, 7x7 / 2 on 10x10
    dgrad inexact divisions         every stride > 1 row; unread input pixels at 9x9, 3x3 / 4 "valid"
                                    (the 9x9, 3x3 / 3 row of the issue reads every pixel)
    grid-stride second trip         VW = 8: 5x128x104x256 (forward 532,480 strips, dgrad 2.1 M
                                    vectors > 2048 * 256 threads); VW = 1: 8x64x64x65
    wgrad idle pixel rows           Cin = 24 (3 channel vectors: 85 rows of 3, one lane idle)
    wgrad several channel groups    VW = 8: Cin = 528 (66 vectors: 64 + 2); VW = 1: Cin = 65, 264 shifted
    wgrad tap groups                3x3 one group, 5x5 three (9 + 9 + 7), 7x7 six (the last holds 4)
    wgrad chunks                    one (short) chunk at the small shapes; 2x37x29: 34 chunks of 64
                                    pixels, the last with 34; 2x130x129x8: chunk length 66 > 64,
                                    509 chunks, the last with 12

Worst figures observed on an MI355X (each test prints its figures before asserting):

    group                                                     worst observed              bound
    geometry matrix (18 shapes)   y, dx / row                 3.66e-3, 3.43e-3            1e-2
    geometry matrix   dw fp32 / tap, overwritten / added to   4.3e-7 / 4.3e-7             2e-3
    grid-stride second trip   y, dx / row                     2.08e-3, 2.07e-3            1e-2
    bias + activation (autograd)   y, dx / row                3.32e-3, 8.21e-3 (tanh)     1e-2
    bias + activation   dw bf16 / tap; bias gradient          1.38e-2 (tanh, C = 5); 3.5e-3   2e-2; 1e-2
    sentinel-guarded buffers, both offsets   y, dx; dw fp32   2.04e-3, 2.88e-3; 4.9e-8    as above
    autograd delivery   dw into a bf16 sink / fresh bf16      2.01e-3 / 2.08e-3           2e-2
    Keras layers (test_keras_separable_gpu.py)   y, dx / row  2.68e-3, 3.78e-3            1e-2
    Keras layers   depthwise / pointwise kernel, bias         2.67e-3 / 2.47e-3, 0        2e-2, 1e-2
"""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16

ROW_BOUND = 1e-2   # bf16 outputs per pixel row
WG32_BOUND = 2e-3  # weight gradient into fp32, per tap
WGBF_BOUND = 2e-2  # weight gradient delivered into a bf16 gradient, per tap
BIAS_BOUND = 1e-2  # bias gradient, relative norm


def _say(*a):
    print("[dwconv]", *a, flush=True)


# ------------------------------------------------------------------------------- metrics


def _row_err(got, ref):
    """Per pixel row over the channel vector: ||got - ref|| / max(||ref||, median row ||ref||),
    maximum over rows.  Rows whose true value is exactly zero must be exactly zero and are left
    out of the median.  Returns (worst, number of zero rows)."""
    C = ref.shape[-1]
    g = got.detach().double().cpu().reshape(-1, C)
    r = ref.reshape(-1, C)
    assert g.shape == r.shape, (g.shape, r.shape)
    assert torch.isfinite(g).all(), "unwritten or non-finite output rows"
    n = r.norm(dim=-1)
    zero = n == 0
    assert (g[zero] == 0).all(), "rows whose true value is zero must be exactly zero"
    live = ~zero
    assert live.any()
    med = n[live].median()
    e = (g[live] - r[live]).norm(dim=-1) / torch.maximum(n[live], med)
    return e.max().item(), int(zero.sum())


def _tap_err(got, ref, base=None):
    """Per filter tap (ky, kx) over the Cout vector of dw [KH, KW, Cin, DM]: ||got - base - ref||
    / ||ref||, maximum over taps.  A tap whose true gradient is exactly zero must hold ``base``
    (0 without one) exactly."""
    KH, KW = ref.shape[:2]
    g = got.detach().double().cpu().reshape(KH, KW, -1)
    r = ref.reshape(KH, KW, -1)
    b = torch.zeros_like(r) if base is None else base.detach().double().cpu().reshape(KH, KW, -1)
    assert torch.isfinite(g).all(), "unwritten or non-finite weight gradient"
    n = r.norm(dim=-1)
    zero = n == 0
    assert torch.equal(g[zero], b[zero]), "structurally zero taps must stay exact"
    live = ~zero
    assert live.any()
    return ((g - b - r)[live].norm(dim=-1) / n[live]).max().item(), int(zero.sum())


# ----------------------------------------------------------------------------- geometry


def _geom(H, W, KH, KW, sh, sw, padding):
    """((pad_top, pad_left), (OH, OW)) of TF's "same" / "valid"."""
    if padding == "same":
        OH, OW = math.ceil(H / sh), math.ceil(W / sw)
        pt = max((OH - 1) * sh + KH - H, 0) // 2
        pl = max((OW - 1) * sw + KW - W, 0) // 2
    else:
        OH, OW = (H - KH) // sh + 1, (W - KW) // sw + 1
        pt = pl = 0
    return (pt, pl), (OH, OW)


def _reference(x, w, dy, stride, pads, out_hw):
    """float64 y, dx, dw of the depthwise convolution as a tap-by-tap shifted sum: x [N,H,W,C],
    w [KH,KW,C,DM], dy [N,OH,OW,C*DM] (all float64); rows / columns past any edge read as zero."""
    N, H, W, C = x.shape
    KH, KW, _, DM = w.shape
    (sh, sw), (pt, pl), (OH, OW) = stride, pads, out_hw
    Hp, Wp = max((OH - 1) * sh + KH, pt + H), max((OW - 1) * sw + KW, pl + W)
    xp = torch.zeros(N, Hp, Wp, C, dtype=torch.float64)
    xp[:, pt:pt + H, pl:pl + W] = x
    xr = xp.repeat_interleave(DM, dim=3)  # channel o = c * DM + m reads input channel c
    y = torch.zeros(N, OH, OW, C * DM, dtype=torch.float64)
    dxp = torch.zeros_like(xr)
    dw = torch.zeros(KH, KW, C * DM, dtype=torch.float64)
    for ky in range(KH):
        for kx in range(KW):
            sl = (slice(None), slice(ky, ky + (OH - 1) * sh + 1, sh), slice(kx, kx + (OW - 1) * sw + 1, sw))
            wv = w[ky, kx].reshape(-1)
            y += xr[sl] * wv
            dw[ky, kx] = (xr[sl] * dy).sum((0, 1, 2))
            dxp[sl] += dy * wv
    dx = dxp[:, pt:pt + H, pl:pl + W].reshape(N, H, W, C, DM).sum(-1)
    return y, dx, dw.reshape(KH, KW, C, DM)


#          name            N   H   W  Cin  KH KW  sh sw  padding  DM
MATRIX = [("one-pixel",    1,  1,  1,   8, 3, 3, 1, 1, "same",  1),
          ("2x2",          1,  2,  2,   8, 3, 3, 1, 1, "same",  1),
          ("c3",           2,  7,  5,   3, 3, 3, 1, 1, "same",  1),
          ("c12-valid",    2,  7,  5,  12, 3, 3, 1, 1, "valid", 1),
          ("8x8-s2",       2,  8,  8,  16, 3, 3, 2, 2, "same",  1),
          ("9x6-s2",       3,  9,  6,  40, 3, 3, 2, 2, "same",  1),
          ("5x5",          2, 11, 13,  24, 5, 5, 1, 1, "same",  1),
          ("7x7-s2",       1, 10, 10,  16, 7, 7, 2, 2, "same",  1),
          ("1x3-s12",      2, 11, 13,   8, 1, 3, 1, 2, "valid", 1),
          ("s3-valid",     2,  9,  9,   8, 3, 3, 3, 3, "valid", 1),
          ("dm2",          2,  6,  7,   8, 3, 3, 1, 1, "same",  2),
          ("dm3-c5-s2",    2,  6,  7,   5, 3, 3, 2, 2, "same",  3),
          ("c264",         1,  5,  5, 264, 3, 3, 1, 1, "same",  1),
          ("37x29",        2, 37, 29,  24, 3, 3, 1, 1, "same",  1),
          # added: the smallest shapes that reach the branches the rows above leave out
          ("s4-unread",    2,  9,  9,   8, 3, 3, 4, 4, "valid", 1),
          ("c528",         1,  5,  5, 528, 3, 3, 1, 1, "same",  1),
          ("long-chunks",  2, 130, 129, 8, 3, 3, 1, 1, "same",  1),
          ("stride-loop1", 8, 64, 64,  65, 3, 3, 1, 1, "same",  1)]
SHAPES = {m[0]: m[1:] for m in MATRIX}
# the epilogue tests' shapes: vector kernels (C = 16) and one channel per lane (C = 5)
EXTRA = {"epi16": (2, 6, 7, 16, 3, 3, 1, 1, "same", 1), "epi5": (2, 6, 7, 5, 3, 3, 1, 1, "same", 1)}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Host operands (bf16) and their float64 reference; computed once and shared, never modified."""
    N, H, W, C, KH, KW, sh, sw, padding, DM = {**SHAPES, **EXTRA}[name]
    pads, out_hw = _geom(H, W, KH, KW, sh, sw, padding)
    g = torch.Generator().manual_seed(1000 + list({**SHAPES, **EXTRA}).index(name))
    x = torch.randn(N, H, W, C, generator=g).to(BF16)
    w = (torch.randn(KH, KW, C, DM, generator=g) / math.sqrt(KH * KW)).to(BF16)
    dy = torch.randn(N, out_hw[0], out_hw[1], C * DM, generator=g).to(BF16)
    y, dx, dw = _reference(x.double(), w.double(), dy.double(), (sh, sw), pads, out_hw)
    return dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw, stride=(sh, sw), pads=pads, out_hw=out_hw)


def _run_raw(d, place=lambda t, out=False: t.to(DEV)):
    """forward, dgrad and wgrad (overwrite, then accumulate onto a base) through the raw
    launchers; ``place`` puts a host tensor (or an output of that shape) on the device."""
    from cloud_amd.ops import raw

    x, w, dy = place(d["x"]), place(d["w"]), place(d["dy"])
    y = place(torch.empty(d["y"].shape, dtype=BF16), True)
    dx = place(torch.empty(d["dx"].shape, dtype=BF16), True)
    raw.dwconv_fwd(x, w, d["stride"], d["pads"], d["out_hw"], out=y)
    raw.dwconv_dgrad(dy, w, x.shape, d["stride"], d["pads"], out=dx)
    dw = raw.dwconv_wgrad(dy, x, w.shape, d["stride"], d["pads"], out=place(torch.empty(d["dw"].shape), True))
    base = torch.full(d["dw"].shape, 0.25)
    acc = place(base, True)
    acc.copy_(base)
    raw.dwconv_wgrad(dy, x, w.shape, d["stride"], d["pads"], out=acc, accumulate=True)
    torch.cuda.synchronize()
    return dict(x=x, w=w, dy=dy, y=y, dx=dx, dw=dw, acc=acc, base=base)


def _check(name, d, r):
    e_y, _ = _row_err(r["y"], d["y"])
    e_dx, z_dx = _row_err(r["dx"], d["dx"])
    e_w, z_w = _tap_err(r["dw"], d["dw"])
    e_a, _ = _tap_err(r["acc"], d["dw"], r["base"])
    _say(f"{name}: y/row {e_y:.3e} dx/row {e_dx:.3e} ({z_dx} zero rows) dw fp32/tap {e_w:.3e} "
         f"({z_w} zero taps) accumulated {e_a:.3e}")
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND, (e_y, e_dx)
    assert e_w < WG32_BOUND and e_a < WG32_BOUND, (e_w, e_a)
    return z_dx, z_w


@pytest.mark.parametrize("name", list(SHAPES))
def test_geometry_matrix_vs_fp64(name):
    d = _case(name)
    z_dx, z_w = _check(name, d, _run_raw(d))
    if name == "s4-unread":  # rows 3, 7, 8 and columns 3, 7, 8 are read by no output
        assert z_dx == 2 * (81 - 36)
    if name == "one-pixel":  # only the centre tap ever meets the image
        assert z_w == 8


def test_grid_stride_second_trip_vec8():
    """5x128x104x256: more strips (forward) and pixel vectors (dgrad) than the capped grid has
    threads, so the last image is computed in the second trip of the grid-stride loops.  The
    first and the last image are compared (the convolution is independent per image)."""
    from cloud_amd.ops import raw

    N, H, W, C = 5, 128, 104, 256
    g = torch.Generator().manual_seed(77)
    x = torch.randn(N, H, W, C, generator=g).to(BF16)
    w = (torch.randn(3, 3, C, 1, generator=g) / 3).to(BF16)
    dy = torch.randn(N, H, W, C, generator=g).to(BF16)
    assert N * H * (W // 4) * (C // 8) > 2048 * 256
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    y = raw.dwconv_fwd(xd, wd, (1, 1), (1, 1), (H, W))
    dx = raw.dwconv_dgrad(dyd, wd, x.shape, (1, 1), (1, 1))
    for n in (0, N - 1):
        ry, rdx, _ = _reference(x[n:n + 1].double(), w.double(), dy[n:n + 1].double(), (1, 1), (1, 1), (H, W))
        e_y, _ = _row_err(y[n:n + 1], ry)
        e_dx, _ = _row_err(dx[n:n + 1], rdx)
        _say(f"grid-stride image {n}: y/row {e_y:.3e} dx/row {e_dx:.3e}")
        assert e_y < ROW_BOUND and e_dx < ROW_BOUND


# ------------------------------------------------------------------------------- epilogue


@pytest.mark.parametrize("act", [None, "relu", "elu", "tanh", "gelu"])
@pytest.mark.parametrize("C", [16, 5])
def test_bias_and_activation_forward_backward(act, C):
    """y = act(dwconv + bias) and its backward through ops.depthwise_conv2d against the float64
    composition, at 2x6x7 with C = 16 (vector kernels, 8-wide elementwise passes) and C = 5 (one
    channel per lane; the activation gradient and the bias column sum take their padded forms)."""
    from cloud_amd import ops

    d = _case("epi%d" % C)
    g = torch.Generator().manual_seed(5)
    bias = torch.randn(C, generator=g)
    x = d["x"].to(DEV).requires_grad_()
    w = d["w"].to(DEV).requires_grad_()
    b = bias.to(DEV).requires_grad_()
    y = ops.depthwise_conv2d(x, w, b, 1, ((1, 1), (1, 1)), act)
    assert y.dtype == BF16
    y.backward(d["dy"].to(DEV))
    torch.cuda.synchronize()
    # float64 composition from the same operands
    x64 = d["x"].double().requires_grad_()
    w64 = d["w"].double().requires_grad_()
    b64 = bias.double().requires_grad_()
    pre = _DwRef.apply(x64, w64, d["stride"], d["pads"], d["out_hw"]) + b64
    ref = {None: lambda t: t, "relu": torch.relu, "elu": torch.nn.functional.elu, "tanh": torch.tanh,
           "gelu": torch.nn.functional.gelu}[act](pre)
    ref.backward(d["dy"].double())
    e_y, _ = _row_err(y, ref.detach())
    e_dx, _ = _row_err(x.grad, x64.grad)
    e_w, _ = _tap_err(w.grad, w64.grad)
    e_b = ((b.grad.double().cpu() - b64.grad).norm() / b64.grad.norm()).item()
    _say(f"epilogue {act} C={C}: y/row {e_y:.3e} dx/row {e_dx:.3e} dw bf16/tap {e_w:.3e} db {e_b:.3e}")
    assert w.grad.dtype == BF16 and b.grad.dtype == torch.float32
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND and e_w < WGBF_BOUND and e_b < BIAS_BOUND


class _DwRef(torch.autograd.Function):
    """The float64 shifted-sum reference as an autograd node (for the epilogue composition)."""

    @staticmethod
    def forward(ctx, x, w, stride, pads, out_hw):
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, pads, out_hw)
        return _reference(x, w, torch.zeros(x.shape[0], *out_hw, w.shape[2] * w.shape[3], dtype=torch.float64),
                          stride, pads, out_hw)[0]

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        _, dx, dw = _reference(x, w, dy, *ctx.cfg)
        return dx, dw, None, None, None


# -------------------------------------------------------------------- bounds of the buffers

GUARD = 64  # elements on either side of every tensor


class _Guarded:
    """Places tensors as interior views of larger buffers filled with a sentinel, ``shift``
    elements past a 128-byte boundary, and checks afterwards that only the views changed."""

    def __init__(self, shift):
        self.shift, self.items = shift, []

    def __call__(self, t, out=False):
        sentinel = 7.0 if t.dtype == BF16 else -3.0
        buf = torch.full((t.numel() + 2 * GUARD,), sentinel, dtype=t.dtype, device=DEV)
        lo = GUARD // 2 + self.shift
        v = buf[lo:lo + t.numel()].view(t.shape)
        if not out:
            v.copy_(t)
        self.items.append((buf, lo, t.numel(), buf.clone() if not out else None, sentinel))
        return v

    def check(self):
        for buf, lo, n, before, sentinel in self.items:
            if before is not None:  # an input: nothing at all may change
                assert torch.equal(buf, before), "an input buffer was written"
            else:
                assert (buf[:lo] == sentinel).all() and (buf[lo + n:] == sentinel).all(), "write outside a tensor"


@pytest.mark.parametrize("name", ["9x6-s2", "c264", "dm3-c5-s2"])
def test_no_access_outside_the_tensors(name):
    """x, w, dy, y, dx and the weight-gradient outputs as interior views of sentinel-filled
    buffers: the sentinels survive, at a 16-byte-aligned base (vector kernels where the shape
    allows) and with every base shifted by one element (2-byte-aligned bf16: the scalar
    kernels), and both runs meet the bounds."""
    d = _case(name)
    for shift in (0, 1):
        place = _Guarded(shift)
        r = _run_raw(d, place)
        assert r["x"].data_ptr() % 16 == 2 * shift
        place.check()
        _check(f"guarded {name} shift {shift}", d, r)


# ------------------------------------------------------------------------------ determinism


def test_weight_gradient_is_bitwise_reproducible():
    from cloud_amd.ops import raw

    d = _case("37x29")
    x, dy = d["x"].to(DEV), d["dy"].to(DEV)
    a = raw.dwconv_wgrad(dy, x, d["w"].shape, d["stride"], d["pads"])
    junk = torch.randn(1 << 20, device=DEV)  # moves the allocator's next workspace
    b = raw.dwconv_wgrad(dy, x, d["w"].shape, d["stride"], d["pads"])
    torch.cuda.synchronize()
    del junk
    assert torch.equal(a, b)


# --------------------------------------------------------------------------------- autograd


@pytest.mark.parametrize("sink", ["arena", "none"])
def test_autograd_weight_gradient_delivery(sink):
    """ops.depthwise_conv2d through backward() with a leaf bf16 weight: an arena-style .grad sink
    is accumulated into (not overwritten, and autograd hands the weight no gradient of its own);
    without one the weight gets a fresh bf16 gradient."""
    from cloud_amd import ops

    d = _case("9x6-s2")
    x = d["x"].to(DEV).requires_grad_()
    w = d["w"].to(DEV).requires_grad_()
    base = None
    if sink != "none":
        g = torch.Generator().manual_seed(9)
        base = (0.5 * torch.randn(d["w"].shape, generator=g)).to(BF16)
        w.grad = base.to(DEV).clone()
        w._ca_arena = True
        held = w.grad
    (pt, pl), (OH, OW) = d["pads"], d["out_hw"]
    y = ops.depthwise_conv2d(x, w, None, d["stride"], ((pt, 0), (pl, 0)), None, out_hw=(OH, OW))
    y.backward(d["dy"].to(DEV))
    torch.cuda.synchronize()
    e_y, _ = _row_err(y, d["y"])
    e_dx, _ = _row_err(x.grad, d["dx"])
    e_w, _ = _tap_err(w.grad, d["dw"], base)
    _say(f"autograd sink={sink}: y/row {e_y:.3e} dx/row {e_dx:.3e} dw/tap {e_w:.3e}")
    if sink != "none":
        assert w.grad is held, "the arena gradient tensor must be written in place"
    assert w.grad.dtype == BF16
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND and e_w < WGBF_BOUND
