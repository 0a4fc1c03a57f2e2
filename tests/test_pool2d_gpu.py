"""Reference tests for the any-window pooling kernels (csrc/kernels/pool2d.hip), their raw
launchers (ops/raw.py pool2d_*) and ``ops.max_pool2d_nhwc`` / ``ops.avg_pool2d_nhwc`` through
autograd.

Every reference is computed in float64 on the host from the same bf16 operands the kernels read:
a plain loop over the window's taps (shifted strided slices of a padded copy, a validity map for
the taps outside the image; no library pooling).  Inputs come from a host ``torch.Generator``:
post-ReLU activations (about half exact zeros) with planted ties at 1.5, channel 0 all zero,
channel 1 all negative with ties at -0.5.

Bounds:

    max y      bitwise equal to the reference
    max idx    the reference's first row-major in-image tap that attains the maximum
    max dx     exactly 0 where the reference is 0; elsewhere |dx - ref| / (2^-8 |ref| + 1e-6) <= 1
    avg y, dx  elementwise |got - ref| <= 2^-8 |ref| + 2^-16 A, A the mean of |x| over the window's
               in-image taps (for dx: the sum of |dy| / count over the covering windows): one bf16
               rounding to nearest is <= 2^-9 relative, doubled for margin; fp32 accumulation of
               <= 255 terms is <= 255 * 2^-24 < 2^-16 of the absolute sum.  Pixels that no window
               reads are exactly 0.

Which shape reaches which branch (VW = 8: 16-byte channel vectors, C % 8 == 0 and aligned bases;
VW = 1: one channel per lane):

    rect-valid      2x7x10x24   2x3 / 2x3 valid     rectangular window, VW = 8, C / 8 = 3
    same-h-sym      2x7x9x24    3x2 / 1x2 same      pads 1 | 1 in H, 0 | 1 in W
    same-5x4        1x5x4x8     3x3 / 2x2 same      pads 1 | 1 in H, 0 | 1 in W
    s4-unread       2x9x9x5     3x3 / 4x4 valid     stride > window: rows / columns 3, 7, 8 unread,
                                                    dx exactly 0 there; VW = 1
    one-pixel       1x1x1x3     3x3 / 1x1 same      one pixel, eight padded taps, divisor 1
    c12             1x2x2x12    2x2 / 1x1 same      12 % 8 != 0: VW = 1
    subsample       3x6x5x16    1x1 / 2x2 valid     pure subsampling (ops: the max pool is today's
                                                    square form and takes pool.hip; raw: pool2d.hip)
    225-taps        1x15x15x8   15x15 / 15x15 valid the argmax byte nearly full (ops: as above)
    5x7             2x13x29x40  5x7 / 3x2 same      large rectangular window, overlapping
    1d-view         1x1x64x8    1x4 / 1x4 valid     the 1D layers' view
    explicit        2x8x8x16    3x3 / 2x2           pads ((0, 1), (0, 1)) with out_hw = (4, 4)
    shifted bases   2x7x9x16    3x2 / 1x2 same      every tensor one element into its buffer: VW = 1
    second trip     VW = 8: 4x96x96x128, 3x2 / 1 same: 589,824 vectors in x and in y, more than the
                    2048 * 256 = 524,288 threads of the capped grid in all four passes;
                    VW = 1: 2x64x64x65, same window: 532,480 elements in x and in y

Each test prints its worst figure before asserting.  Worst figures observed on an MI355X:

    max y, idx (all cases)            bitwise equal, equal
    max dx                            0.000 - 0.996 of 1 ulp; zeros exact
    avg y                             0.992 of the bound (trip8 / trip1), 0.985 on the matrix
    avg dx                            0.992 of the bound (same-h-sym, trip8 / trip1)

The average figures sit close to 1 because a bf16 value carries 8 significant bits: rounding to
nearest is off by up to 2^-8 of a value just above a power of two (2^-9 just below the next), so
the 2^-8 |ref| term is the rounding itself and the 2^-16 A term is what is left for the fp32
arithmetic, which needs about 2^-22 |ref|.  The bound cannot be missed by a correctly rounded result.
"""
import contextlib
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16


def _say(*a):
    print("[pool2d]", *a, flush=True)


# ----------------------------------------------------------------------------- reference


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


def _reference(x, dy, k, s, pads, out_hw):
    """float64 max / average pooling of x [N, H, W, C] and their input gradients for dy
    [N, OH, OW, C], tap by tap.  Returns a dict: max_y, max_idx (first row-major in-image tap
    that attains the maximum), max_dx, avg_y, avg_dx, the bound scales avg_A / avg_dA, and
    ``read`` (how many windows read each pixel)."""
    N, H, W, C = x.shape
    (KH, KW), (sh, sw), (pt, pl), (OH, OW) = k, s, pads, out_hw
    Hp, Wp = max((OH - 1) * sh + KH, pt + H), max((OW - 1) * sw + KW, pl + W)
    xp = torch.zeros(N, Hp, Wp, C, dtype=torch.float64)
    xp[:, pt:pt + H, pl:pl + W] = x
    inside = torch.zeros(1, Hp, Wp, 1, dtype=torch.bool)
    inside[:, pt:pt + H, pl:pl + W] = True

    def window(kh, kw):
        return (slice(None), slice(kh, kh + (OH - 1) * sh + 1, sh), slice(kw, kw + (OW - 1) * sw + 1, sw))

    best = torch.full((N, OH, OW, C), float("-inf"), dtype=torch.float64)
    arg = torch.full((N, OH, OW, C), -1, dtype=torch.long)
    total = torch.zeros(N, OH, OW, C, dtype=torch.float64)
    absum = torch.zeros(N, OH, OW, C, dtype=torch.float64)
    count = torch.zeros(1, OH, OW, 1, dtype=torch.float64)
    for kh in range(KH):
        for kw in range(KW):
            v, ok = xp[window(kh, kw)], inside[window(kh, kw)]
            win = ok & (v > best)  # strict: the first tap that attains the maximum stays
            best = torch.where(win, v, best)
            arg = torch.where(win, torch.full_like(arg, kh * KW + kw), arg)
            total += torch.where(ok, v, torch.zeros_like(v))
            absum += torch.where(ok, v.abs(), torch.zeros_like(v))
            count += ok
    assert (count > 0).all() and (arg >= 0).all()
    dmax, davg, dA = torch.zeros_like(xp), torch.zeros_like(xp), torch.zeros_like(xp)
    read = torch.zeros(1, Hp, Wp, 1, dtype=torch.float64)
    for kh in range(KH):
        for kw in range(KW):
            sl = window(kh, kw)
            ok = inside[sl].double()
            dmax[sl] += dy * (arg == kh * KW + kw)
            davg[sl] += dy / count * ok
            dA[sl] += dy.abs() / count * ok
            read[sl] += ok

    def crop(t):
        return t[:, pt:pt + H, pl:pl + W].contiguous()

    return dict(max_y=best, max_idx=arg, max_dx=crop(dmax), avg_y=total / count, avg_A=absum / count,
                avg_dx=crop(davg), avg_dA=crop(dA), read=crop(read).expand(N, H, W, C))


def _pool_input(N, H, W, C, g):
    x = torch.relu(torch.randn(N, H, W, C, generator=g))
    x[torch.rand(N, H, W, C, generator=g) < 0.15] = 1.5
    x[..., 0] = 0.0
    if C > 1:
        neg = -(torch.randn(N, H, W, generator=g).abs() + 0.125)
        neg[torch.rand(N, H, W, generator=g) < 0.3] = -0.5
        x[..., 1] = neg
    return x.to(BF16)


#          name          N   H   W   C  KH  KW sh  sw  padding
MATRIX = [("rect-valid", 2,  7, 10, 24,  2,  3, 2,  3, "valid"),
          ("same-h-sym", 2,  7,  9, 24,  3,  2, 1,  2, "same"),
          ("same-5x4",   1,  5,  4,  8,  3,  3, 2,  2, "same"),
          ("s4-unread",  2,  9,  9,  5,  3,  3, 4,  4, "valid"),
          ("one-pixel",  1,  1,  1,  3,  3,  3, 1,  1, "same"),
          ("c12",        1,  2,  2, 12,  2,  2, 1,  1, "same"),
          ("subsample",  3,  6,  5, 16,  1,  1, 2,  2, "valid"),
          ("225-taps",   1, 15, 15,  8, 15, 15, 15, 15, "valid"),
          ("5x7",        2, 13, 29, 40,  5,  7, 3,  2, "same"),
          ("1d-view",    1,  1, 64,  8,  1,  4, 1,  4, "valid"),
          ("explicit",   2,  8,  8, 16,  3,  3, 2,  2, ((0, 1), (0, 1), (4, 4)))]
SHAPES = {m[0]: m[1:] for m in MATRIX}
EXTRA = {"shifted": (2, 7, 9, 16, 3, 2, 1, 2, "same"),
         "trip8": (4, 96, 96, 128, 3, 2, 1, 1, "same"), "trip1": (2, 64, 64, 65, 3, 2, 1, 1, "same")}


@functools.lru_cache(maxsize=None)
def _case(name, images=None):
    """Host operands (bf16) and their float64 reference; computed once and shared, never modified.
    ``images``: the reference covers these images only (pooling is independent per image)."""
    table = {**SHAPES, **EXTRA}
    N, H, W, C, KH, KW, sh, sw, padding = table[name]
    if isinstance(padding, str):
        pads, out_hw = _geom(H, W, KH, KW, sh, sw, padding)
        op_pad, op_out = 0, None  # what the ops are given
        if padding == "same":
            tot = (max((out_hw[0] - 1) * sh + KH - H, 0), max((out_hw[1] - 1) * sw + KW - W, 0))
            op_pad, op_out = ((pads[0], tot[0] - pads[0]), (pads[1], tot[1] - pads[1])), out_hw
    else:
        op_pad, op_out = (padding[0], padding[1]), padding[2]
        pads, out_hw = (padding[0][0], padding[1][0]), padding[2]
    g = torch.Generator().manual_seed(2000 + list(table).index(name))
    x = _pool_input(N, H, W, C, g)
    dy = torch.randn(N, out_hw[0], out_hw[1], C, generator=g).to(BF16)
    sel = list(range(N)) if images is None else list(images)
    ref = _reference(x[sel].double(), dy[sel].double(), (KH, KW), (sh, sw), pads, out_hw)
    return dict(x=x, dy=dy, k=(KH, KW), s=(sh, sw), pads=pads, out_hw=out_hw, op_pad=op_pad, op_out=op_out, ref=ref,
                sel=sel)


# --------------------------------------------------------------------------------- checks


def _host(t, d):
    return t.detach()[d["sel"]].cpu()


def _check_max(tag, d, y, idx, dx):
    r = d["ref"]
    y, idx, dx = _host(y, d).double(), _host(idx, d).long(), _host(dx, d).double()
    same_y, same_idx = torch.equal(y, r["max_y"]), torch.equal(idx, r["max_idx"])
    zero_ok = bool((dx[r["max_dx"] == 0] == 0).all())
    ulps = ((dx - r["max_dx"]).abs() / (2.0 ** -8 * r["max_dx"].abs() + 1e-6)).max().item()
    unread = int((r["read"] == 0).sum())
    _say(f"{tag} max: y bitwise {same_y}, idx equal {same_idx}, dx {ulps:.3f} ulp, zeros exact {zero_ok}, "
         f"{unread} unread elements")
    assert same_y, "pooled values must be bitwise equal"
    assert same_idx, "argmax: the first row-major in-image tap that attains the maximum"
    assert zero_ok, "dx must be exactly 0 where the reference is"
    assert ulps <= 1.0, ulps


def _check_avg(tag, d, y, dx):
    r = d["ref"]
    y, dx = _host(y, d).double(), _host(dx, d).double()
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    e_y = ((y - r["avg_y"]).abs() / (2.0 ** -8 * r["avg_y"].abs() + 2.0 ** -16 * r["avg_A"] + 1e-300)).max().item()
    live = r["read"] > 0
    zero_ok = bool((dx[~live] == 0).all())
    e_dx = 0.0
    if live.any():
        bound = 2.0 ** -8 * r["avg_dx"].abs() + 2.0 ** -16 * r["avg_dA"] + 1e-300
        e_dx = ((dx - r["avg_dx"]).abs()[live] / bound[live]).max().item()
    _say(f"{tag} avg: y {e_y:.3f} of the bound, dx {e_dx:.3f} of the bound, unread pixels exact zeros {zero_ok}")
    assert zero_ok, "pixels that no window reads must be exactly 0"
    assert e_y <= 1.0 and e_dx <= 1.0, (e_y, e_dx)


def _run_raw(d, place=lambda t, out=False: t.to(DEV)):
    """The four passes through the raw launchers; ``place`` puts a host tensor (or an output of that
    shape) on the device."""
    from cloud_amd.ops import raw

    x, dy = place(d["x"]), place(d["dy"])
    k, s, pads, out_hw = d["k"], d["s"], d["pads"], d["out_hw"]
    y = place(torch.empty(d["dy"].shape, dtype=BF16), True)
    idx = place(torch.empty(d["dy"].shape, dtype=torch.uint8), True)
    dx = place(torch.empty(d["x"].shape, dtype=BF16), True)
    ya = place(torch.empty(d["dy"].shape, dtype=BF16), True)
    dxa = place(torch.empty(d["x"].shape, dtype=BF16), True)
    raw.pool2d_max_fwd(x, k, s, pads, out_hw, out=y, idx=idx)
    raw.pool2d_max_bwd(dy, idx, x.shape, k, s, pads, out=dx)
    raw.pool2d_avg_fwd(x, k, s, pads, out_hw, out=ya)
    raw.pool2d_avg_bwd(dy, x.shape, k, s, pads, out=dxa)
    torch.cuda.synchronize()
    return dict(x=x, y=y, idx=idx, dx=dx, ya=ya, dxa=dxa)


@pytest.mark.parametrize("name", list(SHAPES))
def test_geometry_matrix_raw_launchers(name):
    """Every row on pool2d.hip through ops.raw.pool2d_* (VW as the table in the module docstring)."""
    d = _case(name)
    r = _run_raw(d)
    _check_max(f"raw {name}", d, r["y"], r["idx"], r["dx"])
    _check_avg(f"raw {name}", d, r["ya"], r["dxa"])
    if name == "s4-unread":  # rows 3, 7, 8 and columns 3, 7, 8 are read by no window
        assert int((d["ref"]["read"] == 0).sum()) == 2 * (81 - 36) * 5
    if name == "one-pixel":  # eight padded taps: divisor 1, argmax the centre tap
        assert torch.equal(r["ya"].cpu(), d["x"]) and (r["idx"] == 4).all()


@pytest.mark.parametrize("name", list(SHAPES))
def test_geometry_matrix_through_autograd(name):
    """ops.max_pool2d_nhwc / ops.avg_pool2d_nhwc forward and backward, with the arguments the Keras
    layers pass ("same" as its pad split plus out_hw)."""
    from cloud_amd import ops

    d = _case(name)
    for kind, op in (("max", ops.max_pool2d_nhwc), ("avg", ops.avg_pool2d_nhwc)):
        x = d["x"].to(DEV).requires_grad_()
        y = op(x, d["k"], d["s"], d["op_pad"], out_hw=d["op_out"])
        assert y.dtype == BF16 and y.grad_fn is not None and "Pool" in type(y.grad_fn).__name__, type(y.grad_fn)
        saved = y.grad_fn.saved_tensors
        y.backward(d["dy"].to(DEV))
        torch.cuda.synchronize()
        if kind == "max":
            _check_max(f"autograd {name}", d, y, saved[0], x.grad)
        else:
            assert saved == ()  # nothing is kept for the backward
            _check_avg(f"autograd {name}", d, y, x.grad)


# -------------------------------------------------------------------- bounds of the buffers

GUARD = 64  # elements on either side of every tensor


class _Guarded:
    """Places tensors as interior views of larger buffers filled with a sentinel, ``shift``
    elements past a 128-byte boundary, and checks afterwards that only the views changed."""

    def __init__(self, shift):
        self.shift, self.items = shift, []

    def __call__(self, t, out=False):
        sentinel = 7.0 if t.dtype == BF16 else 201
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


@pytest.mark.parametrize("shift", [1, 0])
def test_unaligned_bases_and_no_access_outside_the_tensors(shift):
    """C = 16 with x, dy, y, idx and dx as views that start one element (2 bytes; 1 byte for idx)
    into sentinel-filled buffers: the launchers must take VW = 1 (a 16-byte vector access there
    would be misaligned), the results meet the bounds and the sentinels on both sides survive.
    shift 0 is the same placement at aligned bases (VW = 8)."""
    d = _case("shifted")
    place = _Guarded(shift)
    r = _run_raw(d, place)
    assert r["x"].data_ptr() % 16 == 2 * shift and r["y"].data_ptr() % 16 == 2 * shift
    place.check()
    _check_max(f"guarded shift {shift}", d, r["y"], r["idx"], r["dx"])
    _check_avg(f"guarded shift {shift}", d, r["ya"], r["dxa"])


# ------------------------------------------------------------------------------ grid stride


@pytest.mark.parametrize("name", ["trip8", "trip1"])
def test_grid_stride_second_trip(name):
    """More work items than the capped grid has threads (2048 * 256 = 524,288) in all four passes:
    trip8 4x96x96x128 -> 589,824 channel vectors in x and in y (stride 1, "same"); trip1 2x64x64x65
    -> 532,480 elements.  The last image, computed (in part) in the second trip, and the first are
    compared."""
    N = EXTRA[name][0]
    d = _case(name, images=(0, N - 1))
    vw = 8 if name == "trip8" else 1
    assert d["x"].numel() // vw > 2048 * 256 and d["dy"].numel() // vw > 2048 * 256
    r = _run_raw(d)
    _check_max(name, d, r["y"], r["idx"], r["dx"])
    _check_avg(name, d, r["ya"], r["dxa"])


# --------------------------------------------------------------------------------- refusals


def _refused():
    """(x shape, dtype, kernel, stride, (top, left), out_hw, what)"""
    return [((1, 16, 16, 5), BF16, (16, 16), (16, 16), (0, 0), (1, 1), "KH * KW = 256"),
            ((1, 6, 6, 5), BF16, (3, 3), (1, 1), (3, 0), (7, 4), "pad_top = KH"),
            ((1, 4, 4, 5), BF16, (2, 2), (2, 2), (0, 0), (4, 2), "the last window lies below the image"),
            ((1, 4, 4, 5), torch.float32, (2, 2), (2, 2), (0, 0), (2, 2), "a non-bf16 tensor")]


@pytest.mark.parametrize("case", _refused(), ids=lambda c: c[-1])
def test_raw_launchers_refuse_before_writing(case):
    from cloud_amd.ops import _ext, raw

    shape, dtype, k, s, pads, out_hw, what = case
    x = torch.ones(shape, dtype=dtype, device=DEV)
    oshape = (shape[0], *out_hw, shape[3])
    y = torch.full(oshape, 7.0, dtype=dtype, device=DEV)
    dy = torch.ones(oshape, dtype=dtype, device=DEV)
    idx = torch.full(oshape, 201, dtype=torch.uint8, device=DEV)
    dx = torch.full(shape, 7.0, dtype=dtype, device=DEV)
    with pytest.raises(ValueError):
        raw.pool2d_max_fwd(x, k, s, pads, out_hw, out=y, idx=idx)
    with pytest.raises(ValueError):
        raw.pool2d_avg_fwd(x, k, s, pads, out_hw, out=y)
    with pytest.raises(ValueError):
        raw.pool2d_max_bwd(dy, idx, shape, k, s, pads, out=dx)
    with pytest.raises(ValueError):
        raw.pool2d_avg_bwd(dy, shape, k, s, pads, out=dx)
    if dtype == BF16:  # the launchers' own check, under the Python one
        ext = _ext.load(required=True)
        geo = (*shape, *k, *s, *pads, *out_hw, _ext.stream_handle(x.device))
        for call in (lambda: ext.pool2d_max_fwd(x.data_ptr(), y.data_ptr(), idx.data_ptr(), *geo),
                     lambda: ext.pool2d_avg_fwd(x.data_ptr(), y.data_ptr(), *geo),
                     lambda: ext.pool2d_max_bwd(dy.data_ptr(), idx.data_ptr(), dx.data_ptr(), *geo),
                     lambda: ext.pool2d_avg_bwd(dy.data_ptr(), dx.data_ptr(), *geo)):
            with pytest.raises(RuntimeError, match="invalid arguments"):
                call()
    torch.cuda.synchronize()
    assert (y == 7.0).all() and (dx == 7.0).all() and (idx == 201).all(), "an output was written"
    _say(f"refused: {what}")


@contextlib.contextmanager
def _counted(monkeypatch, owners):
    calls = {}

    def wrap(owner, name, tag):
        orig = getattr(owner, name)

        def f(*a, **k):
            calls[tag] = calls.get(tag, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(owner, name, f)

    for owner, names, prefix in owners:
        for name in names:
            wrap(owner, name, prefix + name)
    yield calls


RAW_NAMES = ("pool2d_max_fwd", "pool2d_max_bwd", "pool2d_avg_fwd", "pool2d_avg_bwd")


@pytest.mark.parametrize("case", _refused(), ids=lambda c: c[-1])
def test_ops_send_refused_inputs_to_the_pytorch_expression(case, monkeypatch):
    """The same inputs through ops.*_pool2d_nhwc: no pool2d launcher is called, PyTorch computes."""
    from cloud_amd import ops
    from cloud_amd.ops import raw

    shape, dtype, k, s, pads, out_hw, what = case
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g).to(dtype).to(DEV)
    with _counted(monkeypatch, [(raw, RAW_NAMES, "raw."), (F, ("max_pool2d", "avg_pool2d"), "F.")]) as calls:
        ym = ops.max_pool2d_nhwc(x, k, s, ((pads[0], 0), (pads[1], 0)), out_hw=out_hw)
        ya = ops.avg_pool2d_nhwc(x, k, s, ((pads[0], 0), (pads[1], 0)), out_hw=out_hw)
        torch.cuda.synchronize()
    assert not any(n.startswith("raw.") for n in calls), calls
    assert calls.get("F.max_pool2d") == 1 and calls.get("F.avg_pool2d") == 2, calls
    assert tuple(ym.shape) == tuple(ya.shape) == (shape[0], *out_hw, shape[3]) and ym.dtype == ya.dtype == dtype
    if what in ("KH * KW = 256", "a non-bf16 tensor"):  # every window holds an in-image tap: values too
        ref = _reference(x.double().cpu(), torch.zeros(shape[0], *out_hw, shape[3], dtype=torch.float64), k, s, pads,
                         out_hw)
        assert torch.equal(ym.double().cpu(), ref["max_y"])
        assert ((ya.double().cpu() - ref["avg_y"]).abs() <= 2.0 ** -8 * ref["avg_y"].abs() + 1e-6).all()


# ---------------------------------------------------------------------------------- routing


def test_todays_square_form_keeps_the_old_kernels(monkeypatch):
    from cloud_amd import ops
    from cloud_amd.ops import _ext, raw

    ext = _ext.load(required=True)
    x = _pool_input(2, 9, 9, 8, torch.Generator().manual_seed(5)).to(DEV).requires_grad_()
    with _counted(monkeypatch, [(ext, ("maxpool_fwd", "maxpool_bwd"), "ext."), (raw, RAW_NAMES, "raw.")]) as calls:
        y = ops.max_pool2d_nhwc(x, 3, 2, 1)
        y.sum().backward()
        y2 = ops.max_pool2d_nhwc(x.detach(), (3, 3), (2, 2), ((1, 1), (1, 1)))  # the same call, spelled as pairs
        torch.cuda.synchronize()
    assert calls == {"ext.maxpool_fwd": 2, "ext.maxpool_bwd": 1}, calls
    assert torch.equal(y, y2)


def test_keras_pool_layers_reach_no_library_pooling(monkeypatch):
    """bf16 CUDA forward + backward of MaxPooling2D(3, 1, "same"), AveragePooling2D(2) and
    MaxPooling1D(2): no F.pad, F.max_pool2d, F.avg_pool2d or Tensor.permute; every pass is a
    pool2d launcher."""
    from cloud_amd.keras import layers
    from cloud_amd.ops import raw

    g = torch.Generator().manual_seed(6)
    x4 = torch.randn(2, 9, 10, 16, generator=g).to(BF16).to(DEV).requires_grad_()
    x3 = torch.randn(2, 11, 16, generator=g).to(BF16).to(DEV).requires_grad_()
    jobs = [(layers.MaxPooling2D(3, 1, "same"), x4, (2, 9, 10, 16)), (layers.AveragePooling2D(2), x4, (2, 4, 5, 16)),
            (layers.MaxPooling1D(2), x3, (2, 5, 16))]
    with _counted(monkeypatch, [(F, ("pad", "max_pool2d", "avg_pool2d"), "F."), (torch.Tensor, ("permute",), "Tensor."),
                                (raw, RAW_NAMES, "raw.")]) as calls:
        for layer, x, shape in jobs:
            y = layer(x)
            assert tuple(y.shape) == shape and y.dtype == BF16
            y.sum().backward()
        torch.cuda.synchronize()
    assert calls == {"raw.pool2d_max_fwd": 2, "raw.pool2d_max_bwd": 2, "raw.pool2d_avg_fwd": 1,
                     "raw.pool2d_avg_bwd": 1}, calls
