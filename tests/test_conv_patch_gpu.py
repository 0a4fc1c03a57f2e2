"""Reference tests for the patch-fed 3x3 / stride-1 / pad-1 convolution core (ca_conv_patch.h):
forward (plain and with the BN-forward statistics partials) and input gradient (plain and with
the BN-backward statistics epilogue, random ReLU bitmask).

References are float64 on the host from the same bf16 operands; inputs come from a host
``torch.Generator``.  Metrics and bounds are those of test_resnet_kernel_edges_gpu.py: per
pixel row error <= 1e-2 against max(row norm, median row norm), rows whose true value is zero
exactly zero, statistics partials within 2^-20 * sum |term| per channel.  Every case first
asserts the dispatch predicate (``conv_patch_shape``), so a silent fallback to the tap-gathered
implicit GEMM cannot pass.

Shapes (all 3x3 / s1 / p1), the smallest that reach each way the kernel can go wrong:

    3 x 5 x 7,    64 -> 128   M = 105: one ragged tile spanning three images, H != W
    2 x 9 x 14,  128 -> 128   two channel chunks (patch reloaded); tile 2 starts mid-row of image 1, ragged
    2 x 6 x 28,   64 -> 256   the largest patch, two N tiles, three M tiles
    130 x 1 x 1,  64 -> 128   only the centre tap is ever valid; two tiles
    3 x 7 x 7,   192 -> 128   three chunks, W = 7

Every shape runs in both directions.  The dispatch rule asks for more than 64 output columns,
and an input gradient writes Cin columns: the input gradients of the three 64-input-channel
shapes therefore stay, by that rule, on the tall-tile implicit GEMM (asserted, and still held to
float64).  So that the patch-fed input gradient meets the same geometries, the three are also
run mirrored (Cin and Cout swapped: 64 gathered channels, 128 / 256 output columns) in the
input-gradient tests.

Worst figures observed on an MI355X (each test prints its figures before asserting):

    forward y / row                                    1.98e-3       bound 1e-2
    input gradient dx / row (patch core)               2.11e-3       bound 1e-2
    forward statistics partials, err / bound           0.20          1
    BN-backward statistics partials, err / bound       0.058         1
    NaN-embedded inputs y, dx / row                    1.98e-3, 2.11e-3 (y bitwise that of the plain call)
    patch vs implicit GEMM y, dx, |a - b| / (2^-7 |ref| + 1e-6)   0.56, 0.995   1
"""
import functools
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
NAN = float("nan")

ROW_BOUND = 1e-2         # bf16 outputs per row
PART_BOUND = 2.0 ** -20  # statistics partials: |err| <= 2^-20 * sum |term| per channel

# (N, H, W, Cin, Cout)
CASES = {
    "3x5x7_c64_128": (3, 5, 7, 64, 128),
    "2x9x14_c128_128": (2, 9, 14, 128, 128),
    "2x6x28_c64_256": (2, 6, 28, 64, 256),
    "130x1x1_c64_128": (130, 1, 1, 64, 128),
    "3x7x7_c192_128": (3, 7, 7, 192, 128),
}
# the 64-input-channel shapes mirrored, for the input gradient only (see the module docstring)
DGRAD_EXTRA = {
    "3x5x7_c128_64": (3, 5, 7, 128, 64),
    "2x6x28_c256_64": (2, 6, 28, 256, 64),
    "130x1x1_c128_64": (130, 1, 1, 128, 64),
}
ALL = dict(CASES, **DGRAD_EXTRA)


def _say(*a):
    print("[patch]", *a, flush=True)


def _ext():
    from cloud_amd.ops import _ext as e

    return e.load(required=True)


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


def _partials_err(part, terms_a, terms_b):
    """Statistics partials [rows][2][C]: every row finite (the buffer was pre-filled with NaN);
    the float64 sum of the rows against the float64 sum of the terms [M, C], per channel, as a
    multiple of PART_BOUND * sum |term| (<= 1 passes)."""
    assert torch.isfinite(part).all(), "a statistics partial row was not written"
    worst = 0.0
    for k, t in ((0, terms_a), (1, terms_b)):
        got = part[:, k].double().sum(0).cpu()
        err = (got - t.sum(0)).abs()
        lim = PART_BOUND * t.abs().sum(0)
        assert (err[lim == 0] == 0).all()
        worst = max(worst, (err / lim.clamp_min(1e-300)).max().item())
    return worst


def _relu_bits(keep):
    """[M, C] bool -> the kernels' ReLU bitmask [M, C/8] uint8 (bit j = channel 8c + j)."""
    M, C = keep.shape
    w = (1 << torch.arange(8)).to(torch.int32)
    return (keep.view(M, C // 8, 8).to(torch.int32) * w).sum(-1).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _data(name):
    """bf16 operands (host) and their float64 forward / input gradient, computed once per process
    and shared by every test of the case (never modified)."""
    N, H, W, Cin, Cout = ALL[name]
    g = torch.Generator().manual_seed(7000 + list(ALL).index(name))
    x = torch.randn(N, H, W, Cin, generator=g).to(BF16)
    w = (torch.randn(Cout, 3, 3, Cin, generator=g) / math.sqrt(9 * Cin)).to(BF16)
    dy = torch.randn(N, H, W, Cout, generator=g).to(BF16)
    z = (torch.randn(N, H, W, Cin, generator=g) * 2 + 0.5).to(BF16)
    keep = torch.rand(N * H * W, Cin, generator=g) > 0.4
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    wr = w.double().permute(0, 3, 1, 2).contiguous()
    yr = F.conv2d(xr, wr, None, 1, 1)
    yr.backward(dy.double().permute(0, 3, 1, 2).contiguous())
    return dict(x=x, w=w, dy=dy, z=z, keep=keep, y=yr.detach().permute(0, 2, 3, 1).contiguous(),
                dx=xr.grad.permute(0, 2, 3, 1).contiguous())


def _assert_patch_dispatch(name, dgrad):
    """The direction of the case runs on the patch-fed core in this process -- except, by the
    dispatch rule, with 64 or fewer output columns (Cout forward, Cin input gradient)."""
    N, H, W, Cin, Cout = ALL[name]
    want = (Cin if dgrad else Cout) > 64
    got = _ext().conv_patch_shape(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, int(dgrad))
    assert got == want, f"{name}: {'dgrad' if dgrad else 'forward'} on the patch core: {got}, expected {want}"
    return got


def test_dispatch_predicate_boundaries():
    """What the predicate must refuse: strides, other filters / paddings, W > 28, 64 or fewer
    output columns, a gathered channel count that is no multiple of 64."""
    ext = _ext()
    ok = (4, 14, 14, 128, 128, 3, 3, 1, 1, 1, 1)
    assert ext.conv_patch_shape(*ok, 0) and ext.conv_patch_shape(*ok, 1)
    assert ext.conv_patch_shape(4, 28, 28, 128, 128, 3, 3, 1, 1, 1, 1, 0)
    for bad in [(4, 14, 14, 128, 128, 3, 3, 2, 2, 1, 1), (4, 14, 14, 128, 128, 3, 3, 1, 1, 0, 0),
                (4, 14, 14, 128, 128, 5, 5, 1, 1, 2, 2), (4, 14, 29, 128, 128, 3, 3, 1, 1, 1, 1),
                (4, 56, 56, 64, 64, 3, 3, 1, 1, 1, 1)]:
        assert not ext.conv_patch_shape(*bad, 0) and not ext.conv_patch_shape(*bad, 1), bad
    # forward gathers Cin and writes Cout columns, the input gradient the other way round
    assert ext.conv_patch_shape(4, 14, 14, 64, 128, 3, 3, 1, 1, 1, 1, 0)
    assert not ext.conv_patch_shape(4, 14, 14, 64, 128, 3, 3, 1, 1, 1, 1, 1)  # 64 output columns
    assert not ext.conv_patch_shape(4, 14, 14, 72, 128, 3, 3, 1, 1, 1, 1, 0)  # Cin % 64
    assert not ext.conv_patch_shape(4, 14, 14, 128, 72, 3, 3, 1, 1, 1, 1, 1)  # Cout % 64


@pytest.mark.parametrize("name", list(CASES))
def test_patch_forward_vs_fp64(name):
    """conv_fwd without and with the statistics partials: rows against float64, the two outputs
    bitwise equal, every partial row written, sums and sums of squares of the stored bf16 output
    within 2^-20 * sum |term| per channel."""
    from cloud_amd.ops import raw

    N, H, W, Cin, Cout = CASES[name]
    assert _assert_patch_dispatch(name, False)
    d = _data(name)
    x, w = d["x"].to(DEV), d["w"].to(DEV)
    y0 = raw.conv_fwd(x, w, 1, 1)
    part = raw.conv_stats_buffer(tuple(x.shape), w, 1, 1, x.device).fill_(NAN)
    assert part.shape == ((N * H * W + 127) // 128, 2, Cout)
    y1 = raw.conv_fwd(x, w, 1, 1, stats=part)
    torch.cuda.synchronize()
    e_y, zr = _row_err(y0, d["y"])
    yd = y1.double().cpu().reshape(-1, Cout)
    worst = _partials_err(part, yd, yd * yd)
    _say(f"fwd {name} {CASES[name]}: y/row {e_y:.3e} ({zr} zero rows), {part.shape[0]} partial rows, "
         f"err / bound {worst:.3f}, stats output bitwise equal: {torch.equal(y0, y1)}")
    assert y0.shape == d["y"].shape and y0.dtype == BF16
    assert e_y < ROW_BOUND, e_y
    assert torch.equal(y0, y1)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("name", list(ALL))
def test_patch_dgrad_vs_fp64(name):
    """conv_dgrad plain and with bn=(z, mask) (random ReLU bitmask): rows against float64, dx of
    the two bitwise equal, [sum g | sum g * z] with g = dx * relu' from the stored bf16 dx."""
    from cloud_amd.ops import raw

    N, H, W, Cin, Cout = ALL[name]
    on_patch = _assert_patch_dispatch(name, True)
    assert on_patch or name in CASES
    d = _data(name)
    w, dy, z = d["w"].to(DEV), d["dy"].to(DEV), d["z"].to(DEV)
    bits = _relu_bits(d["keep"]).to(DEV)
    shape = (N, H, W, Cin)
    plain = raw.conv_dgrad(dy, w, shape, 1, 1, out=torch.full(shape, NAN, dtype=BF16, device=DEV), beta=0.0)
    dx, part = raw.conv_dgrad(dy, w, shape, 1, 1, out=torch.full(shape, NAN, dtype=BF16, device=DEV), bn=(z, bits))
    torch.cuda.synchronize()
    e_dx, zr = _row_err(plain, d["dx"])
    assert part.shape == ((N * H * W + 127) // 128, 2, Cin)
    gd = dx.double().cpu().reshape(-1, Cin) * d["keep"]
    worst = _partials_err(part, gd, gd * d["z"].double().reshape(-1, Cin))
    _say(f"dgrad {name} {ALL[name]} patch core {on_patch}: dx/row {e_dx:.3e} ({zr} zero rows), {part.shape[0]} partial rows, "
         f"err / bound {worst:.3f}, bn output bitwise equal: {torch.equal(plain, dx)}")
    assert e_dx < ROW_BOUND, e_dx
    assert torch.equal(plain, dx)
    assert worst <= 1.0, worst


def test_patch_inputs_inside_nan_allocation():
    """x (forward) and dy (input gradient) as views into the middle of a larger NaN-filled
    allocation: the patch rows before the tensor and past its end must read as zeros (a buffer
    span wider than the tensor, or a border handled by multiplying with zero, gives NaN)."""
    from cloud_amd.ops import raw

    name = "2x9x14_c128_128"
    N, H, W, Cin, Cout = CASES[name]
    assert _assert_patch_dispatch(name, False) and _assert_patch_dispatch(name, True)
    d = _data(name)
    w = d["w"].to(DEV)

    def embedded(t):
        pad = 64 * W * t.shape[-1]  # more than a patch's W + 1 halo rows on either side
        big = torch.full((t.numel() + 2 * pad,), NAN, dtype=BF16, device=DEV)
        v = big[pad:pad + t.numel()].view(t.shape)
        v.copy_(t.to(DEV))
        assert v.is_contiguous() and v.data_ptr() % 16 == 0
        return big, v

    bx, xv = embedded(d["x"])
    bd, dv = embedded(d["dy"])
    y = raw.conv_fwd(xv, w, 1, 1)
    dx = raw.conv_dgrad(dv, w, (N, H, W, Cin), 1, 1)
    torch.cuda.synchronize()
    assert torch.isfinite(y.float()).all() and torch.isfinite(dx.float()).all(), "NaN leaked in from outside the tensor"
    e_y, _ = _row_err(y, d["y"])
    e_dx, _ = _row_err(dx, d["dx"])
    _say(f"nan-embedded {name}: y/row {e_y:.3e} dx/row {e_dx:.3e}")
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND, (e_y, e_dx)
    assert torch.equal(y, raw.conv_fwd(d["x"].to(DEV), w, 1, 1))


_IMPLICIT_RUN = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch
import test_conv_patch_gpu as T
from cloud_amd.ops import raw
N, H, W, Cin, Cout = T.CASES[{name!r}]
assert not T._ext().conv_patch_shape(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, 0)
assert not T._ext().conv_patch_shape(N, H, W, Cin, Cout, 3, 3, 1, 1, 1, 1, 1)
d = T._data({name!r})
x, w, dy = (d[k].to("cuda") for k in ("x", "w", "dy"))
y = raw.conv_fwd(x, w, 1, 1)
dx = raw.conv_dgrad(dy, w, (N, H, W, Cin), 1, 1)
torch.cuda.synchronize()
torch.save(dict(y=y.cpu(), dx=dx.cpu()), {out!r})
print("IMPLICIT_OK")
"""


def test_patch_vs_implicit_gemm(tmp_path):
    """The same seeded inputs through a fresh process with CLOUD_AMD_CONV_PATCH=0 (the switch is
    read once per process): |patch - implicit| <= 2^-7 |ref| + 1e-6 elementwise, the halo-vs-implicit
    criterion of test_resnet_kernel_edges_gpu.py."""
    from cloud_amd.ops import raw

    name = "2x9x14_c128_128"
    N, H, W, Cin, Cout = CASES[name]
    assert _assert_patch_dispatch(name, False) and _assert_patch_dispatch(name, True)
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    out = str(tmp_path / "implicit.pt")
    env = dict(os.environ)
    env["CLOUD_AMD_CONV_PATCH"] = "0"
    code = _IMPLICIT_RUN.format(root=root, tests=tests, name=name, out=out)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110)
    print(r.stdout)
    assert r.returncode == 0 and "IMPLICIT_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    imp = torch.load(out)
    d = _data(name)
    x, w, dy = (d[k].to(DEV) for k in ("x", "w", "dy"))
    y = raw.conv_fwd(x, w, 1, 1).cpu()
    dx = raw.conv_dgrad(dy, w, (N, H, W, Cin), 1, 1).cpu()
    c_y = ((y.double() - imp["y"].double()).abs() / (2.0 ** -7 * d["y"].abs() + 1e-6)).max().item()
    c_dx = ((dx.double() - imp["dx"].double()).abs() / (2.0 ** -7 * d["dx"].abs() + 1e-6)).max().item()
    _say(f"patch-vs-implicit {name}: y {c_y:.3f} dx {c_dx:.3f} (|a - b| / (2^-7 |ref| + 1e-6))")
    assert c_y <= 1.0 and c_dx <= 1.0, (c_y, c_dx)
