"""Geometry-edge reference tests for the ResNet-path kernels: the implicit-GEMM convolutions
(conv.hip: forward, input gradient, split-K weight gradient, their BN-statistics epilogues), the
LDS-resident 3x3 kernel (ca_conv_halo.h), the max-pools and the fused stem tail (pool.hip) and
the BatchNorm statistics with a large mean (bn.hip; everything else about the BatchNorm kernels
and the global pools -- tiling branches, gates, backward, switches -- is in
test_bn_kernel_edges_gpu.py, with its references in test_bn_reference_cpu.py).

Every reference is computed in float64 on the host from the same bf16 operands the kernel reads;
inputs come from a host ``torch.Generator``.  The shapes are the smallest that enter the loader
branches the older (all square) tests never reach: H != W so that a swapped fast-division pair or
pitch shows, weight-gradient split-K blocks that start in the middle of a row of a later image,
several image carries inside one block with a ragged last K tile, strided maps, 5x5 / 2x3 / 6x6 /
"valid" / over-padded filters, a one-pixel image, and the halo kernel at one and two row tiles.

Metrics are local: forward outputs and input gradients per pixel row (over the channel vector,
against max(row norm, median row norm)), weight gradients per filter tap, statistics partials
per channel against 2^-20 * sum |term|, max-pool outputs bitwise with an explicit first-tap tie
rule.  Rows / taps whose true value is structurally zero must be exactly zero.

Worst figures observed on an MI355X (each test prints its figures before asserting):

    group                                                     worst observed              bound
    conv geometry matrix   y, dx / row                        2.49e-3, 2.82e-3            1e-2
    conv geometry matrix   dw fp32 / bf16 per tap             1.4e-7 / 1.84e-3            2e-3 / 2e-2
    conv through autograd  y, dx / row; dw bf16 / tap         2.3e-3; 1.70e-3             1e-2; 2e-2
    general loaders (CLOUD_AMD_TAPMASK=0)  row; taps          2.43e-3; 1.0e-7 / 1.69e-3   as above
    register-staged loaders (CLOUD_AMD_GEMM_CORE=reg)         2.43e-3; 1.0e-7 / 1.69e-3   as above
    conv forward statistics partials, err / bound             0.31                        1
    conv dgrad BN-backward partials, err / bound              0.034                       1
    halo kernel y, dx / row                                   2.36e-3, 2.39e-3            1e-2
    halo kernel dw fp32 / bf16 per tap                        1.3e-7 / 1.71e-3            2e-3 / 2e-2
    halo kernel partials fwd / bwd, err / bound               0.14 / 0.024                1
    halo vs implicit GEMM dx, |a - b| / (2^-7 |ref| + 1e-6)   0.98                        1
    max-pool dx, |got - ref| / (2^-8 |ref| + 1e-6)            0.996                       1
    stem tail dz / row                                        5.19e-3                     2e-2
    stem tail dgamma, dbeta, err / (2^-8 sum |term|)          0.30, 0.27                  1
    stem tail mean / rstd vs float64 of the partials          1.6e-8 / 5.5e-8             1e-5
    BN rstd with a large mean                                 see the table below

BN statistics with a large mean (M = 234; relative error of rstd against a float64 two-pass
variance; "one-pass" is fp32 sum / sum of squares combined as q / M - mean^2 in float64):

    mean  spread   fp32 one-pass   kernel reduction   from partials   bound = max(4 x one-pass, 1e-5)
    0     1        4.5e-8          6.4e-8             5.1e-8          1e-5
    0     0.25     7.9e-8          7.4e-8             6.1e-8          1e-5
    4     1        5.6e-7          5.4e-8             3.2e-7          1e-5
    4     0.25     2.9e-14         2.6e-8             2.6e-8          1e-5
    32    1        1.1e-13         5.3e-8             5.3e-8          1e-5
    32    0.25     2.1e-12         5.1e-8             5.1e-8          1e-5
    128   1        2.0e-12         5.5e-8             5.5e-8          1e-5
    128   0.25     2.0e-11         4.9e-8             4.9e-8          1e-5
(at M = 234 the fp32 sums of bf16 values are nearly exact, so the floor holds: see the test)
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

ROW_BOUND = 1e-2        # bf16 outputs per row (the BERT edge tests' bound)
WG32_BOUND = 2e-3       # weight gradient into fp32, per tap (test_conv_halo_gpu.py)
WGBF_BOUND = 2e-2       # weight gradient into bf16, per tap (test_conv_halo_gpu.py)
PART_BOUND = 2.0 ** -20  # statistics partials: |err| <= 2^-20 * sum |term| per channel


def _say(*a):
    print("[edges]", *a, flush=True)


def _ext():
    from cloud_amd.ops import _ext as e

    return e.load(required=True)


def _out_hw(n, k, s, p):
    return (n + 2 * p - k) // s + 1


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


def _tap_err(got, ref, dw, zero_value):
    """Per filter tap (kh, kw) over the [Cout, Cin] slice: ||got - ref|| / ||ref||, maximum over
    taps.  A tap whose true gradient slice ``dw`` is exactly zero must hold ``zero_value`` (0, or
    the accumulated-into tensor) exactly."""
    g = got.detach().double().cpu()
    assert g.shape == ref.shape and torch.isfinite(g).all()
    zero = dw.pow(2).sum((0, 3)) == 0  # [KH, KW]
    gz = g.permute(1, 2, 0, 3)[zero]
    assert torch.equal(gz, zero_value.double().permute(1, 2, 0, 3)[zero]), "structurally zero taps must stay exact"
    d = (g - ref).pow(2).sum((0, 3)).sqrt()
    n = ref.pow(2).sum((0, 3)).sqrt()
    live = ~zero
    assert live.any()
    return (d[live] / n[live]).max().item(), int(zero.sum())


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


# ------------------------------------------------------------------------------- convolution cases

# (N, H, W, Cin, Cout, KH, KW, stride, pad)
CASES = {
    # tap-mask forward / dgrad on the tall 256 x 64 tile (M = 351: one full tile and a 95-row tail,
    # image boundaries inside a tile); GConvWgradBT linear path
    "3x3_9x13": (3, 9, 13, 64, 64, 3, 3, 1, 1),
    # 128 x 128 tiles, two channel slices per tap, Cout tail 192 = 128 + 64
    "3x3_13x9_c128": (3, 13, 9, 128, 192, 3, 3, 1, 1),
    # strided dgrad by parity class on the tap-mask loaders (GConvDgradSAT / SBT); Hq 8 / 7, Wq 5 / 5
    "s2_15x10": (2, 15, 10, 64, 128, 3, 3, 2, 1),
    # the same on the general class loaders (Cout % 64 != 0); general forward loader
    "s2_10x15_c24": (2, 10, 15, 24, 40, 3, 3, 2, 1),
    # strided 1x1: three of four parity classes have no tap, their dx is exactly zero
    "1x1s2_11x7": (3, 11, 7, 128, 256, 1, 1, 2, 0),
    # 49 taps (> 32: general loaders), rectangular
    "7x7s2_12x20": (2, 12, 20, 8, 64, 7, 7, 2, 3),
    # row-segment loader (GConvRowA, KW * Cin == 64) on a rectangle
    "rowseg_9x12": (2, 9, 12, 16, 64, 4, 4, 1, 0),
    # GConvWgradBI, 3 effective splits: kred 1680, k_per_split 576 -- blocks start at pixel 156 of
    # image 1 and pixel 312 of image 2, neither at a row start
    "walk_20x21_3split": (4, 20, 21, 64, 64, 3, 3, 1, 1),
    # GConvWgradBI, one block crossing four image boundaries; kred 660: the last K tile holds 20 pixels
    "walk_12x11_5img": (5, 12, 11, 64, 128, 3, 3, 1, 1),
    # GConvWgradBI on a strided rectangular map (17 x 12, kred 612)
    "walk_s2_33x23": (3, 33, 23, 64, 64, 3, 3, 2, 1),
    # the same with 2 splits (21 x 14, kred 1176: the second block starts at image 2, row 3, column 10)
    "walk_s2_41x27_2split": (4, 41, 27, 64, 64, 3, 3, 2, 1),
    # GConvWgradBI on a one-row map wider than a K tile (dya = 0, dxa = 64): every row carry is
    # also an image carry; kred 390
    "walk_wide_1x130": (3, 1, 130, 64, 64, 3, 3, 1, 1),
    # 25 tap-mask bits
    "5x5_9x11": (2, 9, 11, 64, 64, 5, 5, 1, 2),
    # "valid" 3x3: every mask full, `lin` false
    "valid_9x12": (2, 9, 12, 64, 64, 3, 3, 1, 0),
    # padding 2 with a 3x3: output larger than input, border windows with one live tap
    "pad2_7x9": (2, 7, 9, 64, 64, 3, 3, 1, 2),
    # KH != KW; Cout 72 (dgrad cout_tile off, N tail of 8)
    "2x3_9x12_c72": (2, 9, 12, 64, 72, 2, 3, 1, 0),
    # 36 taps with Cin % 64 == 0: the KH * KW <= 32 guard sends it to the general loader
    "6x6_10x8": (2, 10, 8, 64, 64, 6, 6, 1, 0),
    # the smallest legal convolution: one pixel, one live tap
    "1px": (1, 1, 1, 8, 8, 3, 3, 1, 1),
}
# minimum effective split-K blocks the case exists for, and the workgroup target handed to
# raw.conv_wgrad (explicit, so that a retuned default cannot turn these into single-split runs)
SPLIT_CASES = {"walk_20x21_3split": 3, "walk_s2_41x27_2split": 2}
SPLIT_BLOCKS = 1024
WALK_CASES = [k for k in CASES if k.startswith("walk_")]


@functools.lru_cache(maxsize=None)
def _conv_data(name):
    """bf16 operands (host) and the float64 forward / input-gradient / weight-gradient of them,
    computed once per process and shared by every test of the case (never modified)."""
    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    OH, OW = _out_hw(H, KH, s, p), _out_hw(W, KW, s, p)
    x = torch.randn(N, H, W, Cin, generator=g).to(BF16)
    w = (torch.randn(Cout, KH, KW, Cin, generator=g) / math.sqrt(KH * KW * Cin)).to(BF16)
    dy = torch.randn(N, OH, OW, Cout, generator=g).to(BF16)
    prev = torch.randn(Cout, KH, KW, Cin, generator=g).to(BF16)
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    wr = w.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    yr = F.conv2d(xr, wr, None, s, p)
    yr.backward(dy.double().permute(0, 3, 1, 2).contiguous())
    return dict(x=x, w=w, dy=dy, prev=prev, y=yr.detach().permute(0, 2, 3, 1).contiguous(),
                dx=xr.grad.permute(0, 2, 3, 1).contiguous(), dw=wr.grad.permute(0, 2, 3, 1).contiguous())


def _wgrad_plan(name, blocks=None):
    """What raw.conv_wgrad and ca_conv_wgrad will do for the case: (effective splits,
    k_per_split, OH, OW, kred)."""
    from cloud_amd import config
    from cloud_amd.ops import raw

    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    OH, OW = _out_hw(H, KH, s, p), _out_hw(W, KW, s, p)
    kred = N * OH * OW
    target = blocks or config.get("CLOUD_AMD_WGRAD_BLOCKS_SMALLM" if Cout <= 128 else "CLOUD_AMD_WGRAD_BLOCKS")
    asked = _ext().gemm_splitk_effective(kred, raw.wgrad_splits(Cout, KH * KW * Cin, kred, target_blocks=target))
    kps = max(-(-(kred // asked) // 64) * 64, 64)  # the launcher's k_per_split from the splits it is handed
    return -(-kred // kps), kps, OH, OW, kred


def _assert_split_properties(name, eff, kps, OH, OW, kred):
    """The properties the GConvWgradBI cases exist for (see CASES)."""
    assert OH * OW >= 128, "the incremental pixel walk needs OH * OW >= 2 * BK"
    if name in SPLIT_CASES:
        assert eff >= SPLIT_CASES[name], (name, eff)
        assert kps % (OH * OW) != 0, "a later block must start inside an image"
        assert kps % OW != 0, "a later block must start inside a row"
    else:
        assert eff == 1 and kred % 64 != 0 and kred // (OH * OW) >= 3, (name, eff, kred)


def _conv_case(name, tag="conv"):
    """conv_fwd, conv_dgrad (beta 0), conv_wgrad into fp32 (beta 0) and into a pre-filled bf16
    tensor (beta 1) of one case, each held to the float64 reference.  Outputs written with beta 0
    are pre-filled with NaN: every element must be written."""
    from cloud_amd.ops import raw

    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    d = _conv_data(name)
    x, w, dy, prev = (d[k].to(DEV) for k in ("x", "w", "dy", "prev"))
    blocks = SPLIT_BLOCKS if name in SPLIT_CASES else None
    y = raw.conv_fwd(x, w, s, p)
    dx = raw.conv_dgrad(dy, w, tuple(x.shape), s, p, out=torch.full_like(x, NAN), beta=0.0)
    dw32 = raw.conv_wgrad(dy, x, tuple(w.shape), s, p, out=torch.full(w.shape, NAN, device=DEV), beta=0.0,
                          blocks=blocks)
    dwbf = raw.conv_wgrad(dy, x, tuple(w.shape), s, p, out=prev.clone(), beta=1.0, blocks=blocks)
    torch.cuda.synchronize()
    assert y.shape == d["y"].shape and y.dtype == BF16
    e_y, _ = _row_err(y, d["y"])
    e_dx, z_dx = _row_err(dx, d["dx"])
    e_w32, z_w = _tap_err(dw32, d["dw"], d["dw"], torch.zeros(w.shape))
    e_wbf, _ = _tap_err(dwbf, d["prev"].double() + d["dw"], d["dw"], d["prev"])
    _say(f"{tag} {name} {CASES[name]}: y/row {e_y:.3e} dx/row {e_dx:.3e} ({z_dx} zero rows) "
         f"dw fp32/tap {e_w32:.3e} dw bf16/tap {e_wbf:.3e} ({z_w} zero taps)")
    assert e_y < ROW_BOUND, e_y
    assert e_dx < ROW_BOUND, e_dx
    assert e_w32 < WG32_BOUND, e_w32
    assert e_wbf < WGBF_BOUND, e_wbf
    return e_y, e_dx, e_w32, e_wbf, z_dx, z_w


@pytest.mark.parametrize("name", list(CASES))
def test_conv_geometry_vs_fp64(name):
    """The geometry matrix: one case per loader branch (see CASES), forward, input gradient and
    both weight-gradient output types against float64.  The split-K cases first recompute what
    the launcher will do and assert the properties they exist for."""
    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    if name in WALK_CASES:
        plan = _wgrad_plan(name, SPLIT_BLOCKS if name in SPLIT_CASES else None)
        _say(f"conv {name}: effective splits {plan[0]} k_per_split {plan[1]} map {plan[2]}x{plan[3]} kred {plan[4]}")
        _assert_split_properties(name, *plan)
    res = _conv_case(name)
    if name == "1x1s2_11x7":  # pixels no tap reaches: every row but those with h and w even
        assert res[4] == N * (H * W - ((H + 1) // 2) * ((W + 1) // 2))
    if name == "1px":
        assert res[5] == 8  # all taps but the centre


@pytest.mark.parametrize("name", ["walk_20x21_3split", "s2_15x10", "5x5_9x11", "2x3_9x12_c72"])
def test_conv_autograd_path_vs_fp64(name):
    """ops.conv2d_nhwc + autograd (_ConvFn: choose_wgrad_splits, weight gradient into a fresh bf16
    tensor with beta 0)."""
    from cloud_amd.ops import conv2d_nhwc
    from cloud_amd.ops.conv import choose_wgrad_splits

    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    d = _conv_data(name)
    if name in SPLIT_CASES:
        OH, OW = _out_hw(H, KH, s, p), _out_hw(W, KW, s, p)
        kred = N * OH * OW
        asked = _ext().gemm_splitk_effective(kred, choose_wgrad_splits(Cout, KH * KW * Cin, kred))
        kps = max(-(-(kred // asked) // 64) * 64, 64)
        _assert_split_properties(name, -(-kred // kps), kps, OH, OW, kred)
    x = d["x"].to(DEV).requires_grad_()
    w = d["w"].to(DEV).requires_grad_()
    y = conv2d_nhwc(x, w, None, s, p)
    y.backward(d["dy"].to(DEV))
    torch.cuda.synchronize()
    e_y, _ = _row_err(y, d["y"])
    e_dx, _ = _row_err(x.grad, d["dx"])
    e_w, _ = _tap_err(w.grad, d["dw"], d["dw"], torch.zeros(w.shape))
    _say(f"conv-autograd {name}: y/row {e_y:.3e} dx/row {e_dx:.3e} dw bf16/tap {e_w:.3e}")
    assert w.grad.dtype == BF16
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND, (e_y, e_dx)
    assert e_w < WGBF_BOUND, e_w


_FALLBACK_CHECK = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_resnet_kernel_edges_gpu as T
for name in ("3x3_9x13", "s2_15x10", "5x5_9x11"):
    T._conv_case(name, tag={tag!r})
print("FALLBACK_OK")
"""


@pytest.mark.parametrize("var,value", [("CLOUD_AMD_TAPMASK", "0"), ("CLOUD_AMD_GEMM_CORE", "reg")])
def test_conv_fallback_loaders(var, value):
    """CLOUD_AMD_TAPMASK=0 sends every convolution to the general LDS-DMA gather loaders,
    CLOUD_AMD_GEMM_CORE=reg to the register-staged loaders (ConvFwdA / ConvDgradA / ConvDgradB /
    ConvWgradB).  Both switches are read once per process, so each check runs in its own
    interpreter, one after the other, against the same references and bounds."""
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    env = dict(os.environ)
    env[var] = value
    code = _FALLBACK_CHECK.format(root=root, tests=tests, tag=f"conv[{var}={value}]")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110)
    print(r.stdout)
    assert r.returncode == 0 and "FALLBACK_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_unsupported_geometries_are_refused_before_launch():
    """Channel counts that are no multiple of 8 (every gather is a 16-byte chunk), a pooling window
    whose argmax does not fit its byte, and a stem-tail width whose channel groups do not divide
    the block: the launchers raise before anything runs (accumulate-into tensors untouched), and
    the dispatch predicates of the autograd ops send such inputs elsewhere."""
    from cloud_amd.ops import max_pool2d_nhwc, raw
    from cloud_amd.ops.conv import _native_conv_ok
    from cloud_amd.ops.pooling import stem_tail_ok

    ext = _ext()
    x = torch.ones(1, 5, 6, 12, dtype=BF16, device=DEV)
    w = torch.ones(8, 3, 3, 12, dtype=BF16, device=DEV)
    dy = torch.ones(1, 5, 6, 8, dtype=BF16, device=DEV)
    dx = torch.full_like(x, 3.0)
    dw = torch.full(w.shape, 3.0, device=DEV)
    assert not _native_conv_ok(x, w)
    with pytest.raises(RuntimeError):
        raw.conv_fwd(x, w, 1, 1)
    with pytest.raises(RuntimeError):
        raw.conv_dgrad(dy, w, tuple(x.shape), 1, 1, out=dx, beta=1.0)
    with pytest.raises(RuntimeError):
        raw.conv_wgrad(dy, x, tuple(w.shape), 1, 1, out=dw, beta=1.0)
    with pytest.raises(RuntimeError):
        max_pool2d_nhwc(torch.ones(1, 16, 16, 8, dtype=BF16, device=DEV), 16, 16, 0)
    N, H, W, C = 1, 5, 6, 24  # 256 % (C / 8) != 0
    z = torch.ones(N, H, W, C, dtype=BF16, device=DEV)

    class _BN:
        training, relu = True, True

    class _Pool:
        k, stride, padding = 3, 2, 1

    assert stem_tail_ok(z[..., :8].contiguous(), _BN, _Pool, z) and not stem_tail_ok(z, _BN, _Pool, z)
    yp = torch.ones(N, 3, 3, C, dtype=BF16, device=DEV)
    idx = torch.zeros(N, 3, 3, C, dtype=torch.uint8, device=DEV)
    part = torch.full((ext.maxpool_bnstats_parts(N, H, W, C), 2, C), 3.0, device=DEV)
    with pytest.raises(RuntimeError):
        ext.maxpool_bwd_s2k3_bnstats(yp.data_ptr(), yp.data_ptr(), idx.data_ptr(), z.data_ptr(), 0, part.data_ptr(),
                                     N, H, W, C, 3, 3, 0)
    torch.cuda.synchronize()
    assert (dx == 3).all() and (dw == 3).all() and (part == 3).all()


# ------------------------------------------------------------------------------- statistics epilogues


@pytest.mark.parametrize("name", ["3x3_9x13", "3x3_13x9_c128", "s2_15x10", "rowseg_9x12", "5x5_9x11"])
def test_conv_forward_statistics_on_rectangles(name):
    """conv_fwd(stats=): every partial row written, sums AND sums of squares of the stored bf16
    output per channel within 2^-20 * sum |term| (the tiles' fp32 chains: 4 - 8 rows per thread,
    then 16 - 32 thread partials per column; the rows are combined in float64), and the output
    bitwise that of the call without statistics."""
    from cloud_amd.ops import raw

    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    d = _conv_data(name)
    x, w = d["x"].to(DEV), d["w"].to(DEV)
    y0 = raw.conv_fwd(x, w, s, p)
    part = raw.conv_stats_buffer(tuple(x.shape), w, s, p, x.device).fill_(NAN)
    assert part.shape == (_ext().conv_stat_rows(N, H, W, Cin, Cout, KH, KW, s, s, p, p), 2, Cout)
    y1 = raw.conv_fwd(x, w, s, p, stats=part)
    torch.cuda.synchronize()
    assert torch.equal(y0, y1)
    yd = y1.double().cpu().reshape(-1, Cout)
    worst = _partials_err(part, yd, yd * yd)
    _say(f"conv-stats-fwd {name}: {part.shape[0]} partial rows, err / bound {worst:.3f}")
    assert worst <= 1.0, worst
    assert _row_err(y1, d["y"])[0] < ROW_BOUND


@pytest.mark.parametrize("name", ["s2_15x10", "3x3_9x13"])
def test_conv_dgrad_bn_statistics_on_rectangles(name):
    """conv_dgrad(bn=(z, mask)): dx bitwise the plain input gradient; [sum g | sum g * z] with g =
    dx * relu' taken from the stored bf16 dx, per channel; every partial row written (four
    parity classes' rows follow each other on the strided case)."""
    from cloud_amd.ops import _ext as E
    from cloud_amd.ops import raw

    ext = _ext()
    N, H, W, Cin, Cout, KH, KW, s, p = CASES[name]
    d = _conv_data(name)
    w, dy = d["w"].to(DEV), d["dy"].to(DEV)
    g = torch.Generator().manual_seed(77)
    z_h = (torch.randn(N, H, W, Cin, generator=g) * 2 + 0.5).to(BF16)
    keep = torch.rand(N * H * W, Cin, generator=g) > 0.4
    z, bits = z_h.to(DEV), _relu_bits(keep).to(DEV)
    shape = (N, H, W, Cin)
    plain = raw.conv_dgrad(dy, w, shape, s, p)
    rows = ext.conv_dgrad_stat_rows(N, H, W, Cin, Cout, KH, KW, s, s, p, p, 0.0)
    part = torch.full((rows, 2, Cin), NAN, device=DEV)
    dx = torch.full(shape, NAN, dtype=BF16, device=DEV)
    ext.conv_dgrad_bnstats(dy.data_ptr(), w.data_ptr(), dx.data_ptr(), N, H, W, Cin, Cout, KH, KW, s, s, p, p, 0.0,
                           z.data_ptr(), bits.data_ptr(), part.data_ptr(), E.stream_handle(dy.device))
    dx2, part2 = raw.conv_dgrad(dy, w, shape, s, p, bn=(z, bits))
    torch.cuda.synchronize()
    assert torch.equal(dx, plain) and torch.equal(dx2, plain)
    assert part2.shape == part.shape and torch.equal(part2, part)
    if s > 1:
        assert rows == sum(-(-N * ((H - a + 1) // 2) * ((W - b + 1) // 2) // 128) for a in (0, 1) for b in (0, 1))
    gd = dx.double().cpu().reshape(-1, Cin) * keep
    worst = _partials_err(part, gd, gd * z_h.double().reshape(-1, Cin))
    _say(f"conv-stats-bwd {name}: {rows} partial rows, err / bound {worst:.3f}")
    assert worst <= 1.0, worst
    assert _row_err(dx, d["dx"])[0] < ROW_BOUND


# ------------------------------------------------------------------------------- halo kernel


@functools.lru_cache(maxsize=None)
def _halo_data(N, H):
    g = torch.Generator().manual_seed(500 + 10 * N + H)
    W, C = 56, 64
    x = torch.randn(N, H, W, C, generator=g).to(BF16)
    w = (torch.randn(C, 3, 3, C, generator=g) / 24).to(BF16)
    dy = torch.randn(N, H, W, C, generator=g).to(BF16)
    prev = torch.randn(C, 3, 3, C, generator=g).to(BF16)
    z = (torch.randn(N, H, W, C, generator=g) * 2 + 0.5).to(BF16)
    keep = torch.rand(N * H * W, C, generator=g) > 0.4
    xr = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    wr = w.double().permute(0, 3, 1, 2).contiguous().requires_grad_()
    yr = F.conv2d(xr, wr, None, 1, 1)
    yr.backward(dy.double().permute(0, 3, 1, 2).contiguous())
    return dict(x=x, w=w, dy=dy, prev=prev, z=z, keep=keep, y=yr.detach().permute(0, 2, 3, 1).contiguous(),
                dx=xr.grad.permute(0, 2, 3, 1).contiguous(), dw=wr.grad.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("N,H", [(1, 8), (3, 8), (2, 16), (5, 24)])
def test_halo_kernel_small_heights(N, H):
    """The LDS-resident 3x3 kernel at H = 8 (both image borders in one tile), H = 16 (exactly two
    tiles) and H = 24, with fewer tiles than CUs: the partial-row and split counts equal to
    N * H / 8 prove that it ran.  Forward with statistics, input gradient with the BN-backward
    statistics, weight gradient into fp32 and bf16, all against float64; the beta = 1 input
    gradient into zeros runs on the implicit GEMM and is held to the halo kernel's within one
    bf16 ulp per element."""
    from cloud_amd.ops import raw

    ext = _ext()
    W, C = 56, 64
    tiles = N * H // 8
    geo = (N, H, W, C, C, 3, 3, 1, 1, 1, 1)
    assert ext.conv_stat_rows(*geo) == tiles
    assert ext.conv_dgrad_stat_rows(*geo, 0.0) == tiles
    assert ext.conv_dgrad_stat_rows(*geo, 1.0) == (N * H * W + 127) // 128 != tiles
    assert ext.conv_wgrad_splits(*geo, -1) == tiles
    d = _halo_data(N, H)
    x, w, dy, prev, z = (d[k].to(DEV) for k in ("x", "w", "dy", "prev", "z"))
    bits = _relu_bits(d["keep"]).to(DEV)
    shape = (N, H, W, C)

    part = raw.conv_stats_buffer(shape, w, 1, 1, x.device).fill_(NAN)
    assert part.shape[0] == tiles
    y = raw.conv_fwd(x, w, 1, 1, stats=part)
    assert torch.equal(y, raw.conv_fwd(x, w, 1, 1))
    dx, bpart = raw.conv_dgrad(dy, w, shape, 1, 1, out=torch.full(shape, NAN, dtype=BF16, device=DEV), bn=(z, bits))
    assert bpart.shape[0] == tiles
    dx_halo = raw.conv_dgrad(dy, w, shape, 1, 1)
    dx_gemm = raw.conv_dgrad(dy, w, shape, 1, 1, out=torch.zeros(shape, dtype=BF16, device=DEV), beta=1.0)
    dw32 = raw.conv_wgrad(dy, x, tuple(w.shape), 1, 1, out=torch.full(w.shape, NAN, device=DEV), beta=0.0)
    dwbf = raw.conv_wgrad(dy, x, tuple(w.shape), 1, 1, out=prev.clone(), beta=1.0)
    torch.cuda.synchronize()

    e_y, _ = _row_err(y, d["y"])
    e_dx, _ = _row_err(dx, d["dx"])
    e_dxg, _ = _row_err(dx_gemm, d["dx"])
    yd = y.double().cpu().reshape(-1, C)
    st_f = _partials_err(part, yd, yd * yd)
    gd = dx.double().cpu().reshape(-1, C) * d["keep"]
    st_b = _partials_err(bpart, gd, gd * d["z"].double().reshape(-1, C))
    cross = ((dx_halo.double() - dx_gemm.double()).abs().cpu() / (2.0 ** -7 * d["dx"].abs() + 1e-6)).max().item()
    e_w32, _ = _tap_err(dw32, d["dw"], d["dw"], torch.zeros(w.shape))
    e_wbf, _ = _tap_err(dwbf, d["prev"].double() + d["dw"], d["dw"], d["prev"])
    _say(f"halo N={N} H={H} ({tiles} tiles): y/row {e_y:.3e} dx/row {e_dx:.3e} implicit-GEMM dx/row {e_dxg:.3e} "
         f"partials fwd {st_f:.3f} bwd {st_b:.3f} halo-vs-GEMM {cross:.3f} ulp dw fp32/tap {e_w32:.3e} "
         f"bf16/tap {e_wbf:.3e}")
    assert torch.equal(dx, dx_halo)
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND and e_dxg < ROW_BOUND, (e_y, e_dx, e_dxg)
    assert st_f <= 1.0 and st_b <= 1.0, (st_f, st_b)
    assert cross <= 1.0, cross
    assert e_w32 < WG32_BOUND and e_wbf < WGBF_BOUND, (e_w32, e_wbf)


# ------------------------------------------------------------------------------- max-pool


def _pool_ref(x, k, s, p):
    """Explicit max-pool of x [N, H, W, C] (float64): the windows of the -inf padded input,
    their maximum, and the FIRST row-major tap that attains it (the kernel's strict '>' scan).
    Returns (y [N, OH, OW, C], tap [N, OH, OW, C], windows [N, OH, OW, C, k * k])."""
    N, H, W, C = x.shape
    xp = F.pad(x.permute(0, 3, 1, 2), (p, p, p, p), value=float("-inf"))
    win = xp.unfold(2, k, s).unfold(3, k, s)  # [N, C, OH, OW, k, k]
    OH, OW = win.shape[2], win.shape[3]
    assert (OH, OW) == (_out_hw(H, k, s, p), _out_hw(W, k, s, p))
    win = win.reshape(N, C, OH, OW, k * k).permute(0, 2, 3, 1, 4)
    m = win.max(-1).values
    taps = torch.arange(k * k).expand_as(win)
    first = torch.where(win == m[..., None], taps, torch.full_like(taps, k * k)).min(-1).values
    return m.contiguous(), first.contiguous(), win


def _pool_scatter(dy, tap, H, W, k, s, p):
    """float64 scatter-add of dy [N, OH, OW, C] to the argmax pixels."""
    N, OH, OW, C = dy.shape
    n, oh, ow, c = torch.meshgrid(torch.arange(N), torch.arange(OH), torch.arange(OW), torch.arange(C), indexing="ij")
    h = oh * s - p + tap // k
    w = ow * s - p + tap % k
    assert (h >= 0).all() and (h < H).all() and (w >= 0).all() and (w < W).all()
    dx = torch.zeros(N, H, W, C, dtype=torch.float64)
    dx.index_put_((n, h, w, c), dy.double(), accumulate=True)
    return dx


def _pool_input(N, H, W, C, seed):
    """Post-ReLU activations (about half exact zeros) with planted ties at 1.5, channel 0 all
    zero, channel 1 all negative (with ties at -0.5)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(N, H, W, C, generator=g))
    x[torch.rand(N, H, W, C, generator=g) < 0.15] = 1.5
    x[..., 0] = 0.0
    neg = -(torch.randn(N, H, W, generator=g).abs() + 0.125)
    neg[torch.rand(N, H, W, generator=g) < 0.3] = -0.5
    x[..., 1] = neg
    return x.to(BF16), g


def _pool_case(N, H, W, C, k, s, p, seed):
    from cloud_amd.ops import max_pool2d_nhwc

    x_h, g = _pool_input(N, H, W, C, seed)
    OH, OW = _out_hw(H, k, s, p), _out_hw(W, k, s, p)
    dy_h = torch.randn(N, OH, OW, C, generator=g).to(BF16)
    y_r, tap_r, win = _pool_ref(x_h.double(), k, s, p)
    dx_r = _pool_scatter(dy_h, tap_r, H, W, k, s, p)
    x = x_h.to(DEV).requires_grad_()
    y = max_pool2d_nhwc(x, k, s, p)
    (idx,) = y.grad_fn.saved_tensors
    idx = idx.cpu()
    y.backward(dy_h.to(DEV))
    torch.cuda.synchronize()
    assert y.dtype == BF16 and torch.equal(y.detach().double().cpu(), y_r), "pooled values must be bitwise equal"
    assert torch.equal(idx.long(), tap_r), "argmax: the first row-major tap that attains the maximum"
    dx = x.grad.double().cpu()
    assert (dx[dx_r == 0] == 0).all()
    ulps = ((dx - dx_r).abs() / (2.0 ** -8 * dx_r.abs() + 1e-6)).max().item()
    ties = (win == y_r[..., None]).sum(-1).gt(1).float().mean().item()
    assert ties > 0 or H * W == 1, "the case must contain tied windows"
    assert ulps <= 1.0, ulps
    return ulps, ties


@pytest.mark.parametrize("k,s,p", [(3, 1, 1), (3, 3, 0), (2, 2, 0), (3, 2, 0), (5, 2, 2), (2, 1, 0), (4, 2, 1)])
def test_maxpool_generic_windows_ties_routing(k, s, p):
    """maxpool_fwd_kernel / maxpool_bwd_kernel: overlapping, padded and stride-1 windows
    (oh0 / oh1 with negative numerators), C / 8 = 3 (not a power of two), ties everywhere."""
    for i, (N, H, W, C) in enumerate([(2, 7, 10, 24), (1, 5, 4, 8)]):
        ulps, ties = _pool_case(N, H, W, C, k, s, p, seed=31 * k + 7 * s + p + 100 * i)
        _say(f"maxpool k={k} s={s} p={p} {(N, H, W, C)}: dx {ulps:.3f} ulp, {ties:.0%} of windows tied")


@pytest.mark.parametrize("C", [8, 24])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (5, 6), (6, 5), (7, 7)])
def test_maxpool_3x3s2_specialisation(H, W, C):
    """maxpool_bwd_s2k3_kernel (one thread per 2 x 2 input block) on odd, even and one-pixel maps."""
    ulps, ties = _pool_case(3, H, W, C, 3, 2, 1, seed=1000 + 10 * H + W + C)
    _say(f"maxpool 3x3/2/1 H={H} W={W} C={C}: dx {ulps:.3f} ulp, {ties:.0%} of windows tied")


# ------------------------------------------------------------------------------- fused stem tail

STEM_DZ_BOUND = 2e-2  # the project's bound for bf16 gradients


def _bf16_round(t):
    return t.to(BF16).double()


def _stem_tail_run(z_h, gamma_h, beta_h, dy_h, recompute, monkeypatch):
    from cloud_amd.models.layers import BatchNormAct, MaxPool2d
    from cloud_amd.ops import gemm
    from cloud_amd.ops.pooling import stem_bn_relu_maxpool, stem_tail_ok

    monkeypatch.setenv("CLOUD_AMD_STEM_BWD_RECOMPUTE", "1" if recompute else "0")
    N, H, W, C = z_h.shape
    M = N * H * W
    z = z_h.to(DEV).requires_grad_()
    part = torch.empty(((M + 127) // 128, 2, C), device=DEV)
    gemm.fill_stats_torch(z.detach().view(M, C), part)
    bn = BatchNormAct(C, relu=True, device=DEV)
    with torch.no_grad():
        bn.weight.copy_(gamma_h.to(DEV))
        bn.bias.copy_(beta_h.to(DEV))
    assert stem_tail_ok(z, bn, MaxPool2d(3, 2, 1), part)
    y = stem_bn_relu_maxpool(z, bn, part)
    _, stats, _, idx, _ = y.grad_fn.saved_tensors
    stats, idx = stats.clone(), idx.clone()
    y.backward(dy_h.to(DEV))
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), idx=idx.cpu(), stats=stats.cpu(), part=part.cpu(), dz=z.grad.cpu(),
                dgamma=bn.weight.grad.cpu(), dbeta=bn.bias.grad.cpu())


@pytest.mark.parametrize("N,H,W,C", [(2, 5, 6, 8), (3, 6, 5, 32), (2, 7, 7, 128)])
def test_stem_tail_vs_fp64(N, H, W, C, monkeypatch):
    """stem_bn_relu_maxpool at C = 8, 32, 128 on odd / even maps, with CLOUD_AMD_STEM_BWD_RECOMPUTE
    1 and 0 (the WRITE_G instantiation and the bn_bwd hand-off): both settings bitwise equal.

    Reference: float64 BN from the statistics the partials give, each element rounded to bf16
    before the max (as the kernel documents), the explicit first-tap pool reference, then the
    float64 BN backward.  The kernel forms scale / shift and the FMA in fp32, so an element whose
    float64 value lies within 2^-20 (|z scale| + |mean scale| + |beta|) of a bf16 rounding
    boundary (or of the ReLU's zero) may legitimately round the other way; windows holding such
    an element are compared to one bf16 ulp instead of bitwise, the kernel's tap there must
    attain the window maximum to that ulp, and the backward reference routes those (few)
    windows as the kernel did.  Every other window is compared exactly, ties by the first-tap
    rule."""
    eps = 1e-5
    g = torch.Generator().manual_seed(N * 1000 + H * 100 + W * 10 + C)
    z_h = (torch.randn(N, H, W, C, generator=g) * 2 + 0.3).to(BF16)
    gamma_h = torch.rand(C, generator=g) + 0.5
    beta_h = torch.randn(C, generator=g) * 0.2
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    dy_h = torch.randn(N, OH, OW, C, generator=g).to(BF16)
    a = _stem_tail_run(z_h, gamma_h, beta_h, dy_h, True, monkeypatch)
    b = _stem_tail_run(z_h, gamma_h, beta_h, dy_h, False, monkeypatch)
    same = all(torch.equal(a[k], b[k]) for k in ("y", "idx", "dz", "dgamma", "dbeta"))

    M = N * H * W
    zd = z_h.double()
    mean = a["part"][:, 0].double().sum(0) / M
    var = (a["part"][:, 1].double().sum(0) / M - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    e_mu = ((a["stats"][:C].double() - mean).abs() / torch.maximum(mean.abs(), var.sqrt())).max().item()
    e_rs = (a["stats"][C:2 * C].double() / rstd - 1).abs().max().item()
    scale = gamma_h.double() * rstd
    shift = beta_h.double() - mean * scale
    t = zd * scale + shift
    act = torch.relu(_bf16_round(t))
    slack = 2.0 ** -20 * ((zd * scale).abs() + (mean * scale).abs() + beta_h.double().abs())
    unstable = torch.relu(_bf16_round(t - slack)) != torch.relu(_bf16_round(t + slack))
    y_r, tap_r, win = _pool_ref(act, 3, 2, 1)
    loose = _pool_ref(unstable.double(), 3, 2, 1)[0] > 0  # windows holding an unstable element
    y_k, tap_k = a["y"].double(), a["idx"].long()
    assert torch.equal(y_k[~loose], y_r[~loose]), "pooled values must be bitwise equal"
    assert torch.equal(tap_k[~loose], tap_r[~loose]), "argmax: first row-major tap of the bf16-rounded window"
    tol = 2.0 ** -7 * torch.maximum(y_r, y_k) + 1e-5
    assert ((y_k - y_r).abs() <= tol)[loose].all()
    assert (tap_k >= 0).all() and (tap_k < 9).all()
    at_k = win.gather(-1, tap_k[..., None])[..., 0]
    assert (at_k >= y_r - tol)[loose].all(), "the kernel's tap must attain the window maximum"
    frac = loose.float().mean().item()
    assert frac < 0.05, frac

    tap_u = torch.where(loose, tap_k, tap_r)
    y_u = torch.where(loose, y_k, y_r)
    gr = _pool_scatter(dy_h.double() * (y_u > 0), tap_u, H, W, 3, 2, 1)
    xhat = (zd - mean) * rstd
    dbeta = gr.sum((0, 1, 2))
    dgamma = (gr * xhat).sum((0, 1, 2))
    dz = scale * (gr - dbeta / M - xhat * dgamma / M)
    lim_b = 2.0 ** -8 * gr.abs().sum((0, 1, 2))
    lim_g = 2.0 ** -8 * (gr * xhat).abs().sum((0, 1, 2))
    figs = []
    for tag, r in (("recompute", a), ("write-g", b)):
        e_dz, _ = _row_err(r["dz"], dz)
        e_dg = ((r["dgamma"].double() - dgamma).abs() / lim_g.clamp_min(1e-300)).max().item()
        e_db = ((r["dbeta"].double() - dbeta).abs() / lim_b.clamp_min(1e-300)).max().item()
        figs.append((e_dz, e_dg, e_db))
        _say(f"stem-tail {(N, H, W, C)} {tag}: dz/row {e_dz:.3e} dgamma err/bound {e_dg:.3f} dbeta err/bound "
             f"{e_db:.3f} mean {e_mu:.2e} rstd {e_rs:.2e}; {int(loose.sum())} of {loose.numel()} windows within 1 ulp "
             f"({int(unstable.sum())} unstable elements); settings bitwise equal: {same}")
    assert e_mu < 1e-5 and e_rs < 1e-5, (e_mu, e_rs)
    for e_dz, e_dg, e_db in figs:
        # dgamma / dbeta: the kernel sums the bf16-rounded pooled gradient (2^-9 per term) in fp32
        assert e_dz < STEM_DZ_BOUND and e_dg <= 1.0 and e_db <= 1.0, (e_dz, e_dg, e_db)
    assert same, "CLOUD_AMD_STEM_BWD_RECOMPUTE = 1 and 0 must give bitwise-equal y, argmax, dz, dgamma, dbeta"


# ------------------------------------------------------------------------------- BN statistics, large mean

BN_MEANS, BN_SPREADS = (0.0, 4.0, 32.0, 128.0), (1.0, 0.25)


def test_bn_statistics_with_large_mean():
    """BN statistics are q / M - mean^2 from fp32 partial sums combined in double: channels whose
    mean is large next to their spread lose variance digits.  The kernel's own reduction and the
    convolution-style partials (fill_stats_torch) are held, per (mean, spread) group, to 4 x the
    error of a plain fp32 one-pass on the same input (floor 1e-5, the finalize test's
    tolerance), against a float64 two-pass mean / variance.

    At M = 234 the fp32 sums themselves are nearly exact -- a bf16 value has 8 significant bits,
    its square 16, and 234 terms of one magnitude add fewer than 8 -- so the one-pass error is
    ~1e-12 on the large-mean groups and the floor is what holds.  What the test guards is the
    combine: q / M - mean^2 formed in fp32 instead of double loses every digit of the variance
    at mean = 128 (an fp32 ulp of 16384 is 2e-3)."""
    from cloud_amd.ops import gemm, raw

    eps = 1e-5
    N, H, W, C = 2, 9, 13, 64
    M = N * H * W
    groups = [(m, s) for m in BN_MEANS for s in BN_SPREADS]
    per = C // len(groups)
    g = torch.Generator().manual_seed(4242)
    mvec = torch.tensor([m for m, _ in groups]).repeat_interleave(per)
    svec = torch.tensor([s for _, s in groups]).repeat_interleave(per)
    x_h = (mvec + svec * torch.randn(M, C, generator=g)).to(BF16)
    xd = x_h.double()
    mean64 = xd.mean(0)
    var64 = ((xd - mean64) ** 2).mean(0)
    sd64 = var64.sqrt()
    rstd64 = 1.0 / torch.sqrt(var64 + eps)

    def errs(mean, rstd):
        return ((mean.double() - mean64).abs() / torch.maximum(mean64.abs(), sd64),
                (rstd.double() / rstd64 - 1).abs())

    xf = x_h.float()
    s32, q32 = xf.sum(0), (xf ** 2).sum(0)  # plain fp32 one-pass
    m1 = s32.double() / M
    r1 = 1.0 / torch.sqrt((q32.double() / M - m1 * m1).clamp_min(0) + eps)
    ref_m, ref_r = errs(m1, r1)

    x = x_h.to(DEV).view(N, H, W, C)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    _, st_k, _ = raw.bn_fwd(x, gamma, beta, None, None, eps, 0.1, False)
    part = torch.empty(((M + 127) // 128, 2, C), device=DEV)
    gemm.fill_stats_torch(x.view(M, C), part)
    _, st_p, _ = raw.bn_fwd(x, gamma, beta, None, None, eps, 0.1, False, partials=part)
    torch.cuda.synchronize()
    ker_m, ker_r = errs(st_k[:C].cpu(), st_k[C:2 * C].cpu())
    par_m, par_r = errs(st_p[:C].cpu(), st_p[C:2 * C].cpu())
    bad = []
    for i, (m, s) in enumerate(groups):
        sl = slice(i * per, (i + 1) * per)
        rr, kr, pr = ref_r[sl].max().item(), ker_r[sl].max().item(), par_r[sl].max().item()
        rm, km, pm = ref_m[sl].max().item(), ker_m[sl].max().item(), par_m[sl].max().item()
        _say(f"bn-large-mean mean={m:g} spread={s:g}: rstd err one-pass {rr:.2e} kernel {kr:.2e} partials {pr:.2e} "
             f"(bound {max(4 * rr, 1e-5):.2e}); mean err one-pass {rm:.2e} kernel {km:.2e} partials {pm:.2e}")
        if not (kr <= max(4 * rr, 1e-5) and pr <= max(4 * rr, 1e-5) and km <= max(4 * rm, 1e-5)
                and pm <= max(4 * rm, 1e-5)):
            bad.append((m, s))
    assert not bad, bad
