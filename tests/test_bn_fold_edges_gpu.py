"""Edge-case reference tests for the BN-folded 1x1 GEMM kernels (csrc/include/ca_gemm_xa.h,
dispatched from csrc/kernels/gemm.hip: xa_launch, ca_gemm_xa, ca_gemm_xa_bwd_strided,
ca_gemm_xa_dw), the dense 1x1 input-gradient epilogues they share (ca_dgrad_gemm) and the
persistent resident-weight forward (ext.gemm_bf16 with statistics).

Every reference is float64 on the host, computed from exactly the bf16 operands the kernel reads;
inputs come from a host ``torch.Generator`` with a fixed seed per case.  Metrics are local, those
of test_resnet_kernel_edges_gpu.py: outputs per row, weight gradients per output-channel row,
statistics partials per channel against 2^-20 * sum |term|, the transformed operand per element.

The BN coefficients are drawn at FULL scale on purpose (backward A ~ N(0, 1), B ~ 0.3 N(0, 1),
D ~ N(0, 1); forward scale in [0.5, 1.5], shift ~ 0.75 + 0.5 N(0, 1)).  Rows past M read zeros,
so they transform to the constant D[k] (backward) or relu(shift[k]) (forward), not to zero: with
full-scale coefficients such a row is as large as a real one, and a leak of the rows between M and
the tile end into the statistics partials or into dW shows at full size instead of 10 - 100 x
attenuated.

Every output written with beta 0 is pre-filled with NaN, and every output tensor -- also the ones
the raw launchers allocate themselves -- is the leading view of an allocation with a guard tile
of 128 more rows that must keep its bit pattern (_Arena; the fill IS the guard pattern, a NaN).

Worst figures observed on an MI355X (each test prints its figures before asserting):

    group                                                     worst observed              bound
    A  transformed operand dz / y, err / bound (derived)      0.996 / 0.996               1
    A  forward out / row; partials err / bound                2.52e-3; 0.40               1e-2; 1
    A  backward dx / row; partials err / bound                3.13e-3; 0.096              1e-2; 1
    A  128 x 128 and one-deep 128 x 256 forms                 bitwise the default form's (partials 0.29 / 0.057)
    B  strided dz err / bound (derived); written dx / row     0.995; 2.05e-3              1; 1e-2
    B  sparse accumulate dx / row; partials err / bound       3.83e-3; 0.044              1e-2; 1
    B  skip_empty pair: written dx, accumulated dx / row      2.22e-3, 3.10e-3; 0.053     1e-2; 1
    C  dense 1x1 dgrad dx / row; partials err / bound         2.97e-3; 0.035              1e-2; 1
    D  fused dx / row; partials err / bound                   3.05e-3; 0.093              1e-2; 1
    D  fused dW per row, fp32 / bf16                          1.74e-5 / 2.21e-3           2e-3 / 2e-2
    E  CLOUD_AMD_XA_DW_DEPTH 0 / 2 / 4, _WAVES 8: dx; dW bf16 2.14e-3; 2.12e-3; 0.027     as D
    E  CLOUD_AMD_XA_WAVES 4, _WAVES_N64 0: dz, y; dx, out     0.996, 0.991; 3.13e-3       as A
    F  resident-weight forward y / row; partials err / bound  2.00e-3; 0.24               1e-2; 1

The transformed-operand bound is DERIVED, not measured: |got - ref| <= 2^-8 |ref| + 2^-21 S with
S = |A g| + |B z| + |D| (forward |z scale| + |shift| + |r|, for the shortcut BN |r rscale| +
|rshift| in place of |r|): at most three fp32 operations on terms of total magnitude S (each
<= 2^-24 S), then one bf16 rounding (half an ulp, 2^-8 2^e for |v| in [2^e, 2^(e+1)): up to
2^-8 |v| just above a power of two); XA_BN_RESBN_RELU adds 2^-8 |idn| for the shortcut
value the kernel rounds to bf16 before the add.  The observed 0.996 is that rounding at its worst
place, a value next to the first rounding midpoint of its binade, (1 + 2^-8) 2^e: 1 / (1 + 2^-8).
"""
import contextlib
import functools
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_resnet_kernel_edges_gpu as R  # noqa: E402  (metrics and bounds of the conv edge tests)

_row_err, _partials_err, _relu_bits, _say = R._row_err, R._partials_err, R._relu_bits, R._say
ROW_BOUND, WG32_BOUND, WGBF_BOUND, PART_BOUND = R.ROW_BOUND, R.WG32_BOUND, R.WGBF_BOUND, R.PART_BOUND

DEV = "cuda"
BF16 = torch.bfloat16
NT = 0
GUARD_ROWS = 128
# guard / pre-fill bit patterns: NaNs, so a value that is read instead of written also shows
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FA5A5A5),
            torch.uint8: (torch.uint8, 0xA5)}


def _ext():
    from cloud_amd.ops import _ext as e

    return e.load(required=True)


# ------------------------------------------------------------------------------- guarded outputs


class _Arena:
    """Output allocator: each tensor is the contiguous leading view of a flat allocation that
    carries GUARD_ROWS more rows; the whole allocation is filled with the SENTINEL pattern of its
    type (a NaN for bf16 / fp32), or the view with ``fill`` for tensors that are accumulated
    into.  ``check()`` asserts that every guard still holds the pattern, bit for bit."""

    def __init__(self, device=DEV):
        self.device, self.bufs = device, []

    def new(self, shape, dtype=BF16, fill=None, name="out"):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = math.prod(shape)
        row = n // shape[0] if len(shape) == 3 else (shape[-1] if len(shape) > 1 else 256)
        it, pat = SENTINEL[dtype]
        buf = torch.empty(n + GUARD_ROWS * row, dtype=dtype, device=self.device)
        buf.view(it).fill_(pat)
        view = buf[:n].view(shape)
        if fill is not None:
            view.copy_(fill.reshape(shape))
        self.bufs.append((buf, n, name))
        return view

    def owns(self, t):
        return any(buf.data_ptr() == t.data_ptr() for buf, _, _ in self.bufs)

    def check(self):
        for buf, n, name in self.bufs:
            it, pat = SENTINEL[buf.dtype]
            assert bool((buf[n:].view(it) == pat).all()), f"{name}: written past its last row"


class _TorchProxy:
    """``torch`` as cloud_amd.ops.raw sees it while a test runs: ``empty`` / ``empty_like`` (the
    dx, partials and workspace tensors the launchers allocate themselves) come from the arena."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, k):
        return getattr(torch, k)

    def empty(self, *shape, dtype=torch.float32, device=None):
        if len(shape) == 1 and not isinstance(shape[0], int):
            shape = tuple(shape[0])
        return self._arena.new(shape, dtype, name="raw-allocated")

    def empty_like(self, t):
        return self._arena.new(t.shape, t.dtype, name="raw-allocated")


@contextlib.contextmanager
def _guarded_raw(arena):
    from cloud_amd.ops import raw

    real = raw.torch
    raw.torch = _TorchProxy(arena)
    try:
        yield raw
    finally:
        raw.torch = real


def _is_sentinel(t):
    it, pat = SENTINEL[t.dtype]
    return t.contiguous().view(it) == pat


# ------------------------------------------------------------------------------- metrics


def _side_ratio(got, ref, S, extra=None):
    """Transformed operand per element: |got - ref| / (2^-8 |ref| + 2^-21 S [+ extra]), maximum
    (<= 1 passes; derived bound, see the module docstring).  Returns (ratio, absolute part)."""
    g = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), "unwritten or non-finite transformed elements"
    absolute = 2.0 ** -21 * S + (extra if extra is not None else 0.0)
    lim = 2.0 ** -8 * ref.abs() + absolute
    return ((g - ref).abs() / lim.clamp_min(1e-300)).max().item(), absolute


def _dw_err(got, ref):
    """Weight gradient per output-channel row of [Cout, Cin]: ||got - ref|| / max(||ref row||,
    median row norm), maximum over rows."""
    g = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), "unwritten or non-finite weight-gradient rows"
    n = ref.norm(dim=1)
    return ((g - ref).norm(dim=1) / torch.maximum(n, n.median())).max().item()


def _bf(t):
    return t.to(BF16).double()


# ------------------------------------------------------------------------------- operands


class _D(dict):
    __getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def _bwd_data(M, K, N):
    """Host operands of a backward case, dz [M, K] -> dx [M, N] (never modified): dy, z, the ReLU
    gate and [A | B | D] of the transform; w [K, N]; the epilogues' BN inputs, gates, residual
    source and accumulate-into tensor; the fused kernel's y and previous dW."""
    g = torch.Generator().manual_seed(7919 * M + 31 * K + N)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = _D(M=M, K=K, N=N)
    d.dy, d.z = rn(M, K).to(BF16), rn(M, K).to(BF16)
    d.keep = torch.rand(M, K, generator=g) > 0.4
    d.coef = torch.cat([rn(K), 0.3 * rn(K), rn(K)])  # full scale: see the module docstring
    d.w = (rn(K, N) / math.sqrt(K)).to(BF16)
    d.zb, d.z2 = (rn(M, N) * 2 + 0.5).to(BF16), rn(M, N).to(BF16)
    d.keep_b = torch.rand(M, N, generator=g) > 0.4
    d.src, d.old = rn(M, N).to(BF16), rn(M, N).to(BF16)
    d.keep_r = torch.rand(M, N, generator=g) > 0.5
    d.y = rn(M, N).to(BF16)
    d.prev = rn(K, N).to(BF16)
    return d


def _dz_ref(d, gated=True):
    """float64 dz = A * (dy * relu') + B * z + D of the bf16 operands, and S = sum |term|."""
    K = d.K
    A, B, D = (d.coef[i * K:(i + 1) * K].double() for i in range(3))
    g = d.dy.double() * (d.keep if gated else 1.0)
    return A * g + B * d.z.double() + D, (A * g).abs() + (B * d.z.double()).abs() + D.abs()


@functools.lru_cache(maxsize=None)
def _fwd_data(M, K, N):
    g = torch.Generator().manual_seed(104729 + 7919 * M + 31 * K + N)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = _D(M=M, K=K, N=N)
    d.z, d.r = rn(M, K).to(BF16), rn(M, K).to(BF16)
    # full scale: relu(shift) of a row past M is as large as a real activation
    d.ss = torch.cat([torch.rand(K, generator=g) + 0.5, 0.75 + 0.5 * rn(K)])
    d.rss = torch.cat([torch.rand(K, generator=g) + 0.5, 0.75 + 0.5 * rn(K)])
    d.w = (rn(N, K) / math.sqrt(K)).to(BF16)
    return d


def _v4(t, dev=DEV):
    return t.to(dev).view(1, 1, t.shape[0], -1)


# ------------------------------------------------------------------------------- dgrad epilogues

# name -> (beta, accumulate into `old`, BN statistics, its ReLU gate, second BN, residual, its gate)
EPILOGUES = {
    "plain": (0.0, False, False, False, False, False, False),
    "nomask": (0.0, False, False, False, False, False, False),  # plain, transform without a ReLU gate
    "beta1": (1.0, True, False, False, False, False, False),
    "bn": (0.0, False, True, True, False, False, False),
    "bn_nomask": (0.0, False, True, False, False, False, False),
    "res": (1.0, False, False, False, False, True, True),
    "res_nomask": (1.0, False, False, False, False, True, False),
    "res_bn": (1.0, False, True, True, False, True, True),
    "res2": (1.0, False, True, True, True, True, True),
}


def _epilogue(d, epi, arena, shape=None):
    """Launcher keywords of an epilogue and the float64 addend of its dx reference.  The output
    is pre-filled with NaN unless the epilogue accumulates into it; the residual-gated forms take
    beta 1 and never read it."""
    beta, acc, bn, bn_gate, bn2, res, res_gate = EPILOGUES[epi]
    shape = shape or (1, 1, d.M, d.N)
    dev = arena.device
    put = lambda t: t.to(dev).view(shape)  # noqa: E731
    kw = dict(out=arena.new(shape, fill=d.old if acc else None, name="dx"), beta=beta)
    add = d.old.double() if acc else 0.0
    if bn:
        kw["bn"] = (put(d.zb), _relu_bits(d.keep_b).to(dev) if bn_gate else None) + ((put(d.z2),) if bn2 else ())
    if res:
        kw["res"] = (put(d.src), _relu_bits(d.keep_r).to(dev) if res_gate else None)
        add = d.src.double() * (d.keep_r if res_gate else 1.0)
    return kw, add


def _check_dgrad(tag, r, d, epi, ref):
    """dx per row against ``ref`` [M, N]; the statistics partials against the STORED dx: [sum g |
    sum g z] with g = dx * relu'(bnmask), every partial row written.  Returns (row error,
    worst partials error / bound or None)."""
    _, _, bn, bn_gate, bn2, _, _ = EPILOGUES[epi]
    dx = r[0] if isinstance(r, tuple) else r
    e_dx, _ = _row_err(dx.reshape(-1, d.N), ref)
    e_st = None
    if bn:
        assert isinstance(r, tuple) and len(r) == (3 if bn2 else 2), "statistics partials missing"
        g = dx.double().cpu().reshape(-1, d.N) * (d.keep_b if bn_gate else 1.0)
        assert r[1].shape == ((d.M + 127) // 128, 2, d.N)
        e_st = _partials_err(r[1], g, g * d.zb.double())
        if bn2:
            e_st = max(e_st, _partials_err(r[2], g, g * d.z2.double()))
    _say(f"{tag} {epi}: dx/row {e_dx:.3e}" + ("" if e_st is None else f" partials err/bound {e_st:.3f}"))
    return e_dx, e_st


def _assert_dgrad(e_dx, e_st):
    assert e_dx < ROW_BOUND, e_dx
    assert e_st is None or e_st <= 1.0, e_st


# ------------------------------------------------------------------------------- A. stride 1

# (M, K = channels of A, N); routes by gemm.hip xa_launch with the default CLOUD_AMD_XA_N256 (3)
XA_CASES = [
    (1, 8, 8),          # smallest legal call; N <= 64 -> 128 x 64 8-wave, one K group, 127 rows past M
    (129, 72, 40),      # 128 x 64 8-wave tiles, K tail 8, N tail inside the tile, one row in the second M tile
    (127, 120, 64),     # 128 x 64 8-wave, a single short tile, K tail 56
    (129, 72, 136),     # 128 x 128 8-wave, N tail 8 in the second N tile (NN loader's P.N - 8 clamp; side by N tile 0)
    (257, 64, 256),     # N % 256 == 0, K <= XA_DEEP_KMAX -> 128 x 256 two-deep 16-wave form; one row in the third tile
    (130, 72, 512),     # two-deep form with a K tail and two N tiles
    (130, 2048, 256),   # two-deep form at K == XA_DEEP_KMAX
    (130, 2056, 256),   # K > XA_DEEP_KMAX -> 128 x 256 16-wave one-deep form, with a K tail
]
# (res2 = EPI_BF16_BNR2 always stays on the 128-wide tiles, 4-wave: its three statistics rows do
# not fit the wider forms' LDS image)
XA_BWD_EPIS = ["plain", "nomask", "beta1", "bn", "bn_nomask", "res", "res2"]
N256_CASES = [(257, 72, 256), (130, 2056, 256)]


def _xa_bwd(case, epi, tag="xa-bwd"):
    """raw.conv1x1_dgrad_bnbwd of one case and epilogue, held to float64.  Returns the figures and
    the outputs that must not depend on the tile form."""
    M, K, N = case
    d = _bwd_data(M, K, N)
    gated = epi != "nomask"
    dz, S = _dz_ref(d, gated)
    arena = _Arena()
    side = arena.new((1, 1, M, K), name="side")
    kw, add = _epilogue(d, epi, arena)
    with _guarded_raw(arena) as raw:
        r = raw.conv1x1_dgrad_bnbwd(_v4(d.dy), _v4(d.z), _relu_bits(d.keep).to(DEV) if gated else None,
                                    d.coef.to(DEV), d.w.to(DEV).view(K, 1, 1, N), side, **kw)
    torch.cuda.synchronize()
    arena.check()
    e_side, _ = _side_ratio(side, dz, S)
    _say(f"{tag} {case} {epi}: dz err/bound {e_side:.3f}")
    # the GEMM is judged on the kernel's own stored dz: that separates the transform from the GEMM
    e_dx, e_st = _check_dgrad(f"{tag} {case}", r, d, epi, side.double().cpu().view(M, K) @ d.w.double() + add)
    assert e_side <= 1.0, e_side
    _assert_dgrad(e_dx, e_st)
    return (e_side, e_dx, e_st), dict(side=side, dx=r[0] if isinstance(r, tuple) else r)


def _xa_fwd(case, mode, tag="xa-fwd"):
    """raw.conv1x1_fwd_bnapply (bn / res / resbn) with statistics, held to float64."""
    M, K, N = case
    d = _fwd_data(M, K, N)
    zd, rd = d.z.double(), d.r.double()
    scale, shift = d.ss[:K].double(), d.ss[K:].double()
    pre, S, extra = zd * scale + shift, (zd * scale).abs() + shift.abs(), None
    if mode == "res":
        pre, S = pre + rd, S + rd.abs()
    if mode == "resbn":
        rscale, rshift = d.rss[:K].double(), d.rss[K:].double()
        idn = rd * rscale + rshift
        pre, S, extra = pre + idn, S + (rd * rscale).abs() + rshift.abs(), 2.0 ** -8 * idn.abs()
    arena = _Arena()
    side = arena.new((1, 1, M, K), name="side")
    mask = arena.new((M, K // 8), torch.uint8, name="mask_out")
    stats = arena.new(((M + 127) // 128, 2, N), torch.float32, name="stats")
    with _guarded_raw(arena) as raw:
        out = raw.conv1x1_fwd_bnapply(_v4(d.z), d.ss.to(DEV), d.w.to(DEV).view(N, 1, 1, K), side, mask,
                                      res=_v4(d.r) if mode != "bn" else None,
                                      res_ss=d.rss.to(DEV) if mode == "resbn" else None, stats=stats)
    torch.cuda.synchronize()
    arena.check()
    assert arena.owns(out), "the launcher's own allocation must come from the guarded arena"
    e_side, absolute = _side_ratio(side, pre.clamp_min(0.0), S, extra)
    y = side.double().cpu().view(M, K)
    bit_ok = torch.equal(mask.cpu(), _relu_bits(y > 0))
    sure = pre.abs() > absolute
    sign_ok = bool(((y > 0) == (pre > 0))[sure].all())
    e_out, _ = _row_err(out.reshape(M, N), y @ d.w.double().t())
    od = out.double().cpu().view(M, N)
    e_st = _partials_err(stats, od, od * od)
    _say(f"{tag} {case} {mode}: y err/bound {e_side:.3f} out/row {e_out:.3e} partials err/bound {e_st:.3f} "
         f"({int((~sure).sum())} elements too close to zero to call)")
    assert e_side <= 1.0, e_side
    assert bit_ok, "the ReLU bitmask must mark exactly the stored positives"
    assert sign_ok, "the ReLU bitmask must agree with the float64 pre-activation's sign"
    assert e_out < ROW_BOUND and e_st <= 1.0, (e_out, e_st)
    return (e_side, e_out, e_st), dict(side=side, mask=mask, out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["bn", "res", "resbn"])
@pytest.mark.parametrize("case", XA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xa_forward_vs_fp64(case, mode):
    _xa_fwd(case, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", XA_BWD_EPIS)
@pytest.mark.parametrize("case", XA_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xa_backward_vs_fp64(case, epi):
    _xa_bwd(case, epi)


@pytest.mark.gpu
@pytest.mark.parametrize("case", N256_CASES, ids=lambda c: "x".join(map(str, c)))
def test_xa_tile_forms_bitwise(case):
    """gemm_set_xa_n256(0) (128 x 128 tiles) and (1) (128 x 256 16-wave one-deep) against the
    default form: dz, y, its bitmask, dx and the forward output bitwise equal; each run also
    passes the float64 criteria (the statistics partials regroup their fp32 sums with the tile
    width, so they are held to the partials criterion, not compared bitwise)."""
    ext = _ext()
    base = [_xa_bwd(case, "bn")[1], _xa_fwd(case, "res")[1], _xa_bwd(case, "res")[1]]
    for mode in (0, 1):
        prev = ext.gemm_set_xa_n256(mode)
        try:
            tag = f"[n256={mode}]"
            got = [_xa_bwd(case, "bn", "xa-bwd" + tag)[1], _xa_fwd(case, "res", "xa-fwd" + tag)[1],
                   _xa_bwd(case, "res", "xa-bwd" + tag)[1]]
        finally:
            ext.gemm_set_xa_n256(prev)
        for a, b in zip(got, base):
            for k in b:
                assert torch.equal(a[k], b[k]), (mode, k)


# ------------------------------------------------------------------------------- B. strided shortcut

# (N, H, W, s, Cd, Cin)
STRIDED_CASES = [
    (1, 1, 1, 2, 8, 8),          # one pixel
    (3, 7, 10, 2, 72, 40),       # M = 3 * 4 * 5 = 60, a single short tile; 128 x 64 route
    (5, 9, 13, 2, 128, 256),     # M = 5 * 5 * 7 = 175, image carries inside a tile; 128 x 256 two-deep route + row map
    (2, 7, 11, 3, 64, 64),       # stride 3: M = 2 * 3 * 4 = 24
]
DENSE_PAIR_CASES = [(3, 7, 10, 2, 72, 40), (2, 7, 11, 3, 64, 64)]
C1 = 72  # channels of the stride-1 gradient accumulated on top


@functools.lru_cache(maxsize=None)
def _acc_data(N, H, W, Cin):
    g = torch.Generator().manual_seed(50021 + 1000 * N + 100 * H + 10 * W + Cin)
    M = N * H * W
    d = _D(M=M, N=Cin)
    d.dz1 = torch.randn(M, C1, generator=g).to(BF16)
    d.w1 = (torch.randn(C1, Cin, generator=g) / math.sqrt(C1)).to(BF16)
    d.zb = (torch.randn(M, Cin, generator=g) * 2 + 0.5).to(BF16)
    d.keep_b = torch.rand(M, Cin, generator=g) > 0.4
    return d


def _class_mask(N, H, W, s):
    """[N, H, W] bool: the pixels of the one non-empty output-parity class."""
    live = torch.zeros(N, H, W, dtype=torch.bool)
    live[:, ::s, ::s] = True
    return live


def _check_sparse(tag, dx, strided_ref, live):
    """After the strided call: the written pixels per row, the sentinel everywhere else."""
    Cin = dx.shape[-1]
    e, _ = _row_err(dx.cpu()[live], strided_ref)
    untouched = bool(_is_sentinel(dx).cpu().view(*live.shape, Cin)[~live].all())
    _say(f"{tag}: written pixels dx/row {e:.3e}, {int((~live).sum())} other pixels untouched: {untouched}")
    assert e < ROW_BOUND, e
    assert untouched, "pixels outside the written parity class must keep the sentinel bit pattern"


def _accumulate(tag, raw, dx, strided_ref, live, case, with_bn):
    """raw.conv_dgrad(..., beta=1, beta_stride=s) into the sparse tensor: the whole dx finite, per
    row against the float64 sum, partials against the stored dx."""
    N, H, W, s, Cd, Cin = case
    a = _acc_data(N, H, W, Cin)
    bn = (a.zb.to(DEV).view(N, H, W, Cin), _relu_bits(a.keep_b).to(DEV)) if with_bn else None
    r = raw.conv_dgrad(a.dz1.to(DEV).view(N, H, W, C1), a.w1.to(DEV).view(C1, 1, 1, Cin), (N, H, W, Cin), 1, 0,
                       out=dx, beta=1.0, bn=bn, beta_stride=s)
    torch.cuda.synchronize()
    ref = (a.dz1.double() @ a.w1.double()).view(N, H, W, Cin)
    ref[live] += strided_ref
    return _check_dgrad(tag, r, a, "bn" if with_bn else "plain", ref.view(-1, Cin))


@pytest.mark.gpu
@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("case", STRIDED_CASES, ids=lambda c: "x".join(map(str, c)))
def test_strided_shortcut_then_sparse_accumulate(case, with_bn):
    """raw.conv1x1_strided_dgrad_bnbwd on rectangles (a swapped Hq / Wq pair of the row map
    shows), then the stride-1 accumulate that reads the unwritten pixels as zeros (a swapped
    par_h / par_w pair of ca_dgrad_gemm shows)."""
    N, H, W, s, Cd, Cin = case
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    M = N * Ho * Wo
    d = _bwd_data(M, Cd, Cin)
    dz, S = _dz_ref(d)
    live = _class_mask(N, H, W, s)
    arena = _Arena()
    side = arena.new((N, Ho, Wo, Cd), name="side")
    with _guarded_raw(arena) as raw:
        dx = raw.conv1x1_strided_dgrad_bnbwd(d.dy.to(DEV).view(N, Ho, Wo, Cd), d.z.to(DEV).view(N, Ho, Wo, Cd),
                                             _relu_bits(d.keep).to(DEV), d.coef.to(DEV),
                                             d.w.to(DEV).view(Cd, 1, 1, Cin), side, (N, H, W, Cin), s)
        torch.cuda.synchronize()
        assert arena.owns(dx), "the launcher's own allocation must come from the guarded arena"
        e_side, _ = _side_ratio(side, dz, S)
        tag = f"strided {case}"
        _say(f"{tag}: dz err/bound {e_side:.3f}")
        assert e_side <= 1.0, e_side
        strided_ref = side.double().cpu().view(M, Cd) @ d.w.double()
        _check_sparse(tag, dx, strided_ref, live)
        e_dx, e_st = _accumulate(tag + " accumulate", raw, dx, strided_ref, live, case, with_bn)
    arena.check()
    _assert_dgrad(e_dx, e_st)


@pytest.mark.gpu
@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn"])
@pytest.mark.parametrize("case", DENSE_PAIR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_skip_empty_dgrad_then_sparse_accumulate(case, with_bn):
    """The pair without the fold: conv_dgrad(..., skip_empty=True) of a strided 1x1 (its operand
    is the bf16 dz of a separate BN backward) + the beta_stride accumulate, on rectangles."""
    N, H, W, s, Cd, Cin = case
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    M = N * Ho * Wo
    d = _bwd_data(M, Cd, Cin)
    live = _class_mask(N, H, W, s)
    arena = _Arena()
    dx = arena.new((N, H, W, Cin), name="dx")
    with _guarded_raw(arena) as raw:
        raw.conv_dgrad(d.dy.to(DEV).view(N, Ho, Wo, Cd), d.w.to(DEV).view(Cd, 1, 1, Cin), (N, H, W, Cin), s, 0, out=dx,
                       skip_empty=True)
        torch.cuda.synchronize()
        strided_ref = d.dy.double() @ d.w.double()
        tag = f"skip-empty {case}"
        _check_sparse(tag, dx, strided_ref, live)
        e_dx, e_st = _accumulate(tag + " accumulate", raw, dx, strided_ref, live, case, with_bn)
    arena.check()
    _assert_dgrad(e_dx, e_st)


# ------------------------------------------------------------------------------- C. dense 1x1 dgrad

DENSE_CASES = [(1, 1, 1, 8, 8), (2, 5, 13, 72, 40), (3, 9, 5, 64, 136)]  # (N, H, W, Cout, Cin)
DENSE_EPIS = ["res_nomask", "res", "res_bn", "res2", "bn_nomask", "beta1"]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", DENSE_EPIS)
@pytest.mark.parametrize("case", DENSE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_dense_dgrad_epilogues_vs_fp64(case, epi):
    """ca_dgrad_gemm / the plain and BN-statistics NN GEMM through raw.conv_dgrad of a 1x1
    convolution: the residual-gated beta with and without its mask, with one and two BNs, the
    statistics without a ReLU gate, and a plain accumulate."""
    N, H, W, Cout, Cin = case
    M = N * H * W
    d = _bwd_data(M, Cout, Cin)
    arena = _Arena()
    kw, add = _epilogue(d, epi, arena, (N, H, W, Cin))
    with _guarded_raw(arena) as raw:
        r = raw.conv_dgrad(d.dy.to(DEV).view(N, H, W, Cout), d.w.to(DEV).view(Cout, 1, 1, Cin), (N, H, W, Cin), 1, 0,
                           **kw)
    torch.cuda.synchronize()
    arena.check()
    _assert_dgrad(*_check_dgrad(f"dense-dgrad {case}", r, d, epi, d.dy.double() @ d.w.double() + add))


# ------------------------------------------------------------------------------- D. fused dx + dW

FUSED_SHAPES = [(64, 64), (128, 64), (256, 64), (64, 256), (512, 128)]  # every fusable (Cout, Cin)
# (M, blocks): one row; one row in the second tile; 5 tiles with the default grid (one tile per
# workgroup), ONE workgroup walking every tile (prefetch across tile boundaries), and 4 asked ->
# 2 tiles per workgroup -> 3 workgroups, fewer than the slab workspace was sized for
FUSED_GRIDS = [(1, None), (129, None), (520, None), (520, 1), (520, 4)]
# (256, 64) with beta 0 ("plain", "bn", "bn_nomask") runs the deep-stream kernel
# (mfma_gemm_xa_dw_deep) by default, its other epilogues and every other shape the one-step form
FUSED_EPIS = ["plain", "beta1", "bn", "bn_nomask"]
FUSED_EPIS_K64 = ["res", "res2"]  # Cout == 64 only (the one-K-step instantiations)
FUSED = [(co, ci, m, b, e) for co, ci in FUSED_SHAPES for m, b in FUSED_GRIDS
         for e in FUSED_EPIS + (FUSED_EPIS_K64 if co == 64 else [])]


def _fused(Cout, Cin, M, blocks, epi, dw_dtype, tag="fused"):
    """raw.conv1x1_dgrad_wgrad_bnbwd: dz is never written, so dx and dW are held to the float64
    dz rounded to bf16.  dW into fp32 with dw_beta 0 over NaN, or into a pre-filled bf16 tensor
    with dw_beta 1."""
    d = _bwd_data(M, Cout, Cin)
    dz = _bf(_dz_ref(d)[0])
    arena = _Arena()
    kw, add = _epilogue(d, epi, arena)
    into_bf = dw_dtype == BF16
    dw = arena.new((Cout, 1, 1, Cin), dw_dtype, fill=d.prev if into_bf else None, name="dw")
    with _guarded_raw(arena) as raw:
        r = raw.conv1x1_dgrad_wgrad_bnbwd(_v4(d.dy), _v4(d.z), _relu_bits(d.keep).to(DEV), d.coef.to(DEV),
                                          d.w.to(DEV).view(Cout, 1, 1, Cin), _v4(d.y), dw,
                                          dw_beta=1.0 if into_bf else 0.0, blocks=blocks, **kw)
    torch.cuda.synchronize()
    arena.check()
    tag = f"{tag} ({Cout}, {Cin}) M={M} blocks={blocks} dw={'bf16+=' if into_bf else 'fp32='}"
    e_dx, e_st = _check_dgrad(tag, r, d, epi, dz @ d.w.double() + add)
    e_dw = _dw_err(dw.view(Cout, Cin), dz.t() @ d.y.double() + (d.prev.double() if into_bf else 0.0))
    _say(f"{tag} {epi}: dw/row {e_dw:.3e}")
    _assert_dgrad(e_dx, e_st)
    assert e_dw < (WGBF_BOUND if into_bf else WG32_BOUND), e_dw
    return e_dx, e_st, e_dw


@pytest.mark.gpu
@pytest.mark.parametrize("dw_dtype", [torch.float32, BF16], ids=["dw_fp32_beta0", "dw_bf16_beta1"])
@pytest.mark.parametrize("Cout,Cin,M,blocks,epi", FUSED, ids=lambda v: str(v))
def test_fused_dgrad_wgrad_vs_fp64(Cout, Cin, M, blocks, epi, dw_dtype):
    _fused(Cout, Cin, M, blocks, epi, dw_dtype)


# ------------------------------------------------------------------------------- E. forms chosen once per process


def _child_fused(tag):
    """The stage-1 conv3 shape at 5 tiles, deep-form epilogues, every grid and dW type."""
    for M, blocks in FUSED_GRIDS[2:]:
        for epi in ("bn", "plain"):
            for dt in (torch.float32, BF16):
                _fused(256, 64, M, blocks, epi, dt, tag)


def _child_waves(tag):
    for case in ((129, 72, 40), (129, 72, 136)):
        for mode in ("bn", "res", "resbn"):
            _xa_fwd(case, mode, "xa-fwd" + tag)
        for epi in XA_BWD_EPIS:
            _xa_bwd(case, epi, "xa-bwd" + tag)


_CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_bn_fold_edges_gpu as T
T.{fn}({tag!r})
print("BN_FOLD_EDGES_OK")
"""
_child_failed = []

FORMS = [
    ("CLOUD_AMD_XA_DW_DEPTH", "0", "_child_fused"),   # the one-step form at K = 256 -> N = 64
    ("CLOUD_AMD_XA_DW_DEPTH", "2", "_child_fused"),   # deep form, two / four source steps in flight,
    ("CLOUD_AMD_XA_DW_DEPTH", "4", "_child_fused"),   # one workgroup per CU
    ("CLOUD_AMD_XA_DW_WAVES", "8", "_child_fused"),   # one-step form on one 8-wave workgroup per CU
    ("CLOUD_AMD_XA_WAVES", "4", "_child_waves"),      # 4-wave 128 x 64 and 128 x 128 tiles
    ("CLOUD_AMD_XA_WAVES_N64", "0", "_child_waves"),  # 4-wave 128 x 64, 8-wave 128 x 128
]


@pytest.mark.gpu
@pytest.mark.parametrize("var,value,fn", FORMS, ids=[f"{v}={x}" for v, x, _ in FORMS])
def test_forms_chosen_once_per_process(var, value, fn):
    """Switches read once per process: each value runs in its own interpreter, one after the
    other, against the same references and bounds; none is started after one has failed."""
    assert not _child_failed, f"not started: the child for {_child_failed[0]} failed"
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env[var] = value
    code = _CHILD.format(root=os.path.dirname(tests), tests=tests, fn=fn, tag=f"[{var}={value}]")
    _child_failed.append(f"{var}={value}")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110)
    print(r.stdout)
    assert r.returncode == 0 and "BN_FOLD_EDGES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    _child_failed.pop()


# ------------------------------------------------------------------------------- F. resident-weight forward

# (M, N, K, stats)
PRW_CASES = [(m, 256, 64, st) for m in (128, 129, 401) for st in (False, True)] + [(1029, 512, 128, True),
                                                                                  (1029, 1024, 256, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,stats", PRW_CASES)
def test_resident_weight_forward_vs_fp64(M, N, K, stats):
    """ext.gemm_bf16 (NT) on the shapes the persistent resident-weight core covers, with the
    statistics partials of ext.gemm_stat_rows rows.  Which core runs depends on the CU count; the
    criteria hold on either."""
    from cloud_amd.ops import _ext as E
    from cloud_amd.ops import raw

    ext = _ext()
    g = torch.Generator().manual_seed(15485863 + 7919 * M + 31 * K + N)
    a = torch.randn(M, K, generator=g).to(BF16)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(BF16)
    arena = _Arena()
    y = arena.new((M, N), name="y")
    rows = ext.gemm_stat_rows(M, N, K, K, K, N)
    st = arena.new((rows, 2, N), torch.float32, name="stats") if stats else None
    ad, wd = a.to(DEV), w.to(DEV)
    ext.gemm_bf16(NT, ad.data_ptr(), K, wd.data_ptr(), K, y.data_ptr(), N, M, N, K, E.ptr(st), 0.0,
                  E.stream_handle(ad.device))
    torch.cuda.synchronize()
    arena.check()
    e_y, _ = _row_err(y, a.double() @ w.double().t())
    yd = y.double().cpu()
    e_st = _partials_err(st, yd, yd * yd) if stats else None
    _say(f"prw M={M} N={N} K={K}: resident-weight core {raw.uses_prw(M, N, K)} ({rows} partial rows) y/row {e_y:.3e}"
         + (f" partials err/bound {e_st:.3f}" if stats else ""))
    _assert_dgrad(e_y, e_st)


# ------------------------------------------------------------------------------- host-only controls
# (no GPU: they show that the criteria above reject one deliberate defect each and accept the
# bf16-rounded float64 reference)


def test_control_one_wrong_row_of_520():
    d = _bwd_data(520, 64, 64)
    ref = _bf(_dz_ref(d)[0]) @ d.w.double()
    good = ref.to(BF16)
    assert _row_err(good, ref)[0] < ROW_BOUND
    bad = good.clone()
    bad[300] = (ref[300] * 1.05).to(BF16)
    whole = ((bad.double() - ref).norm() / ref.norm()).item()
    assert whole < 5e-3, whole  # a whole-tensor norm check at 2e-2 does not see it
    assert _row_err(bad, ref)[0] > ROW_BOUND


def test_control_last_k_group_dropped():
    d = _bwd_data(129, 72, 40)
    dz = _bf(_dz_ref(d)[0])
    ref, dw = dz @ d.w.double(), dz.t() @ d.y.double()
    assert _row_err(ref.to(BF16), ref)[0] < ROW_BOUND
    assert _dw_err(dw.float(), dw) < WG32_BOUND and _dw_err(dw.to(BF16), dw) < WGBF_BOUND
    assert _row_err((dz[:, :64] @ d.w.double()[:64]).to(BF16), ref)[0] > ROW_BOUND
    short = dw.clone()
    short[64:] = 0
    assert _dw_err(short.float(), dw) > WGBF_BOUND


def test_control_tail_rows_leak_into_statistics():
    """The rows between M and the tile end transform to D (backward) / relu(shift) (forward); their
    product with the weights added to the partials must trip the partials criterion."""
    M = 129
    d = _bwd_data(M, 72, 40)
    K = d.K
    dx = (_bf(_dz_ref(d)[0]) @ d.w.double()).to(BF16).double()
    g = dx * d.keep_b
    terms = (g, g * d.zb.double())
    good = torch.stack([t.sum(0) for t in terms]).float()[None]
    assert _partials_err(good, *terms) <= 1.0
    leak = (_bf(d.coef[2 * K:].double()) @ d.w.double()).to(BF16).double() * (256 - M)
    assert _partials_err(good + torch.stack([leak, torch.zeros_like(leak)]).float()[None], *terms) > 1.0

    f = _fwd_data(M, 72, 40)
    y = _bf(torch.relu(f.z.double() * f.ss[:72].double() + f.ss[72:].double()))
    out = (y @ f.w.double().t()).to(BF16).double()
    terms = (out, out * out)
    good = torch.stack([t.sum(0) for t in terms]).float()[None]
    assert _partials_err(good, *terms) <= 1.0
    row = (_bf(torch.relu(f.ss[72:].double())) @ f.w.double().t()).to(BF16).double()
    leak = torch.stack([row, row * row]) * (256 - M)
    assert _partials_err(good + leak.float()[None], *terms) > 1.0


def test_control_h_w_swapped_in_sparse_accumulate():
    N, H, W, s, Cd, Cin = 3, 7, 10, 2, 72, 40
    a = _acc_data(N, H, W, Cin)
    d = _bwd_data(N * 4 * 5, Cd, Cin)
    strided = (_bf(_dz_ref(d)[0]) @ d.w.double()).to(BF16).double()
    sparse = torch.zeros(N, H, W, Cin, dtype=torch.float64)
    live = _class_mask(N, H, W, s)
    sparse[live] = strided
    base = a.dz1.double() @ a.w1.double()
    ref = base + sparse.view(-1, Cin)
    assert _row_err(ref.to(BF16), ref)[0] < ROW_BOUND
    # the accumulate's row -> pixel map with H and W exchanged: row m is taken for pixel
    # (m // H % W, m % H), so other rows' old values are read and the written ones dropped
    m = torch.arange(N * H * W)
    taken = ((m // H) % W % s == 0) & (m % H % s == 0)
    bad = base + sparse.view(-1, Cin) * taken[:, None]
    assert not torch.equal(taken, live.view(-1))
    assert _row_err(bad.to(BF16), ref)[0] > ROW_BOUND


def test_control_guard_row_overwritten():
    arena = _Arena("cpu")
    dx = arena.new((1, 1, 129, 40), name="dx")
    part = arena.new((2, 2, 40), torch.float32, name="partials")
    mask = arena.new((129, 5), torch.uint8, name="mask")
    dx.zero_(), part.zero_(), mask.zero_()
    arena.check()
    for t, buf in ((dx, 0), (part, 1), (mask, 2)):
        flat = arena.bufs[buf][0]
        keep = flat[t.numel():t.numel() + 8].clone()
        flat[t.numel():t.numel() + 8] = 0  # the first 8 elements of row M
        with pytest.raises(AssertionError):
            arena.check()
        flat[t.numel():t.numel() + 8] = keep
    arena.check()
