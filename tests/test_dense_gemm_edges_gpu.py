"""Edge-case reference tests for the dense GEMM family (csrc/kernels/gemm.hip: ca_gemm_ex,
ca_gemm_bf16, ca_gemm_splitk, ca_splitk_reduce, ca_splitk_bias_act; csrc/kernels/gradfin.hip:
ca_grad_finalize_multi; csrc/kernels/rowops.hip: ca_colsum and the Keras Dense glue pad_cols /
pad_cols_multi / slice_acc / act_grad), called through the ``ext.*`` bindings directly.

Every reference is float64 on the host, computed from exactly the bf16 / fp32 operands the kernel
reads; inputs come from a host ``torch.Generator`` with a fixed seed per case.  The metrics, bounds
and guards are those of test_resnet_kernel_edges_gpu.py and test_bn_fold_edges_gpu.py; nothing
here is tuned to a run.

    group  what                                   criterion (origin)
    A B D  bf16 GEMM outputs, preact              _row_err per row AND per column < ROW_BOUND 1e-2
                                                  (project constant; the column pass makes a defect
                                                  confined to one 8-column group visible at large N)
    A D    statistics partials of gemm_ex         _partials_err against the STORED output <= 1
                                                  (PART_BOUND 2^-20 * sum |term|, project constant)
    C D    fp32 slabs and fp32 weight gradients   per element <= PART_BOUND * sum_k |a_k b_k| (+ |old|);
                                                  _dw_err per row < WG32_BOUND 2e-3; bf16: < WGBF_BOUND 2e-2
    E F    pure reductions on integer inputs      torch.equal with the float64 sum (derived: every
                                                  partial sum is an integer below 2^24, <= 256 where
                                                  the output is bf16, so any summation order is exact)
    E F    the same on non-integer inputs         per element <= PART_BOUND * sum |term| (+ 2^-8 |ref|
                                                  for the one bf16 rounding)
    F      splitk_bias_act with an activation     per element <= 2^-8 |ref| + 2^-21 (|sum| + |bias|)
    G      pad_cols / pad_cols_multi              bit-identical block, exact zeros
    G      slice_acc, act_grad                    exact on integers; 2^-8 |ref| + 2^-20 |term| otherwise
    all    unwritten / overwritten memory         NaN pre-fill, 128 guard rows (_Arena), columns
                                                  N .. ld-1 keep the sentinel bit for bit
    all    determinism                            every launch repeated once: identical bits; deferred
                                                  finalisation (grad_finalize_multi) = immediate path

Each GEMM case names the branch of dispatch<> / launch<> it is there for; ``_route`` mirrors
want_small_n / use_256 / use_256x96 and only asserts that the case still takes that branch (if a
change of the heuristics moves a case, the assertion says which shape to re-pick).

Worst figures observed on an MI355X (each test prints its figures with ``[edges]`` before
asserting):

    group                                                       worst observed                  bound
    A  NT 128 core: out / row, / column; preact; partials       3.73e-3, 4.95e-3; 2.16e-3; 0.24  1e-2, 1e-2; 1e-2; 1
    B  NN 128 core: dx / row, / column                          3.60e-3, 6.88e-3                1e-2, 1e-2
    C  TN split-K: slab, dW element err / bound                 0.089, 0.089 (beta 1: 0.088)    1
    C  TN split-K: dW per row fp32; bf16                        2.21e-7; 2.20e-3                2e-3; 2e-2
    D  core 6 (256 x 256): out / row, / column; preact          3.11e-3, 3.21e-3; 1.98e-3       1e-2, 1e-2; 1e-2
    D  core 6: partials; slab err / bound; dW fp32; bf16        0.29; 0.096; 1.46e-7; 1.86e-3   1; 1; 2e-3; 2e-2
    D  core 0 (register-staged): out / row, / column; partials  3.73e-3, 3.07e-3; 0.14          1e-2, 1e-2; 1
    D  core 0: slab err / bound; dW fp32; bf16                  0.084; 1.32e-7; 1.97e-3         1; 2e-3; 2e-2
    D  256 x 96 tiles: out / row, / column; preact              2.65e-3, 3.23e-3; 1.87e-3       1e-2, 1e-2; 1e-2
    E  splitk_reduce / grad_finalize_multi, integer inputs      0 elements differ               exact
    E  splitk_reduce non-integer err / bound: fp32; bf16        0.18; 0.994                     1
    E  fin_cols non-integer err / bound                         0.075                           1
    F  colsum integer; non-integer err / bound                  exact; 0.004                    exact; 1
    F  splitk_bias_act: integer sum; activation; non-integer    exact; 0.994; 0.990             exact; 1; 1
    G  pad_cols, slice_acc on integers; slice_acc, act_grad     exact; 0.982, 0.986             exact; 1
    fix 1  gemm_bf16 beta 1, N 256 / K 64: row, column; parts   2.54e-3, 2.66e-3; 0.25          1e-2, 1e-2; 1

The figures next to 1 in E - G are the one bf16 rounding of the result at its worst place (a value
next to the first rounding midpoint of its binade, 1 / (1 + 2^-8)), as in the BN-fold edge tests.
On the commit before the resident-weight fix the beta = 1 cases of "fix 1" fail with 0.76 - 0.82
per row and column: the result is A * B alone (2e-3 from it), the accumulate silently dropped.
"""
import functools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bn_fold_edges_gpu as B  # noqa: E402  (guarded outputs of the BN-fold edge tests)
import test_resnet_kernel_edges_gpu as R  # noqa: E402  (metrics and bounds of the conv edge tests)

_row_err, _partials_err, _say = R._row_err, R._partials_err, R._say
ROW_BOUND, WG32_BOUND, WGBF_BOUND, PART_BOUND = R.ROW_BOUND, R.WG32_BOUND, R.WGBF_BOUND, R.PART_BOUND
_Arena, _is_sentinel, _dw_err, _bf = B._Arena, B._is_sentinel, B._dw_err, B._bf
SENTINEL = B.SENTINEL

DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32
NT, NN, TN = 0, 1, 2
ACT = {"none": 0, "gelu": 1, "relu": 2, "tanh": 3, "gelu_tanh": 4, "elu": 5}
ACTS = ["gelu", "relu", "tanh", "gelu_tanh", "elu"]
_C0 = 0.7978845608028654


def _ext():
    from cloud_amd.ops import _ext as e

    return e.load(required=True)


def _st():
    from cloud_amd.ops import _ext as e

    return e.stream_handle(torch.device(DEV, torch.cuda.current_device()))


def _p(t):
    return 0 if t is None else t.data_ptr()


class _D(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _cdiv(a, b):
    return -(-a // b)


def _bits(t):
    return t.contiguous().view(SENTINEL[t.dtype][0])


def _same(a, b):
    return (a is None and b is None) or torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------- activations


def _act64(name, x):
    if name == "gelu":
        return x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if name == "relu":
        return x.clamp_min(0.0)
    if name == "tanh":
        return torch.tanh(x)
    if name == "gelu_tanh":
        return 0.5 * x * (1.0 + torch.tanh(_C0 * (x + 0.044715 * x ** 3)))
    if name == "elu":
        return torch.where(x > 0, x, torch.expm1(x))
    return x


def _dact64(name, x):
    """d act / dx of the pre-activation x (the GEMM epilogue's dact_src form)."""
    if name == "gelu":
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if name == "relu":
        return (x > 0).double()
    if name == "tanh":
        return 1.0 - torch.tanh(x) ** 2
    if name == "gelu_tanh":
        t = torch.tanh(_C0 * (x + 0.044715 * x ** 3))
        return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _C0 * (1.0 + 3.0 * 0.044715 * x * x)
    if name == "elu":
        return torch.where(x > 0, torch.ones_like(x), torch.exp(x))
    return torch.ones_like(x)


# ------------------------------------------------------------------------------- dispatch mirror


def _balance(t):
    return t / (_cdiv(t, 256) * 256)


def _small_n(M, N, splits=1):
    tm = _cdiv(M, 128)
    t128, t64 = tm * _cdiv(N, 128) * splits, tm * _cdiv(N, 64) * splits
    return N <= 64 or (_balance(t128) < 0.8 and _balance(t64) > _balance(t128) + 0.1)


def _use_256(core, M, N, kps, splits):
    if core == 6:
        return M >= 256 and N >= 256
    if core != 5 or M < 256 or N < 256 or kps < 512:
        return False
    t = _cdiv(M, 256) * _cdiv(N, 256) * splits
    if splits > 1 and 224 <= t <= 256:
        return True
    return t >= 256 and (_balance(t) >= 0.999 or (t >= 512 and _balance(t) >= 0.85))


def _use_256x96(M, N, splits, stats):
    if splits != 1 or N % 96 or M < 4096 or stats:
        return False
    t96, t128 = _cdiv(M, 256) * (N // 96), _cdiv(M, 128) * _cdiv(N, 128)
    return t96 >= 512 and _balance(t96) >= 0.999 and _balance(t128) < 0.95


def _route(core, layout, M, N, K, splits=1, kps=None, stats=False):
    """Tile form gemm.hip dispatch<> / launch<> picks (CLOUD_AMD_* switches at their defaults)."""
    kps = kps or K
    bm = 64 if layout == TN and M <= 64 else 128
    bn = 64 if _small_n(M, N, splits) else 128
    if bm == 128 and bn == 128:
        if _use_256(core, M, N, kps, splits):
            return "256x256"
        if layout == NT and splits == 1 and core != 0 and _use_256x96(M, N, splits, stats):
            return "256x96"
    if core == 0:
        return f"reg{bm}x{bn}/{1 if kps <= 64 else 2}"
    return f"{bm}x{bn}"


def _reduce_form(MN):
    n4 = MN // 4
    return "cb4" if n4 < 8192 else ("cb16" if n4 < 32768 else "cols")


def _kps(K, splits):
    return max(64, _cdiv(K // splits, 64) * 64)


@pytest.fixture
def core():
    """Select a GEMM core for one test; the previous one comes back afterwards."""
    ext = _ext()
    prev = ext.gemm_set_core(-1)
    yield ext.gemm_set_core
    ext.gemm_set_core(prev)


# ------------------------------------------------------------------------------- operands

EDGE_ROWS = {"all": None, "edges": list(range(0, 256)) + list(range(7936, 8000))}


@functools.lru_cache(maxsize=None)
def _gemm_data(layout, M, N, K, rows="all"):
    """Host operands of an NT / NN case (never modified): a [M, K], w ([N, K] or [K, N]), bias,
    the accumulate-into tensor, the act' source, and the float64 product on the reference rows."""
    g = torch.Generator().manual_seed(2750159 + 1000003 * layout + 7919 * M + 31 * N + K)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = _D(layout=layout, M=M, N=N, K=K)
    d.a = rn(M, K).to(BF16)
    d.w = (rn(N, K) / math.sqrt(K)).to(BF16) if layout == NT else (rn(K, N) / math.sqrt(K)).to(BF16)
    d.bias = rn(N)  # full scale: as large as the product itself
    d.old = rn(M, N).to(BF16)
    d.src = (1.5 * rn(M, N + 8)).to(BF16)  # act' source with ld_aux = N + 8 (its pad is garbage, not zero)
    d.sel = None if EDGE_ROWS[rows] is None else torch.tensor(EDGE_ROWS[rows])
    a = d.a if d.sel is None else d.a[d.sel]
    d.acc = a.double() @ (d.w.double().t() if layout == NT else d.w.double())
    return d


def _sel(d, t):
    return t if d.sel is None else t[d.sel.to(t.device)]


def _wide(a, ld, seed):
    """a as the column slice [:, 8 : 8 + K] of a random [M, ld] matrix."""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(a.shape[0], ld, generator=g).to(BF16)
    wide[:, 8:8 + a.shape[1]] = a
    return wide


def _ref_fwd(d, bias, act, beta):
    """float64, unrounded: act(acc + bias) + beta * old; and the pre-activation."""
    pre = d.acc + (d.bias.double() if bias else 0.0)
    return _act64(act, pre) + (beta * _sel(d, d.old).double() if beta else 0.0), pre


def _emu_fwd(d, bias, act, beta):
    """The same rounded to bf16 at the kernel's own rounding points (gemm_epilogue): acc + bias
    (the staged value, what preact stores), its activation, the beta add.  Controls only."""
    pre = _bf(d.acc + (d.bias.double() if bias else 0.0))
    y = _bf(_act64(act, pre)) if act != "none" else pre
    return (_bf(y + beta * _sel(d, d.old).double()) if beta else y), pre


def _ref_bwd(d, dact, beta):
    src = _sel(d, d.src)[:, :d.N].double()
    return d.acc * (_dact64(dact, src) if dact else 1.0) + (beta * _sel(d, d.old).double() if beta else 0.0)


def _both_err(got, ref):
    """(_row_err per row, _row_err per column)."""
    return _row_err(got, ref)[0], _row_err(got.t(), ref.t())[0]


def _whole_err(got, ref):
    return ((got.double() - ref).norm() / ref.norm()).item()


# ------------------------------------------------------------------------------- gemm_ex runner

# name -> keywords of _run_ex
FWD_EPIS = {
    "plain": {},
    "bias": dict(bias=True),
    **{f"bias_{a}_preact": dict(bias=True, act=a, preact=True) for a in ACTS},
    "beta1": dict(beta=1.0),
    "bias_relu_beta1": dict(bias=True, act="relu", beta=1.0),
    "stats": dict(stats=True),
    "stats_relu": dict(stats=True, act="relu"),
    "stats_beta1": dict(stats=True, beta=1.0),
    "ldc_pad": dict(ldc_pad=16),
    "a_slice": dict(lda_pad=24),
}
BWD_EPIS = {
    "plain": {},
    **{f"dact_{a}": dict(dact=a) for a in ACTS},
    "dact_gelu_beta1": dict(dact="gelu", beta=1.0),
    "a_slice": dict(lda_pad=8),
}


def _run_ex(tag, d, bias=False, act="none", preact=False, dact=None, beta=0.0, stats=False, ldc_pad=0, lda_pad=0):
    """ext.gemm_ex of one case and epilogue, launched twice (identical bits), held to float64."""
    ext, layout, M, N, K = _ext(), d.layout, d.M, d.N, d.K
    ldc, ld_aux = N + ldc_pad, N + 8

    def launch():
        arena = _Arena()
        if lda_pad:
            ad = _wide(d.a, K + lda_pad, 17 * M + K).to(DEV)
            a_ptr, lda = ad[:, 8:].data_ptr(), K + lda_pad
        else:
            ad = d.a.to(DEV)
            a_ptr, lda = ad.data_ptr(), K
        wd = d.w.to(DEV)
        c = arena.new((M, ldc), name="C")
        if beta:
            c[:, :N] = d.old.to(DEV)
        pre = arena.new((M, ld_aux), name="preact") if preact else None
        src = d.src.to(DEV) if dact else None
        st = arena.new((_cdiv(M, 128), 2, N), F32, name="stats") if stats else None
        bd = d.bias.to(DEV) if bias else None
        ext.gemm_ex(layout, a_ptr, lda, wd.data_ptr(), wd.stride(0), c.data_ptr(), ldc, M, N, K, _p(st), float(beta),
                    _p(bd), ACT[dact or act], _p(pre), _p(src), ld_aux if (preact or dact) else 0, _st())
        torch.cuda.synchronize()
        arena.check()
        return dict(c=c, pre=pre, st=st)

    o, again = launch(), launch()
    for k in o:
        assert _same(o[k], again[k]), f"{tag}: {k} differs between two identical launches"
    c, pre, st = o["c"], o["pre"], o["st"]
    assert bool(_is_sentinel(c[:, N:]).all()), "columns N .. ldc-1 must keep the sentinel"
    assert bool(torch.isfinite(c[:, :N]).all()), "unwritten output elements"
    if layout == NT:
        ref, pre_ref = _ref_fwd(d, bias, act, beta)
    else:
        ref, pre_ref = _ref_bwd(d, dact, beta), None
    got = _sel(d, c)[:, :N]
    e_r, e_c = _both_err(got, ref)
    e_p = e_st = None
    if preact:
        assert bool(_is_sentinel(pre[:, N:]).all()), "preact columns N .. ld_aux-1 must keep the sentinel"
        e_p = max(_both_err(_sel(d, pre)[:, :N], pre_ref))
    if stats:
        y = c[:, :N].double().cpu()
        e_st = _partials_err(st, y, y * y)
    _say(f"{tag}: out/row {e_r:.3e} out/col {e_c:.3e}" + ("" if e_p is None else f" preact {e_p:.3e}")
         + ("" if e_st is None else f" partials err/bound {e_st:.3f}"))
    assert e_r < ROW_BOUND and e_c < ROW_BOUND, (e_r, e_c)
    assert e_p is None or e_p < ROW_BOUND, e_p
    assert e_st is None or e_st <= 1.0, e_st
    return e_r, e_c, e_p, e_st


def _ids(c):
    return "x".join(map(str, c[:3])) + ("" if len(c) < 4 else "-" + "-".join(map(str, c[3:])))


# ------------------------------------------------------------------------------- A. forward NT, 128 core

# (M, N, K, branch of dispatch<> / launch<> on the default core)
NT_CASES = [
    (1, 8, 8, "128x64"),        # smallest legal call: 127 absent rows, 120 absent columns, one partial MFMA K step
    (129, 72, 200, "128x128"),  # second M tile of one row; 56 absent columns; K = 3 tiles + 8
    (127, 64, 64, "128x64"),    # N <= 64; M one short of a tile
    (128, 136, 72, "128x128"),  # exact M; second column tile one chunk wide; K = 64 + 8
    (300, 264, 40, "128x128"),  # 32 < K < 64: second MFMA step partly zero
    (600, 840, 72, "128x64"),   # want_small_n's balance branch at N > 64 (35 vs 70 tiles); last tile has 8 columns
]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", list(FWD_EPIS))
@pytest.mark.parametrize("case", NT_CASES, ids=_ids)
def test_nt_forward_vs_fp64(case, epi, core):
    M, N, K, route = case
    core(5)
    kw = FWD_EPIS[epi]
    assert _route(5, NT, M, N, K, stats=kw.get("stats", False)) == route, "re-pick this shape for its branch"
    _run_ex(f"A nt {M}x{N}x{K} [{route}] {epi}", _gemm_data(NT, M, N, K), **kw)


# ------------------------------------------------------------------------------- B. input gradient NN

NN_CASES = [(129, 72, 200, "128x128"), (1, 8, 8, "128x64"), (300, 264, 136, "128x128"), (600, 840, 72, "128x64")]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", list(BWD_EPIS))
@pytest.mark.parametrize("case", NN_CASES, ids=_ids)
def test_nn_input_gradient_vs_fp64(case, epi, core):
    M, N, K, route = case
    core(5)
    assert _route(5, NN, M, N, K) == route, "re-pick this shape for its branch"
    _run_ex(f"B nn {M}x{N}x{K} [{route}] {epi}", _gemm_data(NN, M, N, K), **BWD_EPIS[epi])


# ------------------------------------------------------------------------------- C. weight gradient TN


@functools.lru_cache(maxsize=None)
def _tn_data(M, N, K):
    """a [K, M], b [K, N] (K = reduction rows), previous fp32 / bf16 gradients."""
    g = torch.Generator().manual_seed(32452843 + 7919 * M + 31 * N + K)
    d = _D(M=M, N=N, K=K)
    d.a = torch.randn(K, M, generator=g).to(BF16)
    d.b = (torch.randn(K, N, generator=g) / math.sqrt(K)).to(BF16)
    d.old32 = torch.randn(M, N, generator=g)
    d.oldbf = torch.randn(M, N, generator=g).to(BF16)
    return d


def _fin_job(kind, src, nparts, stride, n, out0, out1=None, out2=None, out_bf16=0, accumulate=0):
    return [kind, _p(src), nparts, stride, n, _p(out0), _p(out1), _p(out2), int(out_bf16), int(accumulate), 0, 0]


def _run_tn(tag, M, N, K, splits, route, core_kind=5):
    ext = _ext()
    d = _tn_data(M, N, K)
    kps = _kps(K, splits)
    eff = ext.gemm_splitk_effective(K, splits)
    assert eff == _cdiv(K, kps), (eff, kps)
    assert _route(core_kind, TN, M, N, K, eff, kps) == route, "re-pick this shape for its branch"
    ad, bd = d.a.to(DEV), d.b.to(DEV)
    a64, b64 = d.a.double(), d.b.double()
    slab_ref = torch.stack([a64[s * kps:(s + 1) * kps].t() @ b64[s * kps:(s + 1) * kps] for s in range(eff)])
    slab_abs = torch.stack([a64[s * kps:(s + 1) * kps].abs().t() @ b64[s * kps:(s + 1) * kps].abs()
                            for s in range(eff)])
    ref, S = slab_ref.sum(0), slab_abs.sum(0)

    def launch(out_dtype, beta, mode):
        arena = _Arena()
        ws = arena.new((eff, M, N), F32, name="slabs")
        old = None if not beta else (d.old32 if out_dtype == F32 else d.oldbf)
        out = arena.new((M, N), out_dtype, fill=old, name="dW")
        ext.gemm_splitk(TN, ad.data_ptr(), M, bd.data_ptr(), N, 0 if mode < 0 else out.data_ptr(),
                        mode if mode < 0 else int(out_dtype == BF16), float(beta), M, N, K, splits, ws.data_ptr(),
                        _st())
        torch.cuda.synchronize()
        arena.check()
        assert bool(torch.isfinite(ws).all()), "a slab element was not written"
        if mode < 0:
            assert bool(_is_sentinel(out).all()) if not beta else torch.equal(out.cpu(), old)
            ext.grad_finalize_multi(_fin_job(0, ws, eff, M * N, M * N, out, out_bf16=out_dtype == BF16), [float(beta)],
                                    _st())
            torch.cuda.synchronize()
            arena.check()
        return ws, out

    ws, o32 = launch(F32, 0.0, 0)
    ws2, o32_again = launch(F32, 0.0, 0)
    assert _same(ws, ws2) and _same(o32, o32_again), "two identical launches differ"
    e_slab = ((ws.double().cpu() - slab_ref).abs() / (PART_BOUND * slab_abs).clamp_min(1e-300)).max().item()
    e_el = ((o32.double().cpu() - ref).abs() / (PART_BOUND * S).clamp_min(1e-300)).max().item()
    e_32 = _dw_err(o32, ref)
    _, o32b = launch(F32, 1.0, 0)
    ref_b = ref + d.old32.double()
    e_elb = ((o32b.double().cpu() - ref_b).abs() / (PART_BOUND * (S + d.old32.double().abs()))).max().item()
    e_32b = _dw_err(o32b, ref_b)
    _, obf = launch(BF16, 1.0, 0)
    e_bf = _dw_err(obf, ref + d.oldbf.double())
    _, d32 = launch(F32, 0.0, -1)
    _, dbf = launch(BF16, 1.0, -1)
    _say(f"{tag} [{route}] splits {splits} -> {eff}: slab err/bound {e_slab:.3f} dW fp32 element err/bound {e_el:.3f} "
         f"(beta 1: {e_elb:.3f}) per row {e_32:.3e} / {e_32b:.3e}, bf16 {e_bf:.3e}")
    assert e_slab <= 1.0 and e_el <= 1.0 and e_elb <= 1.0, (e_slab, e_el, e_elb)
    assert e_32 < WG32_BOUND and e_32b < WG32_BOUND and e_bf < WGBF_BOUND, (e_32, e_32b, e_bf)
    assert _same(d32, o32) and _same(dbf, obf), "deferred finalisation must equal the immediate path bit for bit"
    return e_slab, e_32, e_bf


# (M, N, K = reduction rows, requested splits, branch)
TN_CASES = [(40, 136, 1000, s, "64x128") for s in (1, 3, 4)] + [(64, 72, 100, s, "64x128") for s in (1, 3, 4)] + [
    (96, 264, 1000, 3, "128x128"),  # k_per_split 384, last split 232 = 3 tiles + 40
    (136, 72, 77, 2, "128x128"),    # reduction length not a multiple of 8 (rows are K here: legal)
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", TN_CASES, ids=_ids)
def test_tn_weight_gradient_vs_fp64(case, core):
    M, N, K, splits, route = case
    core(5)
    if (M, N, K, splits) == (64, 72, 100, 4):
        assert _ext().gemm_splitk_effective(K, splits) == 2  # 64 / 36
    _run_tn(f"C tn {M}x{N}x{K}", M, N, K, splits, route)


# ------------------------------------------------------------------------------- D. the other cores

CORE6_CASES = [(264, 264, 72), (520, 264, 200), (300, 264, 136)]
CORE6_FWD = ["plain", "bias_gelu_preact", "beta1", "stats_relu"]


@pytest.mark.gpu
@pytest.mark.parametrize("epi", CORE6_FWD + ["nn_dact_gelu_beta1"])
@pytest.mark.parametrize("case", CORE6_CASES, ids=_ids)
def test_core6_256x256_vs_fp64(case, epi, core):
    M, N, K = case
    core(6)
    layout = NN if epi.startswith("nn_") else NT
    kw = BWD_EPIS[epi[3:]] if layout == NN else FWD_EPIS[epi]
    assert _route(6, layout, M, N, K, stats=kw.get("stats", False)) == "256x256"
    _run_ex(f"D core6 {'nn' if layout == NN else 'nt'} {M}x{N}x{K} {epi}", _gemm_data(layout, M, N, K), **kw)


@pytest.mark.gpu
def test_core6_256x256_weight_gradient(core):
    core(6)
    _run_tn("D core6 tn 264x520x1000", 264, 520, 1000, 2, "256x256", core_kind=6)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", ["plain", "bias_gelu_preact", "beta1", "stats_relu", "a_slice"])
@pytest.mark.parametrize("case", [(129, 72, 200, "reg128x128/2"), (129, 72, 64, "reg128x128/1")], ids=_ids)
def test_core0_register_staged_vs_fp64(case, epi, core):
    M, N, K, route = case
    core(0)
    assert _route(0, NT, M, N, K) == route
    _run_ex(f"D core0 nt {M}x{N}x{K} [{route}] {epi}", _gemm_data(NT, M, N, K), **FWD_EPIS[epi])


@pytest.mark.gpu
def test_core0_register_staged_weight_gradient(core):
    core(0)
    _run_tn("D core0 tn 40x136x1000", 40, 136, 1000, 3, "reg64x128/2", core_kind=0)


@pytest.mark.gpu
@pytest.mark.parametrize("epi", ["plain", "bias_gelu_preact", "beta1"])
def test_256x96_tiles_vs_fp64(epi, core):
    """(8000, 2304, 136): the smallest grid that passes use_256x96 (768 tiles against 1134), with a
    64-row M tail and an 8-element K tail; the only place the non-FIXCOL epilogue runs.  The whole
    output goes through the NaN / guard checks on the device, the float64 reference covers rows
    [0, 256) and [7936, 8000)."""
    M, N, K = 8000, 2304, 136
    core(5)
    assert _route(5, NT, M, N, K) == "256x96"
    assert _route(5, NT, M - 256 * 2, N, K) != "256x96"  # one tile row fewer no longer fills whole rounds
    _run_ex(f"D 256x96 nt {M}x{N}x{K} {epi}", _gemm_data(NT, M, N, K, "edges"), **FWD_EPIS[epi])


# ------------------------------------------------------------------------------- E. splitk_reduce, grad_finalize_multi

# element counts on both sides of the form boundaries (n4 = MN / 4: < 8192 CB = 4, < 32768 CB = 16,
# else the column kernel)
REDUCE_MN = [(4, "cb4"), (4 * (4 * 7 + 1), "cb4"), (4 * 8191, "cb4"), (4 * 8192, "cb16"), (4 * (16 * 600 + 1), "cb16"),
             (4 * 32767, "cb16"), (4 * 32768, "cols"), (4 * 32768 + 4, "cols")]
# the unroll tail of the column kernel, the second trip of the 16 slab-lanes at CB = 16 (17) and
# of the 64 slab-lanes at CB = 4 (65)
REDUCE_S = [1, 2, 5, 17, 65]


@functools.lru_cache(maxsize=4)
def _int_slabs(MN, S):
    g = torch.Generator().manual_seed(49979687 + 131 * MN + S)
    return torch.randint(-2, 3, (S, MN), generator=g).float(), torch.randint(-64, 65, (MN,), generator=g).float()


def _reduce(ext, wsd, S, MN, dtype, beta, old):
    arena = _Arena()
    out = arena.new((MN,), dtype, fill=old.to(dtype) if beta else None, name="reduced")
    ext.splitk_reduce(wsd.data_ptr(), S, MN, out.data_ptr(), int(dtype == BF16), float(beta), _st())
    torch.cuda.synchronize()
    arena.check()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", REDUCE_S)
@pytest.mark.parametrize("MN,form", REDUCE_MN)
def test_splitk_reduce_exact(MN, form, S):
    """Integer slabs in {-2 .. 2}, old values integers of magnitude <= 64: |sum| <= 2 * 65 + 64 = 194,
    exact in fp32 and in bf16 in any order."""
    assert _reduce_form(MN) == form
    ext = _ext()
    ws, old = _int_slabs(MN, S)
    wsd = ws.to(DEV)
    total = ws.double().sum(0)
    for dtype in (F32, BF16):
        for beta in (0.0, 1.0):
            got = _reduce(ext, wsd, S, MN, dtype, beta, old)
            assert _same(got, _reduce(ext, wsd, S, MN, dtype, beta, old))
            ref = total + beta * old.double()
            bad = int((got.double().cpu() != ref).sum())
            _say(f"E reduce MN={MN} [{form}] S={S} {dtype} beta={beta}: {bad} elements differ")
            assert torch.equal(got.double().cpu(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("MN,form", [(4 * 29, "cb4"), (4 * (16 * 600 + 1), "cb16"), (4 * 32768 + 4, "cols")])
def test_splitk_reduce_noninteger(MN, form):
    assert _reduce_form(MN) == form
    ext, S = _ext(), 17
    g = torch.Generator().manual_seed(86028121 + MN)
    ws, old = torch.randn(S, MN, generator=g), torch.randn(MN, generator=g).to(BF16)
    wsd = ws.to(DEV)
    for dtype in (F32, BF16):
        out = _reduce(ext, wsd, S, MN, dtype, 1.0, old.float())
        assert _same(out, _reduce(ext, wsd, S, MN, dtype, 1.0, old.float()))
        arena = _Arena()
        fin = arena.new((MN,), dtype, fill=old.float(), name="finalized")  # fin_splitk / fin_splitk_cols
        ext.grad_finalize_multi(_fin_job(0, wsd, S, MN, MN, fin, out_bf16=dtype == BF16), [1.0], _st())
        torch.cuda.synchronize()
        arena.check()
        assert _same(fin, out), "grad_finalize_multi must equal splitk_reduce bit for bit"
        got = out.double().cpu()
        ref = ws.double().sum(0) + old.double()
        lim = PART_BOUND * (ws.double().abs().sum(0) + old.double().abs())
        lim = lim + (2.0 ** -8 * ref.abs() if dtype == BF16 else 0.0)
        e = ((got - ref).abs() / lim).max().item()
        _say(f"E reduce non-integer MN={MN} [{form}] {dtype}: err/bound {e:.3f}")
        assert e <= 1.0, e


@pytest.mark.gpu
def test_splitk_reduce_refuses_mn_not_multiple_of_4():
    ext = _ext()
    arena = _Arena()
    ws = torch.ones(2, 8, device=DEV)
    out = arena.new((8,), F32)
    with pytest.raises(RuntimeError):
        ext.splitk_reduce(ws.data_ptr(), 2, 6, out.data_ptr(), 0, 0.0, _st())
    with pytest.raises(RuntimeError):
        ext.grad_finalize_multi(_fin_job(0, ws, 2, 6, 6, out), [0.0], _st())
    torch.cuda.synchronize()
    assert bool(_is_sentinel(out).all())
    arena.check()


def _cols_case(ext, arena, nparts, N, mode, accumulate, seed, pad=8):
    """One kind-1 job: integer partials [nparts][3 N + pad] (row stride larger than the columns
    used), outputs by ``mode`` (0: out0, 1: out0 + out1, 2: all three, 3: out0, null, out2).
    Returns (job row, outputs, float64 references)."""
    g = torch.Generator().manual_seed(67867979 + seed)
    stride = 3 * N + pad
    part = torch.randint(-2, 3, (nparts, stride), generator=g).float()
    live = [(True, False, False), (True, True, False), (True, True, True), (True, False, True)][mode]
    outs, refs = [], []
    for k in range(3):
        if not live[k]:
            outs.append(None)
            refs.append(None)
            continue
        old = torch.randint(-64, 65, (N,), generator=g).float()
        outs.append(arena.new((N,), F32, fill=old if accumulate else None, name=f"out{k}"))
        refs.append(part[:, k * N:(k + 1) * N].double().sum(0) + (old.double() if accumulate else 0.0))
    pd = part.to(DEV)
    return _fin_job(1, pd, nparts, stride, N, outs[0], outs[1], outs[2], accumulate=accumulate), outs, refs, pd


def _check_outs(tag, outs, refs):
    for k, (o, r) in enumerate(zip(outs, refs)):
        if o is not None:
            assert torch.equal(o.double().cpu(), r), f"{tag}: out{k}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["out0", "out0+1", "out0+1+2", "out0+null+2"])
@pytest.mark.parametrize("N", [8, 24, 264])
def test_fin_cols_exact(N, mode):
    """fin_cols: N = 24 puts out0's last 8 and out1's first 8 columns in one 16-column block."""
    ext = _ext()
    for nparts in (1, 16, 17, 256):
        for accumulate in (0, 1):
            arena = _Arena()
            job, outs, refs, keep = _cols_case(ext, arena, nparts, N, mode, accumulate, 1000 * N + 10 * nparts + mode)
            ext.grad_finalize_multi(job, [0.0], _st())
            torch.cuda.synchronize()
            arena.check()
            _check_outs(f"N={N} nparts={nparts} acc={accumulate}", outs, refs)
    _say(f"E fin_cols N={N} mode={mode}: exact for nparts 1 / 16 / 17 / 256, accumulate 0 / 1")


@pytest.mark.gpu
@pytest.mark.parametrize("nparts,N", [(17, 24), (256, 264)])
def test_fin_cols_noninteger(nparts, N):
    ext = _ext()
    g = torch.Generator().manual_seed(217645177 + nparts)
    part, old = torch.randn(nparts, 3 * N + 8, generator=g), torch.randn(3, N, generator=g)
    pd = part.to(DEV)
    got = []
    for _ in range(2):
        arena = _Arena()
        outs = [arena.new((N,), F32, fill=old[k], name=f"out{k}") for k in range(3)]
        ext.grad_finalize_multi(_fin_job(1, pd, nparts, 3 * N + 8, N, *outs, accumulate=1), [0.0], _st())
        torch.cuda.synchronize()
        arena.check()
        got.append(outs)
    worst = 0.0
    for k in range(3):
        assert _same(got[0][k], got[1][k])
        terms = part[:, k * N:(k + 1) * N].double()
        lim = PART_BOUND * (terms.abs().sum(0) + old[k].double().abs())
        worst = max(worst, ((got[0][k].double().cpu() - terms.sum(0) - old[k].double()).abs() / lim).max().item())
    _say(f"E fin_cols non-integer nparts={nparts} N={N}: err/bound {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.gpu
@pytest.mark.parametrize("njobs", [1, 8, 11])
def test_grad_finalize_multi_job_lists(njobs):
    """Kind 0 in all three forms mixed with kind 1; 11 jobs = two launches (FIN_MAX = 8).  Every job
    is exact and equals its standalone launch bit for bit."""
    ext = _ext()
    kinds = [("k0", 4 * 29, 5, F32, 0.0), ("k1", 17, 24, 2, 1), ("k0", 4 * (16 * 600 + 1), 17, BF16, 1.0),
             ("k1", 256, 264, 3, 0), ("k0", 4 * 32768 + 4, 5, F32, 1.0), ("k1", 1, 8, 0, 1),
             ("k0", 4 * 8192, 65, BF16, 0.0), ("k1", 16, 24, 1, 0), ("k0", 4, 2, F32, 1.0), ("k1", 17, 264, 2, 1),
             ("k0", 4 * 8191, 65, F32, 0.0)][:njobs]
    arena, solo = _Arena(), _Arena()
    jobs, betas, checks, keep = [], [], [], []
    for i, k in enumerate(kinds):
        if k[0] == "k0":
            _, MN, S, dtype, beta = k
            ws, old = _int_slabs(MN, S)
            wsd = ws.to(DEV)
            out = arena.new((MN,), dtype, fill=old.to(dtype) if beta else None, name=f"job{i}")
            jobs += _fin_job(0, wsd, S, MN, MN, out, out_bf16=dtype == BF16)
            betas.append(beta)
            alone = _reduce(ext, wsd, S, MN, dtype, beta, old)
            checks.append(([out], [ws.double().sum(0) + beta * old.double()], [alone]))
            keep.append(wsd)
        else:
            _, nparts, N, mode, acc = k
            job, outs, refs, pd = _cols_case(ext, arena, nparts, N, mode, acc, 7 * i)
            jobs += job
            betas.append(0.0)
            job1, outs1, _, pd1 = _cols_case(ext, solo, nparts, N, mode, acc, 7 * i)
            ext.grad_finalize_multi(job1, [0.0], _st())
            checks.append((outs, refs, outs1))
            keep += [pd, pd1]
    ext.grad_finalize_multi(jobs, betas, _st())
    torch.cuda.synchronize()
    arena.check()
    solo.check()
    for i, (outs, refs, alone) in enumerate(checks):
        _check_outs(f"job {i} of {njobs}", outs, refs)
        for o, a in zip(outs, alone):
            assert _same(o, a), f"job {i}: differs from its standalone launch"
    _say(f"E grad_finalize_multi {njobs} jobs: exact, bitwise the standalone launches")


# ------------------------------------------------------------------------------- F. colsum, splitk_bias_act


def _colsum_rows(M):
    return min(max((M + 63) // 64, 1), 256)  # raw.colsum_into's mirror of ca_colsum's partial rows


@functools.lru_cache(maxsize=None)
def _colsum_data(M, N):
    g = torch.Generator().manual_seed(15485867 + 31 * M + N)
    x = torch.randint(-1, 2, (M, N + 8), generator=g).to(BF16)  # ld = N + 8; the pad is live data too
    return x, torch.randint(-64, 65, (N,), generator=g).float()


# M = 1 and 64: the one-launch path; 65: two partial rows; 16384: exactly the 256-part cap; 16449:
# past it, the grid-stride loop takes a second trip.  N = 264 needs a second column block.
@pytest.mark.gpu
@pytest.mark.parametrize("N", [8, 264])
@pytest.mark.parametrize("M", [1, 64, 65, 16384, 16449])
def test_colsum_exact(M, N):
    from cloud_amd.ops import raw

    ext = _ext()
    x, old = _colsum_data(M, N)
    xd = x.to(DEV)
    ref = x[:, :N].double().sum(0)  # |sum| <= 16449 < 2^24: exact in any order
    nws = ext.colsum_workspace_floats(M, N)
    assert nws >= _colsum_rows(M) * N
    got = {}
    for acc in (0, 1, -1):
        arena = _Arena()
        ws = arena.new((nws // N, N), F32, name="colsum workspace")
        out = arena.new((N,), F32, fill=old if acc == 1 else None, name="colsum")
        ext.colsum(xd.data_ptr(), M, N, N + 8, out.data_ptr(), acc, ws.data_ptr(), _st())
        torch.cuda.synchronize()
        arena.check()
        if acc >= 0:
            assert torch.equal(out.double().cpu(), ref + (old.double() if acc else 0.0)), f"accumulate={acc}"
            got[acc] = out
            continue
        # partials only: exactly the rows the Python mirror counts are written, the output is not
        ry = _colsum_rows(M)
        assert bool(_is_sentinel(out).all())
        assert bool(torch.isfinite(ws[:ry]).all()) and bool(_is_sentinel(ws[ry:]).all()), "partial-row count"
        assert torch.equal(ws[:ry].double().sum(0).cpu(), ref)
        for a in (0, 1):  # consumed by grad_finalize_multi's kind 1: bitwise the immediate path
            fin = arena.new((N,), F32, fill=old if a else None, name="finalized")
            ext.grad_finalize_multi(_fin_job(1, ws, ry, N, N, fin, accumulate=a), [0.0], _st())
            torch.cuda.synchronize()
            arena.check()
            assert _same(fin, got[a])
    # raw.colsum_into under deferred finalisation sizes its job with the same mirror
    xs = xd[:, :N]
    imm = raw.colsum_into(xs, old.to(DEV).clone(), accumulate=True)
    dfr = old.to(DEV).clone()
    with raw.deferred_finalize():
        raw.colsum_into(xs, dfr, accumulate=True)
    torch.cuda.synchronize()
    assert torch.equal(imm.double().cpu(), ref + old.double()) and _same(imm, dfr)
    _say(f"F colsum M={M} N={N}: exact for accumulate 0 / 1 / -1, {_colsum_rows(M)} partial rows")


@pytest.mark.gpu
def test_colsum_noninteger():
    ext, M, N = _ext(), 16449, 264
    g = torch.Generator().manual_seed(982451653)
    x = torch.randn(M, N + 8, generator=g).to(BF16)
    arena = _Arena()
    ws = arena.new((256, N), F32)
    out = arena.new((N,), F32)
    xd = x.to(DEV)
    ext.colsum(xd.data_ptr(), M, N, N + 8, out.data_ptr(), 0, ws.data_ptr(), _st())
    torch.cuda.synchronize()
    arena.check()
    xx = x[:, :N].double()
    e = ((out.double().cpu() - xx.sum(0)).abs() / (PART_BOUND * xx.abs().sum(0))).max().item()
    _say(f"F colsum non-integer M={M} N={N}: err/bound {e:.3f}")
    assert e <= 1.0, e


@functools.lru_cache(maxsize=None)
def _sba_data(M, N, S):
    g = torch.Generator().manual_seed(179424673 + 1000 * M + 10 * N + S)
    return (torch.randint(-2, 3, (S, M, N), generator=g).float(), torch.randn(N, generator=g),
            torch.randint(-3, 4, (N,), generator=g).float())


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("M,N", [(1, 8), (37, 64), (5, 12), (33, 1000)])
def test_splitk_bias_act(M, N, S):
    """Integer slabs: the sum is exact; with an integer bias and no activation the bf16 result is
    too (|sum + bias| <= 9).  With an activation: act(sum + bias) per element within 2^-8 |ref|
    (the bf16 rounding) + 2^-21 (|sum| + |bias|) (the fp32 add and activation)."""
    ext = _ext()
    ws, bias, ibias = _sba_data(M, N, S)
    wsd = ws.to(DEV)
    total = ws.double().sum(0)
    worst = 0.0
    for b in (None, ibias, bias):
        for act in ACT:
            bd = None if b is None else b.to(DEV)
            outs = []
            for _ in range(2):
                arena = _Arena()
                out = arena.new((M, N), name="splitk_bias_act")
                ext.splitk_bias_act(wsd.data_ptr(), S, M, N, _p(bd), ACT[act], out.data_ptr(), _st())
                torch.cuda.synchronize()
                arena.check()
                outs.append(out)
            assert _same(outs[0], outs[1])
            got = outs[0].double().cpu()
            assert torch.isfinite(got).all()
            bb = torch.zeros(N, dtype=torch.float64) if b is None else b.double()
            if act == "none" and b is not bias:
                assert torch.equal(got, total + bb), "the pure reduction must be exact"
            ref = _act64(act, total + bb)
            lim = 2.0 ** -8 * ref.abs() + 2.0 ** -21 * (total.abs() + bb.abs())
            err = (got - ref).abs()
            assert (err[lim == 0] == 0).all()
            worst = max(worst, (err / lim.clamp_min(1e-300)).max().item())
    _say(f"F splitk_bias_act M={M} N={N} S={S}: exact without activation; worst err/bound {worst:.3f}")
    assert worst <= 1.0, worst


@pytest.mark.gpu
def test_splitk_bias_act_noninteger():
    """Non-integer slabs and bias, no activation: PART_BOUND * sum |term| + the bf16 rounding."""
    ext, M, N, S = _ext(), 33, 1000, 3
    g = torch.Generator().manual_seed(472882027)
    ws, bias = torch.randn(S, M, N, generator=g), torch.randn(N, generator=g)
    wsd, bd = ws.to(DEV), bias.to(DEV)
    arena = _Arena()
    out = arena.new((M, N), name="splitk_bias_act")
    ext.splitk_bias_act(wsd.data_ptr(), S, M, N, bd.data_ptr(), 0, out.data_ptr(), _st())
    torch.cuda.synchronize()
    arena.check()
    ref = ws.double().sum(0) + bias.double()
    lim = PART_BOUND * (ws.double().abs().sum(0) + bias.double().abs()) + 2.0 ** -8 * ref.abs()
    e = ((out.double().cpu() - ref).abs() / lim).max().item()
    _say(f"F splitk_bias_act non-integer M={M} N={N} S={S}: err/bound {e:.3f}")
    assert e <= 1.0, e


@pytest.mark.gpu
def test_splitk_bias_act_refuses_n_not_multiple_of_4():
    ext = _ext()
    arena = _Arena()
    ws = torch.ones(2, 4, 16, device=DEV)
    out = arena.new((4, 16))
    with pytest.raises(RuntimeError):
        ext.splitk_bias_act(ws.data_ptr(), 2, 4, 10, 0, 0, out.data_ptr(), _st())
    torch.cuda.synchronize()
    assert bool(_is_sentinel(out).all())
    arena.check()


# ------------------------------------------------------------------------------- G. Keras glue


def _pad_case(arena, rows, cols, ld, rows_out, cols_out, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    src = torch.randn(rows, ld, generator=g).to(dtype).to(DEV)
    out = arena.new((rows_out, cols_out), dtype, name="padded")
    return src, out, [src.data_ptr(), ld, cols, out.data_ptr(), cols_out, rows, rows_out, 2 if dtype == BF16 else 4]


def _check_pad(src, out, rows, cols):
    assert _same(out[:rows, :cols], src[:, :cols]), "the kept block must be bit-identical"
    z = _bits(out).clone()
    z[:rows, :cols] = 0
    assert bool((z == 0).all()), "added rows and columns must be exactly zero"


# (rows, cols, ld, rows_out, cols_out)
PAD_CASES = [(5, 3, 3, 5, 8), (7, 10, 24, 16, 16), (1, 1, 9, 8, 8), (300, 13, 16, 304, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["2byte", "4byte"])
@pytest.mark.parametrize("case", PAD_CASES, ids=_ids)
def test_pad_cols(case, dtype):
    ext = _ext()
    rows, cols, ld, rows_out, cols_out = case
    arena = _Arena()
    src, out, job = _pad_case(arena, rows, cols, ld, rows_out, cols_out, dtype, 31 * rows + cols)
    ext.pad_cols(job[0], ld, cols, job[3], cols_out, rows, rows_out, job[7], _st())
    torch.cuda.synchronize()
    arena.check()
    _check_pad(src, out, rows, cols)
    for bad in ((cols_out + 1, cols_out, rows, rows_out, job[7]), (cols, cols_out, rows_out + 1, rows_out, job[7]),
                (cols, cols_out, rows, rows_out, 3)):
        fresh = arena.new((rows_out, cols_out), dtype)
        with pytest.raises(RuntimeError):
            ext.pad_cols(job[0], ld, bad[0], fresh.data_ptr(), bad[1], bad[2], bad[3], bad[4], _st())
        torch.cuda.synchronize()
        assert bool(_is_sentinel(fresh).all())


@pytest.mark.gpu
@pytest.mark.parametrize("njobs", [1, 2, 3, 4])
def test_pad_cols_multi(njobs):
    ext = _ext()
    arena = _Arena()
    made, jobs = [], []
    for k in range(njobs):
        rows, cols, ld, rows_out, cols_out = PAD_CASES[k]
        src, out, job = _pad_case(arena, rows, cols, ld, rows_out, cols_out, BF16 if k % 2 == 0 else F32, 97 + k)
        made.append((src, out, rows, cols))
        jobs += job
    ext.pad_cols_multi(jobs, _st())
    torch.cuda.synchronize()
    arena.check()
    for m in made:
        _check_pad(*m)


@pytest.mark.gpu
def test_pad_cols_multi_refuses_0_and_5_jobs():
    ext = _ext()
    arena = _Arena()
    jobs = []
    for k in range(5):
        jobs += _pad_case(arena, 5, 3, 3, 5, 8, BF16, k)[2]
    for bad in ([], jobs):
        with pytest.raises(RuntimeError):
            ext.pad_cols_multi(bad, _st())
    torch.cuda.synchronize()
    arena.check()
    for buf, n, _ in arena.bufs:
        assert bool(_is_sentinel(buf[:n]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("rows,cols,ld", [(1, 3, 8), (37, 10, 16), (300, 13, 13)])
def test_slice_acc(rows, cols, ld, dtype):
    """Integer gradient block accumulated into integer old values (|sum| <= 72: exact, also in
    bf16); then a non-integer block within one rounding of its sink."""
    ext = _ext()
    g = torch.Generator().manual_seed(104723 + 100 * rows + cols)
    for exact in (True, False):
        src = (torch.randint(-8, 9, (rows + 3, ld), generator=g).float() if exact
               else torch.randn(rows + 3, ld, generator=g))
        old = (torch.randint(-64, 65, (rows, cols), generator=g).float() if exact
               else torch.randn(rows, cols, generator=g)).to(dtype)
        arena = _Arena()
        out = arena.new((rows, cols), dtype, fill=old, name="sink")
        sd = src.to(DEV)
        ext.slice_acc(sd.data_ptr(), ld, out.data_ptr(), int(dtype == BF16), rows, cols, _st())
        torch.cuda.synchronize()
        arena.check()
        ref = old.double() + src[:rows, :cols].double()
        got = out.double().cpu()
        if exact:
            assert torch.equal(got, ref)
        else:
            lim = (2.0 ** -8 if dtype == BF16 else 2.0 ** -23) * ref.abs() + 2.0 ** -23 * (old.double().abs()
                                                                                          + src[:rows, :cols].abs())
            e = ((got - ref).abs() / lim).max().item()
            _say(f"G slice_acc {rows}x{cols} ld {ld} {dtype}: err/bound {e:.3f}")
            assert e <= 1.0, e


# act_grad takes relu' / elu' / tanh' from the saved OUTPUT y, gelu' from the pre-activation
def _dact_from_saved(act, v):
    if act == "relu":
        return (v > 0).double()
    if act == "elu":
        return torch.where(v > 0, torch.ones_like(v), v + 1.0)
    if act == "tanh":
        return 1.0 - v * v
    return _dact64("gelu", v)


@pytest.mark.gpu
@pytest.mark.parametrize("act", ["relu", "elu", "tanh", "gelu"])
@pytest.mark.parametrize("M,N,Np,ld", [(1, 8, 8, 8), (1, 10, 16, 10), (37, 24, 24, 40), (37, 10, 16, 24)])
def test_act_grad_strided_and_single_row(M, N, Np, ld, act):
    """dy with a row stride larger than N (fast path at N == Np, ld % 8 == 0; scalar path
    otherwise) and M = 1.  One fp32 product of two terms and one bf16 rounding: |err| <=
    2^-8 |ref| + 2^-20 |dy| (act' is at most 1.13 and evaluated in fp32)."""
    ext = _ext()
    g = torch.Generator().manual_seed(611953 + 1000 * M + 10 * N + ld)
    dy = torch.randn(M, ld, generator=g).to(BF16)
    src = torch.randn(M, Np, generator=g).clamp(-0.95, 3.0).to(BF16)
    dyd, sd = dy.to(DEV), src.to(DEV)
    for again in (None, True):
        arena = _Arena()
        out = arena.new((M, Np), name="act_grad")
        ext.act_grad(dyd.data_ptr(), ld, N, sd.data_ptr(), out.data_ptr(), M, Np, ACT[act], _st())
        torch.cuda.synchronize()
        arena.check()
        assert again is None or _same(out, first)
        first = out
    dyp = torch.zeros(M, Np, dtype=torch.float64)
    dyp[:, :N] = dy[:, :N].double()
    ref = dyp * _dact_from_saved(act, src.double())
    got = out.double().cpu()
    assert torch.isfinite(got).all()
    assert (got[:, N:] == 0).all(), "the padding columns must be exactly zero"
    lim = 2.0 ** -8 * ref.abs() + 2.0 ** -20 * dyp.abs()
    err = (got - ref).abs()
    assert (err[lim == 0] == 0).all()
    e = (err / lim.clamp_min(1e-300)).max().item()
    _say(f"G act_grad {act} M={M} N={N} Np={Np} ld={ld}: err/bound {e:.3f}")
    assert e <= 1.0, e


# ------------------------------------------------------------------------------- H. refusals before launch


@pytest.mark.gpu
def test_unsupported_dense_geometries_are_refused_before_launch():
    ext = _ext()
    arena = _Arena()
    a = torch.ones(256, 256, dtype=BF16, device=DEV)
    w = torch.ones(256, 256, dtype=BF16, device=DEV)
    aux = torch.ones(256, 256, dtype=BF16, device=DEV)
    ws = arena.new((4, 128, 128), F32, name="slabs")
    c = arena.new((256, 256), name="C")
    c32 = arena.new((128, 128), F32, name="dW")
    st = _st()

    def ex(layout, M, N, K, preact=0, dact=0, ld_aux=0):
        ext.gemm_ex(layout, a.data_ptr(), 256, w.data_ptr(), 256, c.data_ptr(), 256, M, N, K, 0, 0.0, 0, 0, preact,
                    dact, ld_aux, st)

    def bf(layout, M, N, K):
        ext.gemm_bf16(layout, a.data_ptr(), 256, w.data_ptr(), 256, c.data_ptr(), 256, M, N, K, 0, 0.0, st)

    def sk(layout, M, N, K, splits=2):
        ext.gemm_splitk(layout, a.data_ptr(), 256, w.data_ptr(), 256, c32.data_ptr(), 0, 0.0, M, N, K, splits,
                        ws.data_ptr(), st)

    refused = []
    for layout in (NT, NN):
        for fn in (ex, bf):
            refused += [(fn, (layout, 16, 4, 16)), (fn, (layout, 16, 12, 16)), (fn, (layout, 16, 16, 12))]
        refused += [(sk, (layout, 16, 4, 64)), (sk, (layout, 16, 12, 64))]
        # K % 8 != 0 with a K-contiguous operand: the last 16-byte chunk of a row would take the
        # first elements of the next one
        refused += [(sk, (layout, 16, 16, 76)), (sk, (layout, 16, 16, 12, 1))]
    refused += [(ex, (TN, 12, 16, 16)), (bf, (TN, 12, 16, 16)), (sk, (TN, 12, 16, 64))]
    refused += [(ex, (NT, 16, 16, 16, aux.data_ptr(), 0, 20)), (ex, (NN, 16, 16, 16, 0, aux.data_ptr(), 20))]
    for fn, args in refused:
        with pytest.raises(RuntimeError):
            fn(*args)
    torch.cuda.synchronize()
    arena.check()
    for t in (ws, c, c32):
        assert bool(_is_sentinel(t).all()), "a refused call must leave the output untouched"
    _say(f"H {len(refused)} unsupported geometries refused, outputs untouched")


# ------------------------------------------------------------------------------- fix 1: resident-weight beta


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [False, True], ids=["plain", "stats"])
@pytest.mark.parametrize("beta", [0.0, 1.0], ids=["beta0", "beta1"])
@pytest.mark.parametrize("M", [129, 401])
def test_gemm_bf16_beta_at_resident_weight_shapes(M, beta, stats):
    """ext.gemm_bf16 (NT) at N = 256, K = 64, M >= 128, contiguous operands: with beta 0 the
    persistent resident-weight core runs; it has no beta term, so beta 1 must take the tiled core
    and give C = A * B + C (before the fix the accumulate was dropped without an error)."""
    ext = _ext()
    N, K = 256, 64
    d = _gemm_data(NT, M, N, K)
    ad, wd = d.a.to(DEV), d.w.to(DEV)
    rows = ext.gemm_stat_rows(M, N, K, K, K, N) if beta == 0.0 else _cdiv(M, 128)

    def launch():
        arena = _Arena()
        c = arena.new((M, N), fill=d.old if beta else None, name="C")
        st = arena.new((rows, 2, N), F32, name="stats") if stats else None
        ext.gemm_bf16(NT, ad.data_ptr(), K, wd.data_ptr(), K, c.data_ptr(), N, M, N, K, _p(st), beta, _st())
        torch.cuda.synchronize()
        arena.check()
        return c, st

    c, st = launch()
    c2, st2 = launch()
    assert _same(c, c2)  # (the persistent core's partials follow its grid; both launches share it)
    ref = d.acc + beta * d.old.double()
    e_r, e_c = _both_err(c, ref)
    y = c.double().cpu()
    e_st = _partials_err(st, y, y * y) if stats else None
    _say(f"fix1 gemm_bf16 M={M} beta={beta} stats={stats} ({rows} partial rows): out/row {e_r:.3e} out/col {e_c:.3e}"
         + ("" if e_st is None else f" partials err/bound {e_st:.3f}"))
    assert e_r < ROW_BOUND and e_c < ROW_BOUND, (e_r, e_c)
    assert e_st is None or e_st <= 1.0, e_st


# ------------------------------------------------------------------------------- host-only controls
# (no GPU: each shows that the criteria accept the float64 reference rounded to bf16 at the
# kernel's own rounding points and reject one planted defect in a copy of that good output)


def _passes(got, ref):
    try:
        e_r, e_c = _both_err(got, ref)
    except AssertionError:  # the metric's own assertions (non-finite, a true-zero row not zero) reject too
        return False
    return e_r < ROW_BOUND and e_c < ROW_BOUND


def test_control_bias_off_by_one_column_group():
    """One 8-column group of (600, 840, 72) takes the bias of the next group, with a bias of the
    size trained dense layers carry (0.02): each row changes by sqrt(8 / 840) of the defect, so
    the row metric and a whole-tensor norm both pass; the column metric does not."""
    d = _gemm_data(NT, 600, 840, 72)
    small = 0.02 * d.bias.double()
    ref = d.acc + small
    good = _bf(ref)
    assert _passes(good, ref)
    bad = good.clone()
    bad[:, 416:424] = _bf(d.acc[:, 416:424] + small[424:432])
    e_r, e_c = _both_err(bad, ref)
    assert e_r < ROW_BOUND, e_r
    assert _whole_err(bad, ref) < 5e-3
    assert e_c > ROW_BOUND, e_c


def test_control_one_wrong_row_of_600():
    d = _gemm_data(NT, 600, 840, 72)
    ref, _ = _ref_fwd(d, True, "none", 0.0)
    good, _ = _emu_fwd(d, True, "none", 0.0)
    assert _passes(good, ref)
    bad = good.clone()
    bad[300] = _bf(ref[300] * 1.05)
    assert _whole_err(bad, ref) < 5e-3
    assert _row_err(bad, ref)[0] > ROW_BOUND


def test_control_last_k_group_dropped():
    d = _gemm_data(NT, 129, 72, 200)
    ref, _ = _ref_fwd(d, False, "none", 0.0)
    assert _passes(_bf(ref), ref)
    short = d.a.double()[:, :192] @ d.w.double()[:, :192].t()
    assert _row_err(_bf(short), ref)[0] > ROW_BOUND
    t = _tn_data(40, 136, 1000)
    dw = t.a.double().t() @ t.b.double()
    assert _dw_err(dw.float(), dw) < WG32_BOUND and _dw_err(_bf(dw), dw) < WGBF_BOUND
    assert _dw_err((t.a.double()[:992].t() @ t.b.double()[:992]).float(), dw) > WGBF_BOUND


def test_control_stale_beta_in_the_partial_m_tile():
    """Row 128 of (129, 72, 200) with beta = 1 computed as if beta were 0."""
    d = _gemm_data(NT, 129, 72, 200)
    for bias, act in ((False, "none"), (True, "relu")):
        ref, _ = _ref_fwd(d, bias, act, 1.0)
        good, _ = _emu_fwd(d, bias, act, 1.0)
        assert _passes(good, ref)
        bad = good.clone()
        bad[128] = _emu_fwd(d, bias, act, 0.0)[0][128]
        assert _whole_err(bad, ref) > 0 and _row_err(bad, ref)[0] > ROW_BOUND


def test_control_one_slab_of_65_left_out():
    ws, old = _int_slabs(4 * (16 * 600 + 1), 65)
    ref = ws.double().sum(0) + old.double()
    for dtype in (F32, BF16):
        assert torch.equal((ws.sum(0) + old).to(dtype).double(), ref)  # exact in the output type
        assert not torch.equal((ws.sum(0) - ws[37] + old).to(dtype).double(), ref)
    # ... while a whole-tensor norm at the existing tests' bound would not see it in a real gradient
    g = torch.Generator().manual_seed(5)
    real = torch.randn(65, 4096, generator=g)
    assert ((real.sum(0) - real[37]).double() - real.double().sum(0)).norm() / real.double().sum(0).norm() > 5e-3


def test_control_activation_before_bias():
    d = _gemm_data(NT, 129, 72, 200)
    for act in ACTS:
        ref, _ = _ref_fwd(d, True, act, 0.0)
        good, _ = _emu_fwd(d, True, act, 0.0)
        assert _passes(good, ref), act
        bad = _bf(_bf(_act64(act, _bf(d.acc))) + d.bias.double())
        assert not _passes(bad, ref), act


def test_control_all_epilogues_accept_the_rounded_reference():
    """Every NT / NN case and epilogue of groups A and B: the float64 reference rounded at the
    kernel's rounding points passes the row and the column criterion."""
    for M, N, K, _ in NT_CASES:
        d = _gemm_data(NT, M, N, K)
        for name, kw in FWD_EPIS.items():
            bias, act, beta = kw.get("bias", False), kw.get("act", "none"), kw.get("beta", 0.0)
            ref, pre = _ref_fwd(d, bias, act, beta)
            good, gpre = _emu_fwd(d, bias, act, beta)
            assert _passes(good, ref) and _passes(gpre, pre), (M, N, K, name)
    for M, N, K, _ in NN_CASES:
        d = _gemm_data(NN, M, N, K)
        for name, kw in BWD_EPIS.items():
            dact, beta = kw.get("dact"), kw.get("beta", 0.0)
            ref = _ref_bwd(d, dact, beta)
            good = _bf(_bf(d.acc) * _dact64(dact, d.src[:, :N].double())) if dact else _bf(d.acc)
            good = _bf(good + beta * d.old.double()) if beta else good
            assert _passes(good, ref), (M, N, K, name)


def test_control_preact_written_at_ldc():
    """preact rows stored with the output's row stride instead of ld_aux = N + 8: the sentinel
    columns N .. ld_aux-1 trip."""
    M, N = 129, 72
    d = _gemm_data(NT, M, N, 200)
    _, pre = _emu_fwd(d, True, "gelu", 0.0)
    arena = _Arena("cpu")
    good = arena.new((M, N + 8), name="preact")
    good[:, :N] = pre.to(BF16)
    arena.check()
    assert bool(_is_sentinel(good[:, N:]).all()) and _passes(good[:, :N], pre)
    bad = arena.new((M, N + 8), name="preact")
    bad.view(-1)[:M * N] = pre.to(BF16).reshape(-1)  # row stride N
    arena.check()
    assert not bool(_is_sentinel(bad[:, N:]).all())


def test_control_guard_element_overwritten():
    arena = _Arena("cpu")
    c = arena.new((129, 88), name="C")
    ws = arena.new((3, 40, 136), F32, name="slabs")
    out = arena.new((4 * 29,), F32, name="reduced")
    c.zero_(), ws.zero_(), out.zero_()
    arena.check()
    for t, buf in ((c, 0), (ws, 1), (out, 2)):
        flat = arena.bufs[buf][0]
        keep = flat[t.numel()].clone()
        flat[t.numel()] = 0  # the first element past the tensor
        with pytest.raises(AssertionError):
            arena.check()
        flat[t.numel()] = keep
    arena.check()


def test_control_dispatch_mirror_names_every_branch():
    """The shapes of groups A - D reach every tile form between them."""
    routes = {_route(5, NT, M, N, K) for M, N, K, _ in NT_CASES} | {_route(5, NN, M, N, K) for M, N, K, _ in NN_CASES}
    routes |= {_route(5, TN, M, N, K, _cdiv(K, _kps(K, s)), _kps(K, s)) for M, N, K, s, _ in TN_CASES}
    routes |= {_route(6, NT, *c) for c in CORE6_CASES} | {_route(5, NT, 8000, 2304, 136)}
    assert routes == {"128x64", "128x128", "64x128", "256x256", "256x96"}
    assert [_reduce_form(mn) for mn, _ in REDUCE_MN] == [f for _, f in REDUCE_MN]
