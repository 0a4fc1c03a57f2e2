"""Edge-case reference tests for the training BatchNorm kernels (csrc/kernels/bn.hip: ca_bn_fwd,
ca_bn_fwd_partials[_ex], ca_bn_apply, ca_bn_bwd, ca_bn_bwd_partials) and the global pools
(csrc/kernels/pool.hip: gap_fwd / gap_bwd / gmp_fwd / gmp_bwd).

The float64 references, the criteria with their derivation, the tiling model, the inputs and the
case lists live in test_bn_reference_cpu.py, which proves them on the CPU; nothing here sets a
bound.  Kernels are called through cloud_amd.ops.raw under ``_guarded_raw`` or through the ext
bindings, every output and workspace from ``_Arena`` of test_bn_fold_edges_gpu.py: pre-filled with
the NaN sentinel, 128 guard rows checked bit for bit after every launch.  Inputs come from a host
``torch.Generator`` with a fixed seed per case.

Elementwise outputs (y, dx, the shortcut form) are judged against the float64 expression of the
kernel's OWN fp32 coefficients read back from the device, so they do not depend on the
statistics tests.  The two exact-integer cases (87041x24, 16389x512: 2.1 M and 8.4 M elements) run a
reduced combination matrix: the mask always kept, statistics from partials and the gate from y on
one combination each.

Switches read once per process run in child interpreters, one after the other.  The forward
outputs, dres, and dx under the two apply-grid switches must have the default setting's bits on
all three cases.  Under CLOUD_AMD_BN_FIN_MERGED=0 / CLOUD_AMD_BN_FIN_RPG=64 the backward sums of
300x512 (75 chunks) are grouped differently in fp32, so its coefficients may move in the last
bit: there dx is held to the criterion, and bit for bit on 200x24 (no group pass) and on the
exact-integer 87041x24 (any grouping is exact).

Worst figures observed on an MI355X (each test prints its figures before asserting; reported,
never used to set a bound):

    group                                                     worst observed              bound
    forward y, err / bound (derived)                          0.996                       1
    forward mean / rstd / scale / shift, err / bound          0.18 / 0.18 / 0.41 / 0.15   1 (exact cases: 2^-22)
      random cases alone                                      0.01 / 0.15 / 0.15 / 0.15   1
    running mean / var, err / bound                           0.50 / 0.43                 1
    forward sums of the exact-integer cases                   equal                       equal
    near-zero elements, worst share                           1.9e-4 (131x40: 1 of 5240)  1e-3
    shortcut form y, err / bound; against the op-by-op path   0.964; bitwise equal        1; equal
    statistics-only: rstd / scale / shift                     0.04 / 0.04 / 0.02          1
    inference apply y, err / bound                            0.995                       1
    backward dx, err / bound (derived)                        0.996                       1
    backward dgamma / dbeta, err / counted bound              0.16 / 0.09                 1
    backward A / B / D, err / bound                           0.49 / 0.12 / 0.09          1
    exact-integer cases: dgamma, dbeta; A / B / D             equal; 0 / 0.23 / 0.24      equal; 1 (2^-22 S)
    ``partials=`` dgamma / dbeta, err / bound; dx             0.13 / 0.05; 0.996          1
    gate from the mask against the gate from y                bitwise equal               equal
    repeat, second stream, switches in child interpreters     bitwise equal               equal
    gap_fwd bf16 / fp32, err / bound; integer inputs          0.996 / 0.021; bit-exact    1
    gap_bwd bf16 / fp32 dy, err / bound                       0.946 / 0.995               1
    gmp_fwd value and tie count                               exact                       exact
    gmp_bwd per element; share sums against dy                0.995; 0.995                1

The signed-zero channel of the global max pool (maximum 0, positions -0.0, -0.0 .. +0.0): with a
compare of the bf16 bit patterns in gmp_bwd_kernel 2 of the 3 zeros got dy / 3 and the shares
missed dy by 85 x the bound (per element 256 x); the kernel now compares values, as gmp_fwd_kernel
counts them, and all 3 share.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bn_fold_edges_gpu as FE  # noqa: E402  (the guarded output arena)
import test_bn_reference_cpu as B  # noqa: E402  (references, criteria, inputs, cases)

pytestmark = pytest.mark.gpu

_Arena, _guarded_raw, _say, _relu_bits = FE._Arena, FE._guarded_raw, B._say, B._relu_bits
DEV, BF16, F32 = "cuda", torch.bfloat16, torch.float32
EPS, MOM = B.EPS, B.MOM
_ids = B._ids


def _ext():
    from cloud_amd.ops import _ext as e

    return e.load(required=True)


def _stream():
    from cloud_amd.ops import _ext as e

    return e.stream_handle(torch.device(DEV, torch.cuda.current_device()))


def _raw_buf(arena, n, dtype=F32):
    """The tensor of ``n`` elements a raw launcher allocated for itself (workspace, coefficients)."""
    hits = [buf[:k] for buf, k, name in arena.bufs if name == "raw-allocated" and k == n and buf.dtype == dtype]
    assert len(hits) == 1, (n, len(hits))
    return hits[0]


def _worst(w, r):
    for k, v in r.items():
        w[k] = max(w.get(k, 0.0), v)
    return w


# ------------------------------------------------------------------------------- forward


def _forward(c, relu, res, keep_mask=True, source="kernel", affine=True, running=True, tag="fwd"):
    """raw.bn_fwd of one case, held to the criteria.  Returns the figures and the outputs."""
    from cloud_amd.ops import gemm

    M, C = c.M, c.C
    d = B.bn_data(M, C, c.data)
    exact = c.data == "integer"
    arena = _Arena()
    x = d.x.to(DEV)
    r = d.res.to(DEV) if res else None
    gamma, beta = (d.gamma.to(DEV), d.beta.to(DEV)) if affine else (None, None)
    rm = arena.new(C, F32, fill=d.rm, name="run_mean") if running else None
    rv = arena.new(C, F32, fill=d.rv, name="run_var") if running else None
    part = None
    if source == "partials":
        part = arena.new(((M + 127) // 128, 2, C), F32, name="partials")
        gemm.fill_stats_torch(x, part)
    with _guarded_raw(arena) as raw:
        y, stats, mask = raw.bn_fwd(x, gamma, beta, rm, rv, EPS, MOM, relu, residual=r, partials=part,
                                    keep_mask=keep_mask)
    torch.cuda.synchronize()
    arena.check()
    assert arena.owns(y) and arena.owns(stats), "the launcher's own allocations must come from the guarded arena"
    assert (mask is not None) == (relu and keep_mask)
    g_h, b_h = (d.gamma, d.beta) if affine else (None, None)
    w = dict(B.stats_ratio(stats, d.x, g_h, b_h, exact=exact))
    if running:
        w.update(B.running_ratio(rm, rv, d.rm, d.rv, d.x, exact=exact))
    if source == "kernel":  # the reduction's own partial sums: every chunk written; exact on integer data
        t = B.make_tiling(M, C)
        ws = _raw_buf(arena, _ext().bn_workspace_floats(M, C))[:2 * t.nchunks * C].cpu().view(2, t.nchunks, C)
        assert torch.isfinite(ws).all(), "a chunk's partial sums were not written"
        if exact:
            st = B.stats64(d.x, None, None)
            assert st.Ssum.max() < 2 ** 24 and st.sumsq.max() < 2 ** 24
            assert torch.equal(ws[0].double().sum(0), st.sum) and torch.equal(ws[1].double().sum(0), st.sumsq), \
                "exact-integer sums must EQUAL the float64 sums"
    sh = stats.cpu()
    f = B.fwd_check(y, mask, *B.apply64(d.x, sh[2 * C:3 * C], sh[3 * C:], d.res if res else None), relu)
    w["y"] = f.ratio
    if affine and not res:
        assert (y[:, B.CH_GAMMA0] == 0).all(), "gamma = beta = 0: y must be exactly 0"
        assert mask is None or (mask[:, 0] & 1 == 0).all()
    _say(f"{tag} {c.name} relu={int(relu)} res={int(res)} mask={int(keep_mask)} {source}: err / bound",
         {k: round(v, 3) for k, v in w.items()}, f"near-zero {f.unsure}")
    assert max(w.values()) <= 1.0, w
    return w, B._D(y=y, mask=mask, stats=stats, keep=f.keep, rm=rm, rv=rv)


@pytest.mark.parametrize("relu,res", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["plain", "res", "relu", "res_relu"])
@pytest.mark.parametrize("c", B.CASES, ids=_ids)
def test_forward_vs_fp64(c, relu, res):
    """relu x residual, each with and without the kept mask, statistics from the kernel's own
    reduction and from fill_stats_torch partials."""
    _, base = _forward(c, relu, res, True, "kernel")
    if B.reduced(c):
        if relu and res:
            _, o = _forward(c, relu, res, True, "partials")
            assert torch.equal(o.y, base.y) and torch.equal(o.mask, base.mask)  # exact sums: the same coefficients
        return
    for keep_mask, source in ((True, "partials"),) + (((False, "kernel"), (False, "partials")) if relu else ()):
        _, o = _forward(c, relu, res, keep_mask, source)
        if source == "kernel":
            assert torch.equal(o.y, base.y), "y must not depend on whether the mask is kept"


def test_null_affine_and_absent_running_stats():
    c = B.CASE["200x24"]
    for relu, res in ((True, True), (False, False)):
        _forward(c, relu, res, True, "kernel", affine=False, running=False, tag="fwd[no affine, no running]")
        _forward(c, relu, res, True, "partials", affine=False, running=True, tag="fwd[no affine]")
    _backward(c, True, True, "mask", 0, affine=False)
    _backward(c, False, False, "mask", 0, affine=False)


@pytest.mark.parametrize("c", B.SHORTCUT_CASES, ids=_ids)
def test_shortcut_form_and_statistics_only(c):
    """raw.bn_fwd(residual_ss=...) (bn_apply_resbn_kernel) and raw.bn_fwd_stats: the derived bound,
    and bit for bit the op-by-op path (the shortcut BN's stored output as a plain residual)."""
    from cloud_amd.ops import gemm

    M, C = c.M, c.C
    d = B.bn_data(M, C, c.data)
    ext = _ext()
    arena = _Arena()
    x, r, rss = d.x.to(DEV), d.r.to(DEV), d.rss.to(DEV)
    gamma, beta = d.gamma.to(DEV), d.beta.to(DEV)
    part = arena.new(((M + 127) // 128, 2, C), F32, name="partials")
    gemm.fill_stats_torch(x, part)
    w = {}
    with _guarded_raw(arena) as raw:
        rm, rv = arena.new(C, F32, fill=d.rm), arena.new(C, F32, fill=d.rv)
        only = raw.bn_fwd_stats(x, gamma, beta, rm, rv, EPS, MOM, part)
        torch.cuda.synchronize()
        _worst(w, B.stats_ratio(only, d.x, d.gamma, d.beta))
        _worst(w, B.running_ratio(rm, rv, d.rm, d.rv, d.x))
        idn = arena.new((M, C), name="idn")
        ext.bn_apply(r.data_ptr(), 0, idn.data_ptr(), M, C, rss.data_ptr(), 0, _stream())
        for relu in (True, False):
            y, stats, mask = raw.bn_fwd(x, gamma, beta, None, None, EPS, MOM, relu, residual=r, partials=part,
                                        keep_mask=True, residual_ss=rss)
            y2, stats2, mask2 = raw.bn_fwd(x, gamma, beta, None, None, EPS, MOM, relu, residual=idn, partials=part,
                                           keep_mask=True)
            torch.cuda.synchronize()
            assert torch.equal(stats, only) and torch.equal(stats2, only)
            sh = stats.cpu()
            pre, S, extra, alt = B.resbn64(d.x, sh[2 * C:3 * C], sh[3 * C:], d.r, d.rss[:C], d.rss[C:])
            f = B.fwd_check(y, mask, pre, S, relu, extra, alt)
            w["shortcut"] = max(w.get("shortcut", 0.0), f.ratio)
            assert torch.equal(y.view(torch.int16), y2.view(torch.int16)), "not bit-compatible with the op-by-op path"
            assert mask is None or torch.equal(mask, mask2)
    arena.check()
    _say(f"shortcut {c.name}: err / bound", {k: round(v, 3) for k, v in w.items()})
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("c", B.INFER_CASES, ids=_ids)
def test_inference_apply(c):
    """bn_act(training=False) -> ca_bn_apply with the wrapper's fp32 [scale | shift]."""
    from cloud_amd.ops.batchnorm import bn_act

    M, C = c.M, c.C
    d = B.bn_data(M, C, c.data)
    x, res = d.x.to(DEV), d.res.to(DEV)
    gamma, beta, rm, rv = d.gamma.to(DEV), d.beta.to(DEV), d.rm.to(DEV), d.rv.to(DEV)
    scale = torch.rsqrt(rv + EPS) * gamma
    ss = torch.cat([scale, beta - rm * scale]).float().contiguous()
    w = 0.0
    for relu, with_res in ((True, True), (True, False), (False, True), (False, False)):
        y = bn_act(x, gamma, beta, rm, rv, residual=res if with_res else None, eps=EPS, relu=relu, training=False)
        arena = _Arena()
        y2 = arena.new((M, C), name="y")
        _ext().bn_apply(x.data_ptr(), res.data_ptr() if with_res else 0, y2.data_ptr(), M, C, ss.data_ptr(), int(relu),
                        _stream())
        torch.cuda.synchronize()
        arena.check()
        assert torch.equal(y.view(torch.int16), y2.view(torch.int16))
        assert torch.equal(rm.cpu(), d.rm) and torch.equal(rv.cpu(), d.rv), "inference must not touch the running stats"
        sh = ss.cpu()
        w = max(w, B.fwd_check(y2, None, *B.apply64(d.x, sh[:C], sh[C:], d.res if with_res else None), relu).ratio)
    _say(f"inference apply {c.name}: y err / bound {w:.3f}")
    assert w <= 1.0, w


# ------------------------------------------------------------------------------- backward


@functools.lru_cache(maxsize=2)
def _fwd_for_bwd(name, relu, res):
    c = B.CASE[name]
    d = B.bn_data(c.M, c.C, c.data)
    if c.data == "integer":  # planted gate, integer mean, power-of-two rstd
        return B._D(stats=B.planted_stats(d).to(DEV), keep=d.keep if relu else None, y=d.y_planted.to(DEV),
                    mask=_relu_bits(d.keep).to(DEV) if relu else None)
    return _forward(c, relu, res, True, "kernel", tag="fwd(for bwd)")[1]


def _backward(c, relu, want_dres, gate, accumulate, affine=True, partials=False, exact=None, tag="bwd"):
    """raw.bn_bwd of one case from the forward's outputs (or the planted ones), held to the
    criteria.  Returns the figures and the outputs."""
    M, C = c.M, c.C
    d = B.bn_data(M, C, c.data)
    exact = (c.data == "integer" and not accumulate and not partials) if exact is None else exact
    f = (_fwd_for_bwd(c.name, relu, want_dres) if affine
         else _forward(c, relu, want_dres, True, "kernel", affine=False)[1])
    keep = f.keep if relu else None
    sh = f.stats.cpu()
    mean, rstd = sh[:C], sh[C:2 * C]
    g_h = d.gamma if affine else None
    ref = B.bwd_ref(d, keep, mean, rstd, g_h)
    arena = _Arena()
    old = (d.old_dgamma, d.old_dbeta) if accumulate else None
    dgamma = arena.new(C, F32, fill=old[0] if old else None, name="dgamma")
    dbeta = arena.new(C, F32, fill=old[1] if old else None, name="dbeta")
    dx_out = arena.new((M, C), name="dx")
    part = arena.new(((M + 127) // 128, 2, C), F32, fill=B.partials_of(ref.dz, ref.dz * d.x.double()),
                     name="partials") if partials else None
    use_mask = relu and gate == "mask"
    with _guarded_raw(arena) as raw:
        dx, dres = raw.bn_bwd(d.dy.to(DEV), f.y if (relu and not use_mask) else None, d.x.to(DEV),
                              d.gamma.to(DEV) if affine else None, f.stats, relu, dgamma=dgamma, dbeta=dbeta,
                              want_dres=want_dres, dx_out=dx_out, accumulate=int(accumulate),
                              mask=f.mask if use_mask else None, partials=part)
    torch.cuda.synchronize()
    arena.check()
    assert dx.data_ptr() == dx_out.data_ptr() and (dres is None or arena.owns(dres))
    coef = _raw_buf(arena, 3 * C)
    if partials:
        w = dict(B.raw_ratio(dgamma, dbeta, ref, part.shape[0], int(os.environ.get("CLOUD_AMD_BN_FIN_RPG", 512)), old))
        assert torch.isfinite(coef).all()
    else:
        w = dict(B.sums_ratio(dgamma, dbeta, coef, ref, M, C, mean, B.chain_k(M, C, "dgamma", accumulate),
                              B.chain_k(M, C, "dbeta", accumulate), old, exact))
    ch = coef.cpu()
    w["dx"] = B.elem_ratio(dx, *B.dx64(ref.dz, d.x, ch[:C], ch[C:2 * C], ch[2 * C:]))
    if want_dres:
        want = d.dy.view(torch.int16) * (keep.to(torch.int16) if keep is not None else 1)
        assert torch.equal(dres.cpu().view(torch.int16), want), "dres: the bits of dy where gated on, +0 elsewhere"
    if affine:
        assert (dx[:, B.CH_GAMMA0] == 0).all(), "gamma = 0: dx must be exactly 0"
    _say(f"{tag} {c.name} relu={int(relu)} dres={int(want_dres)} gate={gate} acc={int(accumulate)}"
         f"{' partials' if partials else ''}{' exact' if exact else ''}: err / bound",
         {k: round(v, 3) for k, v in w.items()})
    assert max(w.values()) <= 1.0, w
    return w, B._D(dx=dx, dres=dres, dgamma=dgamma, dbeta=dbeta, coef=coef, unsure=0)


@pytest.mark.parametrize("relu,want_dres", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["plain", "dres", "relu", "relu_dres"])
@pytest.mark.parametrize("c", B.CASES, ids=_ids)
def test_backward_vs_fp64(c, relu, want_dres):
    """relu x dres; the gate from the forward's mask and from y (identical bits); dgamma / dbeta
    written over the NaN sentinel and accumulated into pre-loaded values."""
    _, base = _backward(c, relu, want_dres, "mask", 0)
    big = B.reduced(c)
    if relu and (not big or want_dres):
        _, o = _backward(c, relu, want_dres, "y", 0)
        # mask bit == (y > 0) everywhere (asserted by the forward), so the two gates agree on every
        # element, also on the few whose pre-activation is too close to zero to call
        for k in ("dx", "dres", "dgamma", "dbeta", "coef"):
            assert (base[k] is None and o[k] is None) or torch.equal(base[k], o[k]), k
    if not big or not want_dres:
        _backward(c, relu, want_dres, "mask", 1)


@pytest.mark.parametrize("name", ["234x64", "300x512", "16641x8"])
def test_backward_from_partials(name):
    """``partials=`` (raw moments per 128-row tile, float64-exact, rounded once): 2, 3 and 131
    rows, the last through the group pass."""
    c = B.CASE[name]
    for relu, acc in ((True, 0), (False, 1)):
        _, p = _backward(c, relu, True, "mask", acc, partials=True)
        _, k = _backward(c, relu, True, "mask", acc)
        assert torch.equal(p.dres, k.dres)


def test_repeat_and_second_stream():
    """A second launch from the same inputs gives identical bits; so does a launch on a second
    stream (the ticket words of group_finalize_kernel are per stream and must re-arm)."""
    c = B.CASE["300x512"]
    _fwd_for_bwd.cache_clear()
    runs = []
    for rep in range(2):
        _, f = _forward(c, True, True, True, "partials", tag=f"fwd[repeat {rep}]")
        _, b = _backward(c, True, True, "mask", 0, tag=f"bwd[repeat {rep}]")
        _, p = _backward(c, True, True, "mask", 0, partials=True, tag=f"bwd[repeat {rep}]")
        runs.append((f.y, f.mask, f.stats, b.dx, b.dres, b.dgamma, b.dbeta, b.coef, p.dx, p.dgamma))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        for rep in range(2):
            _fwd_for_bwd.cache_clear()
            _, f = _forward(c, True, True, True, "partials", tag=f"fwd[stream 2, {rep}]")
            _, b = _backward(c, True, True, "mask", 0, tag=f"bwd[stream 2, {rep}]")
            _, p = _backward(c, True, True, "mask", 0, partials=True, tag=f"bwd[stream 2, {rep}]")
            runs.append((f.y, f.mask, f.stats, b.dx, b.dres, b.dgamma, b.dbeta, b.coef, p.dx, p.dgamma))
    s.synchronize()
    torch.cuda.synchronize()
    _fwd_for_bwd.cache_clear()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------- switches read once per process


def _digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _apply_digests(tag=""):
    """Forward (res, ReLU, mask kept) and backward (dres) of the child cases to the criteria;
    returns the digests of the apply outputs."""
    out = {}
    for name in B.CHILD_CASES:
        c = B.CASE[name]
        _fwd_for_bwd.cache_clear()
        _, f = _forward(c, True, True, True, "kernel", tag="fwd" + tag)
        _, b = _backward(c, True, True, "mask", 0, tag="bwd" + tag)
        if c.data == "integer":  # 681 partial rows: the group pass of the ``partials=`` path under every setting
            _backward(c, True, True, "mask", 0, partials=True, tag="bwd" + tag)
        out[name + " fwd"] = _digest(f.y, f.mask)
        out[name + " dres"] = _digest(b.dres)
        out[name + " dx"] = _digest(b.dx)
    _fwd_for_bwd.cache_clear()
    return out


def _child(tag, sums_regrouped):
    got = _apply_digests(tag)
    want = json.loads(os.environ["BN_EDGES_EXPECT"])
    for k, v in want.items():
        if sums_regrouped and k == "300x512 dx":
            continue  # held to the criterion above: see the module docstring
        assert got[k] == v, f"{k}: the apply output differs from the default setting's bits"


_CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_bn_kernel_edges_gpu as T
T._child({tag!r}, {regrouped!r})
print("BN_KERNEL_EDGES_OK")
"""
_child_failed = []
_default_digests = {}

SWITCHES = [("CLOUD_AMD_BN_APPLY_ILV", "0", False), ("CLOUD_AMD_BN_APPLY_BLOCKS", "3", False),
            ("CLOUD_AMD_BN_FIN_MERGED", "0", True), ("CLOUD_AMD_BN_FIN_RPG", "64", True)]


@pytest.mark.parametrize("var,value,regrouped", SWITCHES, ids=[f"{v}={x}" for v, x, _ in SWITCHES])
def test_switches_read_once_per_process(var, value, regrouped):
    """Each setting in its own interpreter, one after the other, against the same references; the
    apply outputs against the digests of the default setting.  None is started after one failed."""
    assert not _child_failed, f"not started: the child for {_child_failed[0]} failed"
    if not _default_digests:
        _default_digests.update(_apply_digests("[default]"))
    tests = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ)
    env[var] = value
    env["BN_EDGES_EXPECT"] = json.dumps(_default_digests)
    code = _CHILD.format(root=os.path.dirname(tests), tests=tests, tag=f"[{var}={value}]", regrouped=regrouped)
    _child_failed.append(f"{var}={value}")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110)
    print(r.stdout)
    assert r.returncode == 0 and "BN_KERNEL_EDGES_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    _child_failed.pop()


# ------------------------------------------------------------------------------- controls
# A copy of the kernel's output is corrupted on the host and the criterion must reject it; nothing
# is provoked on the device.


def test_control_one_ulp_mask_bit_and_guard():
    c = B.CASE["234x64"]
    M, C = c.M, c.C
    d = B.bn_data(M, C, c.data)
    _, f = _forward(c, True, True, True, "kernel", tag="control fwd")
    sh = f.stats.cpu()
    pre, S = B.apply64(d.x, sh[2 * C:3 * C], sh[3 * C:], d.res)
    y, mask = f.y.cpu(), f.mask.cpu()
    assert B.fwd_check(y, mask, pre, S, True).ratio <= 1.0
    # one element of y moved past the bound by whole bf16 ulps, away from the reference
    i = int(pre.clamp_min(0).flatten().argmax())
    bad = y.clone().flatten()
    step = 2 if bad[i].double() >= pre.flatten()[i] else -2
    bad.view(torch.int16)[i] += step
    assert B.fwd_check(bad.view(M, C), mask, pre, S, True).ratio > 1.0
    # one mask bit flipped
    flipped = mask.clone()
    flipped[M // 2, 3] ^= 4
    with pytest.raises(AssertionError):
        B.fwd_check(y, flipped, pre, S, True)
    # one guard element overwritten
    arena = _Arena("cpu")
    t = arena.new((M, C), name="y")
    t.copy_(y)
    arena.check()
    arena.bufs[0][0][t.numel()] = 0
    with pytest.raises(AssertionError):
        arena.check()


def test_control_one_row_missing_from_dbeta():
    for name in ("6272x256", "16389x512"):
        c = B.CASE[name]
        M, C = c.M, c.C
        d = B.bn_data(M, C, c.data)
        exact = c.data == "integer"
        _, b = _backward(c, True, False, "mask", 0, tag="control bwd")
        f = _fwd_for_bwd(name, True, False)
        sh = f.stats.cpu()
        ref = B.bwd_ref(d, f.keep, sh[:C], sh[C:2 * C], d.gamma)
        kg, kb = B.chain_k(M, C, "dgamma"), B.chain_k(M, C, "dbeta")
        assert max(B.sums_ratio(b.dgamma, b.dbeta, b.coef, ref, M, C, sh[:C], kg, kb, exact=exact).values()) <= 1.0
        row = M - 1
        short = (b.dbeta.cpu().double() - ref.dz[row]).float()
        assert not torch.equal(short, b.dbeta.cpu())
        if exact:
            with pytest.raises(AssertionError):
                B.sums_ratio(b.dgamma, short, b.coef, ref, M, C, sh[:C], kg, kb, exact=True)
        else:
            r = B.sums_ratio(b.dgamma, short, b.coef, ref, M, C, sh[:C], kg, kb)
            _say(f"control {name}: dbeta without row {row}: {r.dbeta:.1f} of the bound")
            assert r.dbeta > 1.0
    _fwd_for_bwd.cache_clear()


# ------------------------------------------------------------------------------- global pools

_pool_ids = lambda c: "x".join(map(str, c))  # noqa: E731


@pytest.mark.parametrize("case", B.POOL_CASES, ids=_pool_ids)
def test_global_average_pool_vs_fp64(case):
    """gap_fwd with bf16 and fp32 output, gap_bwd with bf16 and fp32 dy; integer inputs bit-exact."""
    N, H, W, C = case
    HW = H * W
    ext = _ext()
    w = {}
    for integer in (False, True):
        d = B.pool_data(N, H, W, C, integer)
        x = d.x.to(DEV)
        for bf in (True, False):
            arena = _Arena()
            y = arena.new((N, C), BF16 if bf else F32, name="y")
            ext.gap_fwd(x.data_ptr(), y.data_ptr(), int(bf), N, HW, C, _stream())
            dy = (d.dy.to(BF16) if bf else d.dy)
            dx = arena.new((N * HW, C), name="dx")
            dyd = dy.to(DEV)
            ext.gap_bwd(dyd.data_ptr(), int(bf), dx.data_ptr(), N, HW, C, _stream())
            torch.cuda.synchronize()
            arena.check()
            k = "_bf16" if bf else "_fp32"
            w["gap" + k] = max(w.get("gap" + k, 0.0), B.gap_ratio(y, d.x, bf))
            w["gap_bwd" + k] = max(w.get("gap_bwd" + k, 0.0), B.gap_bwd_ratio(dx.view(N, HW, C), dy, HW))
            if integer:
                assert torch.equal(y.cpu(), B.gap_exact(d.x, bf)), "integer inputs: float32(sum) * float32(1 / HW)"
                inv = torch.tensor(1.0) / torch.tensor(float(HW))
                assert torch.equal(dx.cpu().view(N, HW, C), (dy.float() * inv).to(BF16)[:, None].expand(-1, HW, -1))
    _say(f"gap {case}: err / bound", {k: round(v, 3) for k, v in w.items()})
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("case", B.POOL_CASES, ids=_pool_ids)
def test_global_max_pool_vs_fp64(case):
    """gmp_fwd: values and tie counts exact; gmp_bwd with bf16 and fp32 dy: per element, zeros
    below the maximum, and the shares of every (n, c) summing to dy -- on the planted ties too: a
    whole-channel tie at 0, a two-way tie, an all-negative channel, a zero maximum of both signs."""
    N, H, W, C = case
    HW = H * W
    ext = _ext()
    d = B.pool_data(N, H, W, C)
    x = d.x.to(DEV)
    m, cnt_ref = B.gmp64(d.x)
    w = {}
    for bf in (True, False):
        arena = _Arena()
        y, cnt = arena.new((N, C), name="y"), arena.new((N, C), F32, name="cnt")
        ext.gmp_fwd(x.data_ptr(), y.data_ptr(), cnt.data_ptr(), N, HW, C, _stream())
        dy = d.dy.to(BF16) if bf else d.dy
        dyd = dy.to(DEV)
        dx = arena.new((N * HW, C), name="dx")
        ext.gmp_bwd(dyd.data_ptr(), int(bf), x.data_ptr(), y.data_ptr(), cnt.data_ptr(), dx.data_ptr(), N, HW, C,
                    _stream())
        torch.cuda.synchronize()
        arena.check()
        assert torch.equal(y.double().cpu(), m), "the maximum must be exact"
        assert torch.equal(cnt.double().cpu(), cnt_ref), "the tie count must be exact"
        for ch, k in B.planted_tie_counts(d).items():
            assert cnt[0, ch].item() == k and cnt[N - 1, ch].item() == k, (ch, k)
        per, tot = B.gmp_bwd_ratio(dx.view(N, HW, C), dy, d.x)
        sz = dx.view(N, HW, C)[0, :, B.CH_SZERO].double().cpu()
        _say(f"gmp {case} dy {'bf16' if bf else 'fp32'}: per element {per:.3f}, share sums {tot:.3f} of the bound; "
             f"signed-zero channel: {int((sz != 0).sum())} of {min(HW, 3)} zeros share dy")
        w["per" + str(bf)], w["sum" + str(bf)] = per, tot
    assert max(w.values()) <= 1.0, w
