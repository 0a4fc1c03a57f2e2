"""LayerNorm at any width on the GPU: ``raw.layer_norm_fwd`` / ``raw.layer_norm_bwd`` (the
any-width kernels of csrc/kernels/layernorm.hip and, for ``C % 4 == 0``, ``C <= 1344`` with
8-byte-aligned activations, the tuned pair of rowops.hip), ``ops.layer_norm`` and the Keras
``LayerNormalization`` on top of them.

Every reference is an fp64 LayerNorm of the same bf16 / fp32 inputs.  Metrics are per row, as
in test_bert_kernel_edges_gpu.test_layernorm_rows_vs_fp64, with the project's bounds:

    y / row  < 1e-2      dh / row  < 2e-2      dgamma, dbeta (relative norm)  < 1e-2
    |mean - ref| / max(|ref mean|, row sd)  < 1e-5      |rstd * sd - 1|  < 1e-5

The shapes: widths that are no multiple of 4 (rows then start on 2-byte boundaries), the first
widths past the tuned backward (1347, 1348) and around the tuned forward's limit (2048, 2052),
wide rows with a ragged last vector (16383), every (lanes per row, vectors per lane) bucket of
the new kernels (C <= 512 / 1024: one wave per row; <= 2048 / 4096: 256 lanes; <= 8192: 512
lanes; above: 512 lanes forward, 1024 backward -- 1001 and 6150 are there for the second and the
fifth), and 2053 rows of 131 (odd row pitch, several row chunks in the column pass).

The inputs are seeded on the host.  With a residual the backward reads the bf16-rounded sum
h, as the BERT path does, and the reference the unrounded one: that rounding is the 2e-3 of
dgamma in the residual rows below, and on a row of 3 or 6 columns, where dh is what is left of
g*dy after two projections, it reaches a few 1e-3 of the row.  An fp32 emulation of the kernels'
arithmetic on the CPU gives the same figures to two digits.

Worst figures observed on an MI355X (each test prints its own before asserting):

    group                             y/row     dh/row    dgamma    dbeta     mean      rstd
    shapes, plain                     2.68e-03  2.56e-03  1.27e-07  2.92e-08  3.46e-08  1.65e-07
    shapes, residual                  2.55e-03  3.54e-03  2.27e-03  3.11e-08  2.46e-08  1.31e-07
    mean 64                           1.80e-03  1.83e-03  8.51e-08  0         5.72e-08  8.74e-08
    mean 64 + residual (forward)      2.02e-03  -         -         -         1.34e-07  6.41e-08
    constant row                      1.72e-03  1.86e-03  7.88e-08  0         6.91e-09  7.76e-08
    aligned base (C = 128, 131)       2.02e-03  2.03e-03  2.18e-03  0         8.02e-09  1.23e-07
    shifted base (C = 128, 131)       2.02e-03  2.03e-03  2.19e-03  0         8.02e-09  1.23e-07
    ops.layer_norm, 3-D + residual    1.95e-03  2.11e-03  1.72e-03  0         -         -
    Keras layer                       1.99e-03  2.18e-03  1.05e-07  0         -         -
    bounds                            1e-2      2e-2      1e-2      1e-2      1e-5      1e-5
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS = 1e-3
Y_BOUND, DH_BOUND, DP_BOUND, STAT_BOUND = 1e-2, 2e-2, 1e-2, 1e-5

SHAPES = [(5, 3), (7, 6), (5, 131), (5, 1001), (5, 1347), (5, 1348), (3, 2048), (3, 2052), (3, 4096), (3, 6150),
          (2, 16384), (3, 16383), (2053, 131)]


def _say(*a):
    print("[layer_norm]", *a, flush=True)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


def _row_err(got, ref):
    return ((got.double() - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max().item()


def make_inputs(M, C, res, seed=5, offset=0.0, device=DEV):
    """bf16 x, residual (or None), dy and fp32 gamma, beta, from a host generator."""
    g = torch.Generator().manual_seed(seed + 1000 * C + M)
    x = (torch.randn(M, C, generator=g) + offset).to(torch.bfloat16)
    r = torch.randn(M, C, generator=g).to(torch.bfloat16) if res else None
    dy = torch.randn(M, C, generator=g).to(torch.bfloat16)
    gamma = torch.randn(C, generator=g) * 0.5 + 1
    beta = torch.randn(C, generator=g) * 0.1
    return tuple(None if t is None else t.to(device) for t in (x, r, dy, gamma, beta))


def reference(x, r, dy, gamma, beta, eps=EPS):
    """fp64 LayerNorm of the same inputs: y, dh, dgamma, dbeta, mean, sd = sqrt(var + eps)."""
    h = x.double() if r is None else x.double() + r.double()
    h.requires_grad_()
    gr, br = gamma.double().requires_grad_(), beta.double().requires_grad_()
    y = F.layer_norm(h, (x.shape[-1],), gr, br, eps)
    y.backward(dy.double())
    hd = h.detach()
    return dict(y=y.detach(), dh=h.grad, dgamma=gr.grad, dbeta=br.grad, mean=hd.mean(-1),
                sd=(hd.var(-1, unbiased=False) + eps).sqrt(), h=hd)


def errors(out, ref):
    """out: dict y, dh, dgamma, dbeta, mean, rstd (any subset of the gradients)."""
    e = dict(y=_row_err(out["y"], ref["y"]),
             mean=((out["mean"].double() - ref["mean"]).abs() / torch.maximum(ref["mean"].abs(), ref["sd"])).max().item(),
             rstd=(out["rstd"].double() * ref["sd"] - 1).abs().max().item())
    if "dh" in out:
        e.update(dh=_row_err(out["dh"], ref["dh"]), dgamma=rel(out["dgamma"], ref["dgamma"]),
                 dbeta=rel(out["dbeta"], ref["dbeta"]))
    return e


def check(e, tag):
    _say(tag + ": " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["mean"] < STAT_BOUND and e["rstd"] < STAT_BOUND, (tag, e)
    assert e["y"] < Y_BOUND, (tag, e)
    if "dh" in e:
        assert e["dh"] < DH_BOUND, (tag, e)
        assert e["dgamma"] < DP_BOUND and e["dbeta"] < DP_BOUND, (tag, e)


def run_raw(x, r, dy, gamma, beta, eps=EPS):
    from cloud_amd.ops import raw

    y, h, mean, rstd = raw.layer_norm_fwd(x, gamma, beta, eps, residual=r)
    assert (h is not None) == (r is not None)
    dh, dgamma, dbeta = raw.layer_norm_bwd(dy, x if h is None else h, mean, rstd, gamma)
    torch.cuda.synchronize()
    out = dict(y=y, h=h, mean=mean, rstd=rstd, dh=dh, dgamma=dgamma, dbeta=dbeta)
    for k, t in out.items():
        if t is not None:
            assert torch.isfinite(t.float()).all(), k
    assert y.dtype == dh.dtype == torch.bfloat16 and y.shape == dh.shape == x.shape
    assert dgamma.dtype == dbeta.dtype == mean.dtype == rstd.dtype == torch.float32
    assert dgamma.shape == dbeta.shape == gamma.shape and mean.shape == rstd.shape == (x.shape[0],)
    return out


@pytest.mark.parametrize("res", [False, True], ids=["plain", "residual"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_rows_vs_fp64(M, C, res):
    ins = make_inputs(M, C, res)
    out = run_raw(*ins)
    ref = reference(*ins)
    if res:
        assert _row_err(out["h"], ref["h"]) < 1e-2
    check(errors(out, ref), f"M={M} C={C} res={int(res)}")


def test_large_mean_rows():
    """x = 64 + randn: a one-pass variance E[x^2] - mean^2 loses the row's spread here (rstd
    off by 2e-4 and more); mean first, then the centred squares, does not.  Without a residual
    the backward reads x itself, so its bounds hold as well; with one, bf16 cannot hold the sum
    (steps of 0.5 at 64), so only what the forward computes from its fp32 sum is held."""
    for M, C in ((4, 131), (3, 2052), (3, 4096), (2, 16384)):
        ins = make_inputs(M, C, False, offset=64.0)
        check(errors(run_raw(*ins), reference(*ins)), f"mean 64: M={M} C={C}")
        ins = make_inputs(M, C, True, offset=64.0)
        e = errors(run_raw(*ins), reference(*ins))
        check({k: e[k] for k in ("y", "mean", "rstd")}, f"mean 64 + residual (forward): M={M} C={C}")


@pytest.mark.parametrize("M,C", [(5, 131), (3, 4096)])
def test_constant_row(M, C):
    """A row of equal values has variance 0: rstd = 1 / sqrt(eps), everything finite, and
    (the row's sum and its mean are exact for 3.25) y is beta rounded to bf16."""
    x, _, dy, gamma, beta = make_inputs(M, C, False)
    x[1] = 3.25
    out = run_raw(x, None, dy, gamma, beta)
    check(errors(out, reference(x, None, dy, gamma, beta)), f"constant row: M={M} C={C}")
    assert torch.equal(out["y"][1], beta.to(torch.bfloat16))
    assert abs(out["rstd"][1].item() * math.sqrt(EPS) - 1) < 1e-6 and out["mean"][1].item() == 3.25
    r = torch.zeros_like(x)
    out_r = run_raw(x, r, dy, gamma, beta)
    assert torch.equal(out_r["y"], out["y"]) and torch.equal(out_r["h"], x) and torch.equal(out_r["dh"], out["dh"])


def test_single_column():
    """C = 1: every row is its own mean, y is beta and no gradient reaches x."""
    x, r, dy, gamma, beta = make_inputs(5, 1, True)
    for res in (None, r):
        out = run_raw(x, res, dy, gamma, beta)
        assert torch.equal(out["y"], beta.to(torch.bfloat16).expand(5, 1))
        assert torch.equal(out["dh"], torch.zeros_like(out["dh"]))
        assert torch.equal(out["dgamma"], torch.zeros_like(gamma))
        assert rel(out["dbeta"], dy.double().sum(0)) < 1e-6
        h = x.float() if res is None else x.float() + res.float()
        assert torch.equal(out["mean"], h[:, 0])


def _shifted(t):
    """The same values one element (2 bytes) past an allocation's start."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 4 == 2 and v.is_contiguous()
    return v


@pytest.mark.parametrize("C", [128, 131])
def test_misaligned_base(C, monkeypatch):
    """x (and the residual, dy) sliced one element into their allocations: C = 128 must leave
    the tuned kernels, which read 8 bytes at a time; both widths give the aligned call's
    errors."""
    from cloud_amd.ops import raw

    tuned = []
    old = raw.ln_fwd
    monkeypatch.setattr(raw, "ln_fwd", lambda *a, **k: (tuned.append(1), old(*a, **k))[1])
    M = 9
    for res in (False, True):
        x, r, dy, gamma, beta = make_inputs(M, C, res)
        ref = reference(x, r, dy, gamma, beta)
        aligned = run_raw(x, r, dy, gamma, beta)
        assert len(tuned) == (1 if C == 128 else 0)
        del tuned[:]
        shifted = run_raw(_shifted(x), None if r is None else _shifted(r), _shifted(dy), gamma, beta)
        assert not tuned, "a 2-byte-aligned x may not reach the tuned kernels"
        ea, es = errors(aligned, ref), errors(shifted, ref)
        check(ea, f"aligned C={C} res={int(res)}")
        check(es, f"shifted C={C} res={int(res)}")
        if C == 131:  # the same kernels, the same lanes and order: only the addresses differ
            for k in ("y", "mean", "rstd", "dh", "dgamma", "dbeta"):
                assert torch.equal(aligned[k], shifted[k]), k


def test_tuned_widths_are_the_bert_kernels_bitwise():
    """(9, 384) with a residual runs the tuned pair: bit for bit raw.ln_fwd / raw.ln_bwd (the
    old backward accumulates, so it is given zero-filled accumulators)."""
    from cloud_amd.ops import raw

    x, r, dy, gamma, beta = make_inputs(9, 384, True)
    new = run_raw(x, r, dy, gamma, beta)
    y, h, mean, rstd = raw.ln_fwd(x, gamma, beta, EPS, residual=r)
    dg, db = torch.zeros_like(gamma), torch.zeros_like(beta)
    dh, _ = raw.ln_bwd(dy, h, mean, rstd, gamma, dg, db)
    torch.cuda.synchronize()
    for k, t in dict(y=y, h=h, mean=mean, rstd=rstd, dh=dh, dgamma=dg, dbeta=db).items():
        assert torch.equal(new[k], t), k


@pytest.mark.parametrize("M,C", [(2053, 131), (3, 4096)])
def test_two_calls_are_bitwise_equal(M, C):
    ins = make_inputs(M, C, True)
    a, b = run_raw(*ins), run_raw(*ins)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("M,C", [(5, 131), (3, 16383)])
def test_guards_after_the_outputs(M, C):
    """y, h, dh, mean and rstd are slices of larger allocations filled with a pattern: the
    entry points of the new kernels write M*C (M) elements and nothing before or after."""
    from cloud_amd.ops import _ext, raw

    ext = _ext.load(required=True)
    x, r, dy, gamma, beta = make_inputs(M, C, True)
    want = run_raw(x, r, dy, gamma, beta)
    G = 64

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * G,), fill, dtype=dtype, device=DEV)
        return buf, buf[G:G + n]

    bufs = {k: guarded(M * C, torch.bfloat16, -1234.0) for k in ("y", "h", "dh")}
    bufs.update({k: guarded(M, torch.float32, 7.5e8) for k in ("mean", "rstd")})
    o = {k: v[1] for k, v in bufs.items()}
    st = torch.cuda.current_stream().cuda_stream
    ext.layer_norm_fwd(x.data_ptr(), r.data_ptr(), gamma.data_ptr(), beta.data_ptr(), o["y"].data_ptr(),
                       o["h"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(), M, C, EPS, st)
    parts = ext.layer_norm_bwd_parts(M, C)
    assert ext.layer_norm_bwd_workspace_floats(M, C) == parts * 2 * C + M
    ws_buf, ws = guarded(parts * 2 * C + M, torch.float32, 7.5e8)
    ext.layer_norm_bwd(dy.data_ptr(), o["h"].data_ptr(), o["mean"].data_ptr(), o["rstd"].data_ptr(),
                       gamma.data_ptr(), o["dh"].data_ptr(), ws.data_ptr(), M, C, st)
    torch.cuda.synchronize()
    for k, (buf, view) in list(bufs.items()) + [("ws", (ws_buf, ws))]:
        fill = -1234.0 if buf.dtype == torch.bfloat16 else 7.5e8
        assert torch.equal(buf[:G], torch.full_like(buf[:G], fill)), f"{k}: written before the tensor"
        assert torch.equal(buf[-G:], torch.full_like(buf[-G:], fill)), f"{k}: written past the tensor"
    for k, v in o.items():
        assert torch.equal(v.view(want[k].shape), want[k]), k
    assert not (ws == 7.5e8).any(), "every partial and every row mean is written"
    assert rel(ws[:parts * 2 * C].view(parts, 2, C).sum(0)[0], want["dgamma"]) < 1e-6


def test_rejected_widths_raise_before_launch():
    from cloud_amd.ops import raw

    x = torch.zeros(2, 16385, dtype=torch.bfloat16, device=DEV)
    g = torch.ones(16385, device=DEV)
    with pytest.raises(ValueError):
        raw.layer_norm_fwd(x, g, g, EPS)
    with pytest.raises(ValueError):
        raw.layer_norm_bwd(x, x, torch.zeros(2, device=DEV), torch.ones(2, device=DEV), g)
    with pytest.raises(ValueError):
        raw.layer_norm_fwd(x[:, :64].float(), g[:64], g[:64], EPS)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------- ops.layer_norm


def test_op_autograd_nd_and_routing(monkeypatch):
    from cloud_amd import ops
    from cloud_amd.ops import raw

    calls = []
    fwd = raw.layer_norm_fwd
    monkeypatch.setattr(raw, "layer_norm_fwd", lambda *a, **k: (calls.append(tuple(a[0].shape)), fwd(*a, **k))[1])
    B, T, C = 3, 7, 131
    x, r, dy, gamma, beta = make_inputs(B * T, C, True)
    ref = reference(x, r, dy, gamma, beta)
    xs, rs = x.view(B, T, C).clone().requires_grad_(), r.view(B, T, C).clone().requires_grad_()
    gp, bp = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    y = ops.layer_norm(xs, gp, bp, eps=EPS, residual=rs)
    assert calls == [(B, T, C)] and y.shape == (B, T, C) and y.dtype == torch.bfloat16
    y.backward(dy.view(B, T, C))
    torch.cuda.synchronize()
    assert torch.equal(xs.grad, rs.grad)
    e = dict(y=_row_err(y.detach().view(-1, C), ref["y"]), dh=_row_err(xs.grad.view(-1, C), ref["dh"]),
             dgamma=rel(gp.grad, ref["dgamma"]), dbeta=rel(bp.grad, ref["dbeta"]))
    _say("op 3-D: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["y"] < Y_BOUND and e["dh"] < DH_BOUND and e["dgamma"] < DP_BOUND and e["dbeta"] < DP_BOUND, e

    # a transposed (non-contiguous) x is made contiguous; gamma = beta = None are ones / zeros
    xt = x.view(B, T, C).transpose(0, 1)
    assert not xt.is_contiguous()
    y0 = ops.layer_norm(xt.clone().requires_grad_(), eps=EPS)
    y1 = ops.layer_norm(xt.contiguous(), torch.ones(C, device=DEV), torch.zeros(C, device=DEV), eps=EPS)
    assert torch.equal(y0, y1) and len(calls) == 3
    y0.float().sum().backward()  # no parameter to hand a gradient to

    # rows wider than the kernels take, fp32 inputs and empty tensors run the reference expression
    del calls[:]
    wide = torch.randn(2, 16385, device=DEV).to(torch.bfloat16)
    assert torch.equal(ops.layer_norm(wide, eps=EPS), F.layer_norm(wide.float(), (16385,), None, None, EPS).to(wide.dtype))
    assert ops.layer_norm(x.float(), gamma, beta).dtype == torch.float32
    assert ops.layer_norm(x[:0], gamma, beta).shape == (0, C)
    assert not calls
    with pytest.raises(ValueError):
        ops.layer_norm(x, gamma[:5], beta)
    with pytest.raises(ValueError):
        ops.layer_norm(x, gamma, beta, residual=r.float())


# --------------------------------------------------------------------------- Keras


def _no_library_layer_norm(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("torch.nn.functional.layer_norm was reached")

    monkeypatch.setattr(torch.nn.functional, "layer_norm", boom)


def test_keras_transformer_block_stays_native(monkeypatch):
    """x -> MHA(2, 64) -> Add -> LayerNormalization -> Dense(gelu) -> Dense -> Add ->
    LayerNormalization under mixed_bfloat16: a training step with the library's layer_norm
    removed."""
    from cloud_amd import keras
    from cloud_amd.keras import engine, layers
    from cloud_amd.ops import raw

    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = raw.layer_norm_fwd, raw.layer_norm_bwd
    monkeypatch.setattr(raw, "layer_norm_fwd", lambda *a, **k: (calls.__setitem__("fwd", calls["fwd"] + 1), fwd(*a, **k))[1])
    monkeypatch.setattr(raw, "layer_norm_bwd", lambda *a, **k: (calls.__setitem__("bwd", calls["bwd"] + 1), bwd(*a, **k))[1])
    old = engine._POLICY
    engine.set_global_policy("mixed_bfloat16")
    try:
        torch.manual_seed(0)
        T, DIM = 16, 128
        inp = keras.Input(shape=(T, DIM))
        a = layers.MultiHeadAttention(2, 64)([inp, inp])
        h1 = layers.LayerNormalization(name="ln1")(layers.Add()([inp, a]))
        f = layers.Dense(DIM)(layers.Dense(4 * DIM, activation="gelu")(h1))
        out = layers.LayerNormalization(name="ln2")(layers.Add()([h1, f]))
        model = keras.Model(inp, out)
        rs = np.random.RandomState(0)
        x = rs.randn(2, T, DIM).astype(np.float32)
        y = rs.randn(2, T, DIM).astype(np.float32)
        model.compile(optimizer="adam", loss="mse")
        lns = [model.get_layer("ln1"), model.get_layer("ln2")]
        _no_library_layer_norm(monkeypatch)
        hist = model.fit(x, y, batch_size=2, epochs=1, verbose=0)
        torch.cuda.synchronize()
        assert math.isfinite(hist.history["loss"][0])
        assert calls == {"fwd": 2, "bwd": 2}, calls
        for ln in lns:
            assert ln.gamma.dtype == torch.float32 and ln.gamma.is_cuda
            assert not torch.equal(ln.gamma.detach().cpu(), torch.ones(DIM)), "gamma received no update"
            assert not torch.equal(ln.beta.detach().cpu(), torch.zeros(DIM)), "beta received no update"
    finally:
        engine._POLICY = old


def test_keras_layer_vs_fp64(monkeypatch):
    from cloud_amd.keras import layers

    B, T, C = 2, 16, 128
    x, _, dy, gamma, beta = make_inputs(B * T, C, False)
    ref = reference(x, None, dy, gamma, beta)  # (the library's layer_norm, in fp64)
    _no_library_layer_norm(monkeypatch)
    layer = layers.LayerNormalization(epsilon=EPS, dtype="mixed_bfloat16")
    xs = x.view(B, T, C).clone().requires_grad_()
    layer._maybe_build((None, T, C), torch.device(DEV))
    with torch.no_grad():
        layer.gamma.copy_(gamma)
        layer.beta.copy_(beta)
    y = layer(xs, training=True)
    assert y.dtype == torch.bfloat16
    y.backward(dy.view(B, T, C))
    torch.cuda.synchronize()
    e = dict(y=_row_err(y.detach().view(-1, C), ref["y"]), dh=_row_err(xs.grad.view(-1, C), ref["dh"]),
             dgamma=rel(layer.gamma.grad, ref["dgamma"]), dbeta=rel(layer.beta.grad, ref["dbeta"]))
    _say("keras layer: " + " ".join(f"{k} {v:.3e}" for k, v in e.items()))
    assert e["y"] < Y_BOUND and e["dh"] < DH_BOUND and e["dgamma"] < DP_BOUND and e["dbeta"] < DP_BOUND, e
