"""Edge-case reference tests for the BERT-path kernels: attention (attn.hip), LayerNorm
(rowops.hip), softmax cross-entropy (xent.hip) and the classifier head (head.hip).

Every reference is computed in float64 from the same bf16 / fp32 inputs the kernel reads;
dropout references take the kernels' own keep-mask from ``raw.dropout_mask`` with the
kernel's element index.  The shapes are the smallest that enter the dispatch branches the
older tests never reach: key blocks entirely past ``key_len``, key loops shorter than
S / 64 (S / 32 in the fused backward), ``key_len`` 1 and on / next to the 16 / 32 / 64
boundaries, the LayerNorm backward's second grid-stride trip, the NV = 2 and NV = 8
LayerNorm instantiations, label smoothing, ignored labels, strided logits, the LM = 16
head instantiation and the head's dropout path.

Metrics are local, not one norm over the whole tensor: attention errors are taken per
(batch, head) block, LayerNorm errors per row, the head's bf16 output per element, so one
wrong slab or one wrong trailing row cannot hide behind the rest of the tensor.

Worst errors observed on an MI355X (each test prints its figures before asserting):

    group                                               worst observed   bound
    attention long path    ctx / block                  2.44e-3          1e-2
    attention long path    dQ, dK, dV / block           2.61e-3          2e-2
    attention long path    dQ / dK, key_len = 1, p > 0  2.92e-2 / 3.11e-2  8.8e-2 / 9.3e-2 (*)
    attention short path   ctx / block                  2.59e-3          1e-2
    attention short path   dQ, dK, dV / block           2.86e-3          2e-2
    attention short path   dQ / dK, key_len = 1, p > 0  1.28e-2 / 1.74e-2  2e-2
    attention scale = 0.2  ctx / dqkv per block         2.35e-3 / 2.76e-3  1e-2 / 2e-2
    attention generic path at S <= 128, ctx / dqkv      2.34e-3 / 3.07e-3  1e-2 / 2e-2
    attention lse (log2 domain, absolute)               9.97e-7          1e-3
    LayerNorm y / row                                   2.19e-3          1e-2
    LayerNorm dh, dx / row                              2.35e-3          2e-2
    LayerNorm mean / rstd vs fp64 row statistics        4.2e-8 / 1.4e-7  1e-5
    head logits, gwc, gbc (relative norm)               1.26e-6          1e-5
    head dpre / element, |got - ref| / (2^-8 |ref| + 1e-6)   0.995       1

(*) the one bound that is not the project's own: see test_attention_long_path_key_len_edges.
The kernel's per-block errors equal those of a bf16-faithful fp32 emulation of the same
inputs to three digits (dQ 2.887e-2 / 2.924e-2, dK 3.055e-2 / 3.114e-2 in both).
"""
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _say(*a):
    print("[edges]", *a, flush=True)


def rel(a, b):
    return ((a.double() - b.double()).norm() / (b.double().norm() + 1e-300)).item()


# --------------------------------------------------------------------------- attention

CTX_BOUND, DQKV_BOUND, LSE_BOUND = 1e-2, 2e-2, 1e-3


def _attn_inputs(B, S, H, seed=1):
    g = torch.Generator().manual_seed(seed)  # host generator: the same inputs on every machine
    C = H * 64
    qkv = (torch.randn(B * S, 3 * C, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B * S, C, generator=g).to(torch.bfloat16)
    return qkv.to(DEV), dctx.to(DEV)


def _attn_ref(qkv, dctx, B, S, H, key_len, p, seed, scale):
    """fp64 attention of the bf16 inputs.  Returns ctx [B,H,S,64], grads [3,B,H,S,64] (Q, K,
    V) and the log2-domain log-sum-exp [B,H,S] of the masked, scaled scores."""
    from cloud_amd.ops import raw

    kl = torch.full((B,), S, device=DEV) if key_len is None else key_len.long().clamp(1, S)
    q_, k_, v_ = qkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = [t.clone().requires_grad_() for t in (q_, k_, v_)]
    sc = (q @ k.transpose(-1, -2)) * scale
    keymask = torch.arange(S, device=DEV)[None, :] >= kl[:, None]
    sc = sc.masked_fill(keymask[:, None, None, :], float("-inf"))
    lse2 = (torch.logsumexp(sc, -1) / math.log(2.0)).detach()
    att = sc.softmax(-1)
    if p > 0:
        keep = raw.dropout_mask(B * H * S * S, p, seed).view(B, H, S, S).double()
        att = att * keep / (1.0 - p)
    out = att @ v
    out.backward(dctx.double().view(B, S, H, 64).permute(0, 2, 1, 3))
    return out.detach(), torch.stack([q.grad, k.grad, v.grad], 0), lse2, kl


def _block_err(got, ref):
    """Per (batch, head) block: ||got - ref|| / max(||ref||, median block ||ref||); the median
    is over the blocks of the same tensor (for dqkv: of the same Q / K / V third).  The floor
    is what makes a block whose true value is exactly zero (dQ / dK at key_len = 1)
    measurable."""
    d = (got - ref).flatten(-2).norm(dim=-1)  # [..., B, H]
    n = ref.flatten(-2).norm(dim=-1)
    med = torch.quantile(n.flatten(-2), 0.5, dim=-1)
    assert (med > 0).all(), "median block norm is zero: too many key_len = 1 rows in this case"
    return d / torch.maximum(n, med[..., None, None])


def _attn_case(S, key_len, p, H=2, scale=None, tag="attn", zero_block_bounds=None):
    """Run forward + backward once and hold every output to the fp64 reference.
    ``zero_block_bounds`` = (dQ bound, dK bound) for the blocks of batch entries with
    key_len = 1 (see test_attention_long_path_key_len_edges); every other block keeps
    DQKV_BOUND."""
    from cloud_amd.ops import raw

    B = len(key_len)
    assert sum(1 for v in key_len if v <= 1) * 2 < B
    qkv, dctx = _attn_inputs(B, S, H)
    kl_t = torch.tensor(key_len, dtype=torch.int32, device=DEV)
    seed = 1234
    ctx, lse = raw.attn_fwd(qkv, B, S, H, kl_t, p, seed, scale=scale)
    dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl_t, p, seed, scale=scale)
    torch.cuda.synchronize()
    ctx_r, dqkv_r, lse_r, kl = _attn_ref(qkv, dctx, B, S, H, kl_t, p, seed, 0.125 if scale is None else scale)

    ctx_g = ctx.double().view(B, S, H, 64).permute(0, 2, 1, 3)
    dqkv_g = dqkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    e_ctx = _block_err(ctx_g, ctx_r)
    e_d = _block_err(dqkv_g, dqkv_r)
    e_lse = (lse.double() - lse_r).abs().max().item()
    _say(f"{tag} S={S} key_len={key_len} p={p} scale={scale}: ctx/block max {e_ctx.max().item():.3e} "
         f"dq {e_d[0].max().item():.3e} dk {e_d[1].max().item():.3e} dv {e_d[2].max().item():.3e} "
         f"lse abs {e_lse:.3e}")
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(dqkv.float()).all() and torch.isfinite(lse).all()
    # keys at or past key_len take no part: their dK / dV rows are exactly zero
    pad = (torch.arange(S, device=DEV)[None, :] >= kl[:, None])[None, :, None, :, None].expand(2, B, H, S, 64)
    assert pad.any() or all(v >= S for v in key_len)
    assert (dqkv_g[1:][pad] == 0).all(), "dK / dV rows of masked keys must be exactly zero"
    assert e_lse < LSE_BOUND, e_lse
    assert e_ctx.max().item() < CTX_BOUND, e_ctx
    bound = torch.full_like(e_d, DQKV_BOUND)
    if zero_block_bounds is not None:
        one = kl == 1
        bound[0][one] = zero_block_bounds[0]
        bound[1][one] = zero_block_bounds[1]
        _say(f"{tag} key_len = 1 blocks: dq {e_d[0][one].flatten().tolist()} dk {e_d[1][one].flatten().tolist()}")
    assert (e_d < bound).all(), e_d
    return e_ctx.max().item(), e_d.max().item()


@pytest.mark.parametrize("S,key_len,p", [
    (192, [192, 128, 65, 64], 0.0), (192, [192, 128, 65, 64], 0.1),
    (192, [17, 1, 129, 192], 0.0), (192, [17, 1, 129, 192], 0.1),
    (256, [256, 1, 64, 200], 0.0),
])
def test_attention_long_path_key_len_edges(S, key_len, p):
    """S > 128: online-softmax forward and the three-kernel backward.  The key_len sets reach
    64-key blocks entirely past key_len in the dK/dV kernel (zeros staged and stored) and
    every key-loop length from 1 to S / 64 in the forward and dQ kernels.

    One bound is not the project's 2e-2: key_len = 1 WITH dropout (S = 192, key_len
    [17, 1, 129, 192], p = 0.1, the two blocks of batch entry 1).  There the true dQ and dK
    are zero, and what a correct kernel stores is the bf16 rounding of the context inside
    Dv = rowsum(dO * ctx): dS = P (dP * mask - Dv) no longer cancels exactly once ctx =
    bf16(V / (1 - p)) is rounded.  A bf16-faithful fp32 emulation of these very inputs (P *
    mask and dS rounded to bf16 before their matmuls; ctx, dQ, dK, dV rounded to bf16; the
    same dropout hash) gives, relative to the median block norm, dQ 2.89e-2 / 2.92e-2 and dK
    3.06e-2 / 3.11e-2 on those two blocks (2.1e-3 .. 2.5e-3 on every other block of every case
    in this module; 1.3e-2 / 1.7e-2 for the same situation at S = 128, which stays inside
    2e-2).  Those blocks are held to 3 x the emulation: dQ 8.8e-2, dK 9.3e-2 (the margin covers
    summation order and exp2f).  Measured on the kernel: dQ 2.887e-2 /
    2.924e-2, dK 3.055e-2 / 3.114e-2 -- the emulation's figures."""
    zb = (8.8e-2, 9.3e-2) if (p > 0 and 1 in key_len) else None
    _attn_case(S, key_len, p, tag="attn-long", zero_block_bounds=zb)


@pytest.mark.parametrize("S,key_len,p", [
    (128, [128, 33, 32, 31], 0.0), (128, [128, 33, 32, 31], 0.1),
    (128, [17, 16, 1, 127], 0.0), (128, [17, 16, 1, 127], 0.1),
    (64, [64, 1, 33], 0.0),
])
def test_attention_short_path_key_len_edges(S, key_len, p):
    """S = 64 / 128: one-workgroup forward and fused backward; the dQ phase's 32-key loop
    runs 1 .. S / 32 trips, key_len sits on and next to the 16 / 32 boundaries."""
    _attn_case(S, key_len, p, tag="attn-short")


@pytest.mark.parametrize("S", [64, 192])
def test_attention_key_len_and_scale_contract(S):
    """key_len=None means all keys; key_len is clamped to [1, S] (an all-padding row of
    attention_mask sums to 0); a non-default scale reaches every kernel."""
    from cloud_amd.ops import raw

    B, H, p, seed = 2, 2, 0.1, 77
    qkv, dctx = _attn_inputs(B, S, H, seed=3)

    def run(kl):
        kl_t = None if kl is None else torch.tensor(kl, dtype=torch.int32, device=DEV)
        ctx, lse = raw.attn_fwd(qkv, B, S, H, kl_t, p, seed)
        dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl_t, p, seed)
        return ctx, lse, dqkv

    for a, b in ((None, [S, S]), ([0, S + 5], [1, S])):
        for x, y in zip(run(a), run(b)):
            assert torch.equal(x, y), (a, b)
    _attn_case(S, [S, S - 21, 7], 0.1, scale=0.2, tag="attn-scale")


_GENERIC_CHECK = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import test_bert_kernel_edges_gpu as T
T._attn_case(128, [128, 40, 1, 64], 0.0, tag="attn-generic")
T._attn_case(64, [64, 5], 0.0, tag="attn-generic")
print("GENERIC_OK")
"""


def test_attention_generic_path_at_short_sequences():
    """CLOUD_AMD_ATTN_FUSED_BWD=0 sends S <= 128 to the generic forward and the three-kernel
    backward.  The switch is read once per process, so the check runs in its own
    interpreter, against the same reference and bounds."""
    tests = os.path.dirname(os.path.abspath(__file__))
    root = os.path.dirname(tests)
    env = dict(os.environ, CLOUD_AMD_ATTN_FUSED_BWD="0")
    r = subprocess.run([sys.executable, "-c", _GENERIC_CHECK.format(root=root, tests=tests)], env=env,
                       capture_output=True, text=True, timeout=110)
    print(r.stdout)
    assert r.returncode == 0 and "GENERIC_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


# --------------------------------------------------------------------------- LayerNorm


def _row_err(got, ref):
    return ((got.double() - ref).norm(dim=-1) / ref.norm(dim=-1).clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("M,C,res,p_in,p_out,xb", [
    (2053, 128, True, 0.1, 0.0, True),    # second grid-stride trip, ragged tail
    (2049, 768, True, 0.0, 0.1, False),   # second trip at BERT's width
    (9, 384, True, 0.1, 0.0, False),      # NV = 2
    (5, 1280, False, 0.0, 0.1, True),     # NV = 8 (default: branch)
    (5, 1344, True, 0.0, 0.0, False),     # the backward's upper bound
    (3, 4, False, 0.0, 0.0, False),       # one vector
])
def test_layernorm_rows_vs_fp64(M, C, res, p_in, p_out, xb):
    """Every row of y / dh / dx against an fp64 LayerNorm of the same inputs (the tolerances
    of test_layernorm_fwd_bwd, applied per row), fp32 row statistics against fp64 ones,
    dgamma / dbeta / dsum accumulated into pre-filled buffers."""
    from cloud_amd.ops import raw

    torch.manual_seed(2)
    x = torch.randn(M, C, device=DEV).to(torch.bfloat16)
    r = torch.randn(M, C, device=DEV).to(torch.bfloat16) if res else None
    g = torch.randn(C, device=DEV) * 0.5 + 1
    b = torch.randn(C, device=DEV) * 0.1
    xbias = torch.randn(C, device=DEV) * 0.3 if xb else None
    s_in, s_out, eps = 77, 78, 1e-12
    y, h, mu, rs = raw.ln_fwd(x, g, b, eps, residual=r, p_in=p_in, seed_in=s_in, p_out=p_out, seed_out=s_out,
                              x_bias=xbias)
    assert (h is not None) == (res or p_in > 0 or xb)
    dy = torch.randn_like(y)
    dg = torch.full((C,), 0.25, device=DEV)  # accumulate semantics
    db = torch.ones(C, device=DEV)
    dsum = torch.full((C,), 0.5, device=DEV)
    hh = h if h is not None else x
    dh, dx = raw.ln_bwd(dy, hh, mu, rs, g, dg, db, p_in=p_in, seed_in=s_in, p_out=p_out, seed_out=s_out,
                        want_dx=True, dsum=dsum)
    torch.cuda.synchronize()

    xr = x.double().requires_grad_()
    gr, br = g.double().requires_grad_(), b.double().requires_grad_()
    t = xr if xbias is None else xr + xbias.double()
    if p_in > 0:
        t = t * raw.dropout_mask(M * C, p_in, s_in).view(M, C).double() / (1 - p_in)
    if r is not None:
        t = t + r.double()
    t.retain_grad()
    yr = F.layer_norm(t, (C,), gr, br, eps)
    if p_out > 0:
        yr = yr * raw.dropout_mask(M * C, p_out, s_out).view(M, C).double() / (1 - p_out)
    yr.backward(dy.double())
    td = t.detach()
    mu_r = td.mean(-1)
    sd_r = (td.var(-1, unbiased=False) + eps).sqrt()

    e_y, e_dh, e_dx = _row_err(y, yr.detach()), _row_err(dh, t.grad), _row_err(dx, xr.grad)
    e_dg, e_db = rel(dg - 0.25, gr.grad), rel(db - 1, br.grad)
    e_ds = rel(dsum - 0.5, xr.grad.sum(0))
    # the mean's natural scale is the row's standard deviation (a row mean can sit next to 0)
    e_mu = ((mu.double() - mu_r).abs() / torch.maximum(mu_r.abs(), sd_r)).max().item()
    e_rs = ((rs.double() * sd_r) - 1).abs().max().item()
    _say(f"ln M={M} C={C}: y/row {e_y:.3e} dh/row {e_dh:.3e} dx/row {e_dx:.3e} dgamma {e_dg:.3e} "
         f"dbeta {e_db:.3e} dsum {e_ds:.3e} mu {e_mu:.3e} rstd {e_rs:.3e}")
    for o in (y, dh, dx, dg, db, dsum, mu, rs):
        assert torch.isfinite(o.float()).all()
    if h is not None:
        assert _row_err(h, td) < 1e-2
    assert e_mu < 1e-5 and e_rs < 1e-5, (e_mu, e_rs)
    assert e_y < 1e-2, e_y
    assert e_dh < 2e-2, e_dh
    assert e_dx < 2e-2, e_dx
    assert e_dg < 1e-2 and e_db < 1e-2, (e_dg, e_db)
    assert e_ds < 2e-2, e_ds


def test_layernorm_rejects_unsupported_widths():
    """Widths the kernels cannot take raise before anything is launched: the accumulators
    handed to the backward are untouched and the stream is healthy afterwards."""
    from cloud_amd.ops import raw

    def fwd(C):
        x = torch.randn(4, C, device=DEV).to(torch.bfloat16)
        return raw.ln_fwd(x, torch.ones(C, device=DEV), torch.zeros(C, device=DEV), 1e-12)

    def bwd(C):
        dy = torch.randn(4, C, device=DEV).to(torch.bfloat16)
        hh = torch.randn(4, C, device=DEV).to(torch.bfloat16)
        mu, rs = torch.zeros(4, device=DEV), torch.ones(4, device=DEV)
        acc = [torch.full((C,), v, device=DEV) for v in (0.25, 1.0, 0.5)]
        with pytest.raises(RuntimeError):
            raw.ln_bwd(dy, hh, mu, rs, torch.ones(C, device=DEV), acc[0], acc[1], want_dx=True, dsum=acc[2])
        torch.cuda.synchronize()
        for t, v in zip(acc, (0.25, 1.0, 0.5)):
            assert torch.equal(t, torch.full_like(t, v))

    for C in (2052, 6):
        with pytest.raises(RuntimeError):
            fwd(C)
    for C in (1348, 6):
        bwd(C)
    torch.cuda.synchronize()
    y, _, mu, rs = fwd(1348)  # the forward alone takes rows up to 2048 wide
    assert torch.isfinite(y.float()).all()


# --------------------------------------------------------------------------- softmax cross-entropy

ROW_KERNEL_SHAPE = (130, 1009)  # B * C > 2^17: the row-parallel kernel; B % 4 != 0, C % 64 != 0
BATCH_KERNEL_SHAPES = [(1, 2), (17, 10), (33, 130), (64, 1000)]
ACC0 = (1.5, 2.0, 3.0)


def _xent_run(z, y, ls, denom, grad_mult, pad=0):
    """One forward + backward through ops.softmax_cross_entropy.  pad > 0: the logits are the
    [:, :C] view of a [B, C + pad] leaf (the padded-head view).  grad_mult None: backward
    seeded with unit_seed (the stored gradient is handed on as is); else backward of
    grad_mult * loss."""
    from cloud_amd.ops import softmax_cross_entropy
    from cloud_amd.ops.losses import unit_seed

    B, C = z.shape
    if pad:
        leaf = torch.zeros(B, C + pad, dtype=z.dtype, device=DEV)
        leaf[:, :C] = z
        leaf[:, C:] = 100.0  # would win every argmax / dominate every sum if it were read
        leaf.requires_grad_()
        zz = leaf[:, :C]
        assert zz.stride(0) == C + pad
    else:
        leaf = z.clone().requires_grad_()
        zz = leaf
    acc = torch.tensor(ACC0, device=DEV)
    loss, correct = softmax_cross_entropy(zz, y, denom=denom, label_smoothing=ls, acc=acc, acc_weight=0.5)
    if grad_mult is None:
        torch.autograd.backward(loss, grad_tensors=unit_seed(loss.device))
    else:
        (grad_mult * loss).backward()
    grad = leaf.grad
    if pad:
        assert torch.equal(grad[:, C:], torch.zeros_like(grad[:, C:]))
        grad = grad[:, :C].contiguous()
    return loss.detach(), correct, grad, acc


def _xent_check(z, y, ls, tag=""):
    """Loss, correct flags, both backward forms and the metric accumulator against fp64."""
    B, C = z.shape
    denom = 2 * B
    tol = 2e-2 if z.dtype == torch.bfloat16 else 1e-5
    zd = z.double()
    valid = (y >= 0) & (y < C)
    zr = zd.clone().requires_grad_()
    per = F.cross_entropy(zr[valid], y[valid], reduction="none", label_smoothing=ls)
    (per.sum() / denom).backward()
    ref_loss, ref_grad = (per.sum() / denom).detach(), zr.grad
    # smallest index among the row's maxima, spelled out
    cols = torch.arange(C, device=DEV).expand(B, C)
    first = torch.where(zd == zd.max(-1, keepdim=True).values, cols, torch.full_like(cols, C)).min(-1).values
    ref_correct = ((first == y) & valid).float()
    ref_acc = torch.tensor(ACC0, device=DEV).double() + 0.5 * torch.stack(
        [per.sum().detach(), ref_correct.sum().double(), torch.tensor(float(B), device=DEV).double()])

    loss, correct, g1, acc = _xent_run(z, y, ls, denom, None)
    loss3, correct3, g3, _ = _xent_run(z, y, ls, denom, 3.0)
    torch.cuda.synchronize()
    _say(f"xent{tag} B={B} C={C} {z.dtype} ls={ls}: loss err {(loss.double() - ref_loss).abs().item():.3e} "
         f"grad max abs err * denom {((g1.double() - ref_grad).abs().max() * denom).item():.3e}")
    torch.testing.assert_close(loss.double(), ref_loss, atol=1e-3, rtol=1e-3)
    assert torch.equal(loss, loss3) and torch.equal(correct, correct3)
    assert torch.equal(correct, ref_correct)
    torch.testing.assert_close(g1.double(), ref_grad, atol=tol / denom, rtol=tol)
    torch.testing.assert_close(g3.double(), 3 * ref_grad, atol=tol / denom, rtol=tol)
    assert torch.equal(g1[~valid], torch.zeros_like(g1[~valid]))
    assert torch.equal(g3[~valid], torch.zeros_like(g3[~valid]))
    torch.testing.assert_close(acc[0].double(), ref_acc[0], atol=1e-3, rtol=1e-3)
    assert acc[1].item() == ref_acc[1].item() and acc[2].item() == ref_acc[2].item(), (acc, ref_acc)
    return loss, correct, g1, acc


def _xent_inputs(B, C, dtype, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = (torch.randn(B, C, device=DEV, generator=g) * 3).to(dtype)
    y = torch.randint(0, C, (B,), device=DEV, generator=g)
    return z, y


@pytest.mark.parametrize("B,C", [ROW_KERNEL_SHAPE] + BATCH_KERNEL_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_softmax_xent_vs_fp64(B, C, dtype, ls):
    """Both kernels, both dtypes, label smoothing, denom = 2B, unit-seed and scaled backward,
    in-kernel metric accumulation with a weight."""
    z, y = _xent_inputs(B, C, dtype)
    _xent_check(z, y, ls)


@pytest.mark.parametrize("B,C", [ROW_KERNEL_SHAPE] + BATCH_KERNEL_SHAPES[1:])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_softmax_xent_ignored_labels(B, C, dtype):
    """Labels -1 and C in a third of the rows: zero loss, zero correct, zero gradient, yet
    counted in denom and in acc[2]."""
    z, y = _xent_inputs(B, C, dtype, seed=2)
    y[1::6] = -1
    y[4::6] = C
    assert ((y < 0) | (y >= C)).sum().item() >= B // 3 - 1
    for ls in (0.0, 0.1):
        _, correct, _, _ = _xent_check(z, y, ls, tag="-ignored")
        assert correct[1::6].sum().item() == 0 and correct[4::6].sum().item() == 0


@pytest.mark.parametrize("B,C", [ROW_KERNEL_SHAPE, (33, 130)])
def test_softmax_xent_large_magnitude_fp32(B, C):
    """Logits of magnitude 60: exp() of the raw values overflows fp32, the max-subtracted
    form does not."""
    g = torch.Generator(device=DEV).manual_seed(3)
    sign = torch.randint(0, 2, (B, C), device=DEV, generator=g).float() * 2 - 1
    z = sign * 60 + torch.randn(B, C, device=DEV, generator=g)
    y = torch.randint(0, C, (B,), device=DEV, generator=g)
    for ls in (0.0, 0.1):
        _xent_check(z, y, ls, tag="-mag60")


@pytest.mark.parametrize("B,C", [ROW_KERNEL_SHAPE, (17, 10), (33, 130)])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_softmax_xent_tied_maxima(B, C, dtype):
    """Duplicated row maxima (in one lane's stride and across lanes): `correct` goes to the
    smallest index."""
    z, y = _xent_inputs(B, C, dtype, seed=4)
    top = z.float().max().item() + 1.0
    for row in range(B):
        a = (row * 7) % C
        b = (a + (64 if row % 2 and C > 64 else 3)) % C
        z[row, a] = top
        z[row, b] = top
        y[row] = (min(a, b), max(a, b), (a + 1) % C)[row % 3]  # first max, second max, neither
    _, correct, _, _ = _xent_check(z, y, 0.0, tag="-ties")
    assert correct[0::3].sum().item() == len(range(0, B, 3)) and correct[1::3].sum().item() == 0


@pytest.mark.parametrize("B,C", BATCH_KERNEL_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_softmax_xent_strided_logits(B, C, dtype):
    """The padded-head view big[:, :C] of a [B, C + 6] tensor goes to the one-block kernel
    without a copy and gives bitwise the results of the contiguous logits."""
    z, y = _xent_inputs(B, C, dtype, seed=5)
    if B > 2:
        y[1] = -1
    for ls in (0.0, 0.1):
        for mult in (None, 3.0):
            a = _xent_run(z, y, ls, 2 * B, mult)
            b = _xent_run(z, y, ls, 2 * B, mult, pad=6)
            for u, v in zip(a, b):
                assert torch.equal(u, v)
        _xent_check(z, y, ls, tag="-contig-of-strided")


# --------------------------------------------------------------------------- classifier head


def _head_case(B, C, L, p, strided, seed):
    from cloud_amd.ops import raw

    g = torch.Generator(device=DEV).manual_seed(seed)
    S = 3
    if strided:
        hbuf = torch.tanh(torch.randn(B * S, C, device=DEV, generator=g)).to(torch.bfloat16)
        pooled = hbuf.view(B, S, C)[:, 0]
        assert pooled.stride(0) == S * C
    else:
        pooled = torch.tanh(torch.randn(B, C, device=DEV, generator=g)).to(torch.bfloat16)
    wc = torch.randn(L, C, device=DEV, generator=g) * 0.05
    bc = torch.randn(L, device=DEV, generator=g) * 0.1
    dl = torch.randn(B, L, device=DEV, generator=g)
    gwc0 = torch.randn(L, C, device=DEV, generator=g) * 0.5
    gbc0 = torch.randn(L, device=DEV, generator=g) * 0.5
    drop_seed = 4321

    def run():
        logits = raw.cls_head_fwd(pooled, wc, bc, p, drop_seed)
        gwc, gbc = gwc0.clone(), gbc0.clone()
        dpre = raw.cls_head_bwd(dl, pooled, wc, gwc, gbc, p, drop_seed)
        return logits, dpre, gwc, gbc

    out = run()
    again = run()
    torch.cuda.synchronize()
    for u, v in zip(out, again):
        assert torch.equal(u, v), "the head kernels claim a fixed summation order"
    logits, dpre, gwc, gbc = out

    y = pooled.double()
    if p > 0:
        scale = 1.0 / (1.0 - torch.tensor(p, dtype=torch.float32).double().item())
        m = raw.dropout_mask(B * C, p, drop_seed).view(B, C).double() * scale
    else:
        m = torch.ones(B, C, dtype=torch.float64, device=DEV)
    dld, wcd = dl.double(), wc.double()
    logits_r = (y * m) @ wcd.t() + bc.double()
    dpre_r = (dld @ wcd) * m * (1 - y * y)
    gwc_r = dld.t() @ (y * m)
    gbc_r = dld.sum(0)

    e_lo, e_gw, e_gb = rel(logits, logits_r), rel(gwc - gwc0, gwc_r), rel(gbc - gbc0, gbc_r)
    err = (dpre.double() - dpre_r).abs()
    ulps = (err / (2.0 ** -8 * dpre_r.abs() + 1e-6)).max().item()
    assert torch.isfinite(logits).all() and torch.isfinite(dpre.float()).all()
    assert e_lo < 1e-5 and e_gw < 1e-5 and e_gb < 1e-5, (B, C, L, p, strided, e_lo, e_gw, e_gb)
    assert ulps <= 1.0, (B, C, L, p, strided, ulps)
    return max(e_lo, e_gw, e_gb), ulps


@pytest.mark.parametrize("L", [1, 4, 5, 16])
@pytest.mark.parametrize("B", [1, 5, 33])
def test_cls_head_vs_fp64(L, B):
    """Both label-count instantiations (L <= 4, L <= 16), with and without dropout, pooled
    contiguous and as the strided [CLS]-row view, gwc / gbc accumulated into pre-filled
    buffers, two identical calls bitwise equal."""
    worst_f, worst_u = 0.0, 0.0
    for C in (64, 300, 768):
        for p in (0.0, 0.1):
            for strided in (False, True):
                f, u = _head_case(B, C, L, p, strided, seed=100 * L + B)
                worst_f, worst_u = max(worst_f, f), max(worst_u, u)
    _say(f"head L={L} B={B}: fp32 outputs rel {worst_f:.3e}, dpre {worst_u:.3f} ulp")


def test_cls_head_rejects_too_many_labels():
    from cloud_amd.ops import raw

    B, C, L = 4, 64, 17
    pooled = torch.zeros(B, C, dtype=torch.bfloat16, device=DEV)
    wc, bc = torch.zeros(L, C, device=DEV), torch.zeros(L, device=DEV)
    with pytest.raises(RuntimeError):
        raw.cls_head_fwd(pooled, wc, bc)
    gwc, gbc = torch.ones(L, C, device=DEV), torch.ones(L, device=DEV)
    with pytest.raises(RuntimeError):
        raw.cls_head_bwd(torch.ones(B, L, device=DEV), pooled, wc, gwc, gbc)
    torch.cuda.synchronize()
    assert torch.equal(gwc, torch.ones_like(gwc)) and torch.equal(gbc, torch.ones_like(gbc))
