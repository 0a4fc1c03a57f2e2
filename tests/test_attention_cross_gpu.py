"""Cross-attention kernels of attn.hip (``raw.attn_cross_fwd`` / ``raw.attn_cross_bwd``) and
``ops.cross_attention``: T queries ``q [B*T, H*64]`` against S keys / values ``kv [B*S, 2*H*64]``
(``K | V``), T and S independent, ``key_len`` a prefix mask, dropout element index
``(b*H + h)*T*S + q*S + key``.

Inputs follow test_bert_kernel_edges_gpu._attn_inputs (seeded host generator, ``randn * 0.5`` in
bf16, ``dctx = randn``); the per-(batch, head) block metric ``_block_err`` and the bounds
(CTX_BOUND 1e-2, DQKV_BOUND 2e-2, LSE_BOUND 1e-3) are imported from that module.  They carry over
because the kernels are the non-causal generic self-attention kernels with the query rows and
the key / value rows taken apart: with T == S on views of one packed tensor they store the same
bits (test_cross_equals_self_attention_bitwise).  Beyond the bounds the new indexing is held to
bitwise statements: pitched operands equal contiguous ones, the tail variant equals zero
padding, key blocks past ``key_len`` are not read, batch entries do not see each other.

The cases avoid ``key_len = 1`` together with dropout and rows with 2 - 4 visible keys: there
dS = P (dP - Dv) cancels and the bf16 rounding of the context dominates (the (*) notes of
test_bert_kernel_edges_gpu and test_attention_causal_gpu).

T = S = 1 is the one case the block metric cannot take for dQ and dK: the only probability is
1, so both are exactly zero in every block and the metric's median floor is zero.  There they
are held to DQKV_BOUND of the magnitude of the terms that cancel, scale * |dO| |V| |K| per block
(what dQ would be if dP - Dv did not cancel); ctx, dV and the log-sum-exp keep the metric.

Worst per-block figures observed on an MI355X (each test prints its own before asserting):

    T    S    key_len              p     ctx       dQ        dK        dV        lse abs
    1    1    None                 0     0         3.4e-9    3.4e-9    0         1.1e-8    (dQ, dK: see above)
    1    200  [200, 65, 7]         0     2.60e-3   2.42e-3   2.58e-3   2.65e-3   4.5e-7
    2    65   [65, 64, 17]         0.1   2.59e-3   2.65e-3   2.56e-3   2.46e-3   4.9e-7
    64   64   [64, 33, 17]         0     2.33e-3   2.45e-3   2.49e-3   2.57e-3   8.0e-7
    64   128  [128, 1, 65, 64]     0     2.45e-3   2.36e-3   2.38e-3   2.31e-3   7.9e-7
    128  64   [64, 5, 33]          0.1   2.39e-3   2.69e-3   2.82e-3   2.66e-3   7.6e-7
    65   63   [63, 17, 62]         0.1   2.42e-3   2.44e-3   2.46e-3   2.50e-3   7.5e-7
    63   129  [129, 128, 1, 65]    0     2.48e-3   2.36e-3   2.35e-3   2.66e-3   8.1e-7
    200  72   [72, 64, 9]          0.1   2.35e-3   2.61e-3   2.58e-3   2.52e-3   7.7e-7
    192  128  None                 0.1   2.26e-3   2.38e-3   2.40e-3   2.43e-3   8.4e-7
    70   100  [100, 79, 7]         0.1   2.34e-3   2.71e-3   2.74e-3   2.46e-3   7.7e-7    (scale = 0.2)
    bounds                               1e-2      2e-2      2e-2      2e-2      1e-3

No case came near a bound, so no block carries an emulation-derived one.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bert_kernel_edges_gpu as E  # noqa: E402  (inputs, metric and bounds)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_attn_inputs, _block_err, _say = E._attn_inputs, E._block_err, E._say
CTX_BOUND, DQKV_BOUND, LSE_BOUND = E.CTX_BOUND, E.DQKV_BOUND, E.LSE_BOUND
H = 2
C = H * 64


def _kl(key_len):
    return None if key_len is None else torch.tensor(key_len, dtype=torch.int32, device=DEV)


def _cross_inputs(B, T, S, seed=1):
    g = torch.Generator().manual_seed(seed)  # host generator: the same inputs on every machine
    q = (torch.randn(B * T, C, generator=g) * 0.5).to(torch.bfloat16)
    kv = (torch.randn(B * S, 2 * C, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B * T, C, generator=g).to(torch.bfloat16)
    return q.to(DEV), kv.to(DEV), dctx.to(DEV)


def _run(q, kv, dctx, B, T, S, key_len, p=0.0, seed=1234, scale=None):
    from cloud_amd.ops import raw

    kl = _kl(key_len)
    ctx, lse = raw.attn_cross_fwd(q, kv, B, T, S, H, kl, p, seed, scale=scale)
    dq, dkv = raw.attn_cross_bwd(q, kv, ctx, dctx, lse, B, T, S, H, kl, p, seed, scale=scale)
    torch.cuda.synchronize()
    return ctx, lse, dq, dkv


def _cross_ref(q, kv, dctx, B, T, S, key_len, p, seed, scale=0.125):
    """E._attn_ref with separate T and S: fp64 attention of the bf16 inputs.  Returns ctx
    [B,H,T,64], dq [B,H,T,64], dkv [2,B,H,S,64] (K, V), the log2-domain log-sum-exp [B,H,T] and
    the clamped key_len."""
    from cloud_amd.ops import raw

    kl = torch.full((B,), S, device=DEV) if key_len is None else _kl(key_len).long().clamp(1, S)
    q_ = q.double().view(B, T, H, 64).permute(0, 2, 1, 3)
    k_, v_ = kv.double().view(B, S, 2, H, 64).permute(2, 0, 3, 1, 4)
    qd, k, v = [t.clone().requires_grad_() for t in (q_, k_, v_)]
    sc = (qd @ k.transpose(-1, -2)) * scale
    keymask = torch.arange(S, device=DEV)[None, :] >= kl[:, None]
    sc = sc.masked_fill(keymask[:, None, None, :], float("-inf"))
    lse2 = (torch.logsumexp(sc, -1) / math.log(2.0)).detach()
    att = sc.softmax(-1)
    if p > 0:
        keep = raw.dropout_mask(B * H * T * S, p, seed).view(B, H, T, S).double()
        att = att * keep / (1.0 - p)
    out = att @ v
    out.backward(dctx.double().view(B, T, H, 64).permute(0, 2, 1, 3))
    return out.detach(), qd.grad, torch.stack([k.grad, v.grad], 0), lse2, kl


def _views(ctx, dq, dkv, B, T, S):
    return (ctx.double().view(B, T, H, 64).permute(0, 2, 1, 3), dq.double().view(B, T, H, 64).permute(0, 2, 1, 3),
            dkv.double().view(B, S, 2, H, 64).permute(2, 0, 3, 1, 4))


def _check_vs_fp64(q, kv, dctx, B, T, S, key_len, p, seed=1234, scale=None, tag="cross"):
    ctx, lse, dq, dkv = _run(q, kv, dctx, B, T, S, key_len, p, seed, scale)
    sc = 0.125 if scale is None else scale
    ctx_r, dq_r, dkv_r, lse_r, kl = _cross_ref(q, kv, dctx, B, T, S, key_len, p, seed, sc)
    ctx_g, dq_g, dkv_g = _views(ctx, dq, dkv, B, T, S)
    e_ctx = _block_err(ctx_g, ctx_r)
    e_lse = (lse.double() - lse_r).abs().max().item()
    if T == 1 and S == 1:
        # dQ = dK = 0 exactly (module docstring): in units of the terms that cancel, per block
        nrm = lambda t: t.flatten(-2).norm(dim=-1)  # noqa: E731
        g = dctx.double().view(B, T, H, 64).permute(0, 2, 1, 3)
        k_r, v_r = kv.double().view(B, S, 2, H, 64).permute(2, 0, 3, 1, 4)
        q_r = q.double().view(B, T, H, 64).permute(0, 2, 1, 3)
        assert (dq_r == 0).all() and (dkv_r[0] == 0).all()
        e_dq = nrm(dq_g) / (sc * nrm(g) * nrm(v_r) * nrm(k_r))
        e_dk = nrm(dkv_g[0]) / (sc * nrm(g) * nrm(v_r) * nrm(q_r))
        e_dv = _block_err(dkv_g[1], dkv_r[1])
    else:
        e_dq = _block_err(dq_g, dq_r)
        e_dk, e_dv = _block_err(dkv_g, dkv_r)
    _say(f"{tag} T={T} S={S} key_len={key_len} p={p} scale={scale}: ctx/block max {e_ctx.max().item():.3e} "
         f"dq {e_dq.max().item():.3e} dk {e_dk.max().item():.3e} dv {e_dv.max().item():.3e} lse abs {e_lse:.3e}")
    for t in (ctx, lse, dq, dkv):
        assert torch.isfinite(t.float()).all()
    # keys at or past key_len take no part: their dK / dV rows are exactly zero
    pad = (torch.arange(S, device=DEV)[None, :] >= kl[:, None])[None, :, None, :, None].expand(2, B, H, S, 64)
    assert pad.any() or key_len is None or all(v >= S for v in key_len)
    assert (dkv_g[pad] == 0).all(), "dK / dV rows of masked keys must be exactly zero"
    assert e_lse < LSE_BOUND, e_lse
    assert e_ctx.max().item() < CTX_BOUND, e_ctx
    for name, e in (("dq", e_dq), ("dk", e_dk), ("dv", e_dv)):
        assert (e < DQKV_BOUND).all(), (name, e)
    return ctx, lse, dq, dkv


CASES = [
    (1, 1, None, 0.0),
    (1, 200, [200, 65, 7], 0.0),
    (2, 65, [65, 64, 17], 0.1),
    (64, 64, [64, 33, 17], 0.0),
    (64, 128, [128, 1, 65, 64], 0.0),
    (128, 64, [64, 5, 33], 0.1),
    (65, 63, [63, 17, 62], 0.1),
    (63, 129, [129, 128, 1, 65], 0.0),
    (200, 72, [72, 64, 9], 0.1),
    (192, 128, None, 0.1),
]


@pytest.mark.parametrize("T,S,key_len,p", CASES)
def test_cross_attention_vs_fp64(T, S, key_len, p):
    """Forward and backward once, every output against the fp64 reference per (batch, head)
    block; dK / dV rows of keys >= key_len are exactly zero; T = S = 1 copies V."""
    B = 4 if key_len is None else len(key_len)
    assert key_len is None or sum(1 for v in key_len if v <= 1) * 2 < B
    q, kv, dctx = _cross_inputs(B, T, S)
    ctx, _, _, _ = _check_vs_fp64(q, kv, dctx, B, T, S, key_len, p)
    if T == 1 and S == 1:  # the only probability is exactly 1
        assert torch.equal(ctx, kv[:, C:])


@pytest.mark.parametrize("S", [100, 192, 200])
def test_cross_equals_self_attention_bitwise(S):
    """T == S, q and kv the column views of one packed qkv (both at pitch 3C): the self- and the
    cross-attention entry points reach the same generic kernels, one with its gradients at pitch 3C
    inside dqkv, the other with contiguous dq and dkv, and both store the same bits.  (Self-attention
    at 64 and 128 dispatches to the one-workgroup kernels, which sum in another order, and is not
    compared.)"""
    from cloud_amd.ops import raw

    B, p, seed = 3, 0.1, 4321
    qkv, dctx = _attn_inputs(B, S, H)
    kl = _kl([S, S // 2 + 1, 37])
    ctx0, lse0 = raw.attn_fwd(qkv, B, S, H, kl, p, seed)
    dqkv0 = raw.attn_bwd(qkv, ctx0, dctx, lse0, B, S, H, kl, p, seed)
    q, kv = qkv[:, :C], qkv[:, C:]
    assert q.stride(0) == 3 * C and kv.stride(0) == 3 * C and not kv.is_contiguous()
    ctx, lse = raw.attn_cross_fwd(q, kv, B, S, S, H, kl, p, seed)
    dq, dkv = raw.attn_cross_bwd(q, kv, ctx, dctx, lse, B, S, S, H, kl, p, seed)
    torch.cuda.synchronize()
    assert torch.equal(ctx, ctx0)
    assert torch.equal(lse, lse0)
    assert torch.equal(dq, dqkv0[:, :C])
    assert torch.equal(dkv, dqkv0[:, C:])
    assert dq.is_contiguous() and dkv.is_contiguous()


def test_pitched_operands_equal_contiguous_ones_bitwise():
    """q inside a [B*T, C + 64] buffer, kv inside a [B*S, 2C + 8] buffer, everything around them
    NaN: the row pitch and the base pointer are all the kernels take from the buffer."""
    B, T, S, p = 2, 65, 130, 0.1
    q, kv, dctx = _cross_inputs(B, T, S)
    qbuf = torch.full((B * T, C + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    kvbuf = torch.full((B * S, 2 * C + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    qv, kvv = qbuf[:, 64:], kvbuf[:, 8:]
    qv.copy_(q)
    kvv.copy_(kv)
    assert qv.stride(0) == C + 64 and kvv.stride(0) == 2 * C + 8
    ref = _run(q, kv, dctx, B, T, S, [130, 77], p)
    got = _run(qv, kvv, dctx, B, T, S, [130, 77], p)
    for a, b in zip(got, ref):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    for a, b in zip(_run(qv.contiguous(), kvv.contiguous(), dctx, B, T, S, [130, 77], p), ref):
        assert torch.equal(a, b)


def test_operand_contract_raises():
    """Pitches are multiples of 8 elements and bases 16-byte aligned (the kernels load 16 bytes)."""
    from cloud_amd.ops import raw

    B, T, S = 1, 3, 5
    q, kv, dctx = _cross_inputs(B, T, S)
    qb = torch.zeros(B * T, C + 12, dtype=torch.bfloat16, device=DEV)
    kvb = torch.zeros(B * S, 2 * C + 16, dtype=torch.bfloat16, device=DEV)
    bad = [
        (qb[:, :C], kv),                   # pitch C + 12: no multiple of 8
        (q, kvb[:, 4:4 + 2 * C]),          # base 8 bytes into a row
        (q.t().contiguous().t(), kv),      # column stride != 1
        (q.float(), kv),                   # dtype
        (q[:, :64], kv),                   # width
        (q, kv[:S - 1]),                   # rows
    ]
    for qq, kk in bad:
        with pytest.raises(ValueError):
            raw.attn_cross_fwd(qq, kk, B, T, S, H)
    ctx, lse = raw.attn_cross_fwd(q, kv, B, T, S, H)
    with pytest.raises(ValueError):
        raw.attn_cross_bwd(qb[:, :C], kv, ctx, dctx, lse, B, T, S, H)
    with pytest.raises(ValueError):
        raw.attn_cross_bwd(q, kv, ctx, dctx[:, :64], lse, B, T, S, H)
    for shape in ((B, 0, S), (B, T, 0)):
        with pytest.raises(ValueError):
            raw.attn_cross_fwd(q[:shape[0] * shape[1]], kv[:shape[0] * shape[2]], *shape, H)


def test_tail_equals_zero_padding_bitwise():
    """(T, S) = (100, 200) against the same rows inside zero tensors of (128, 256) with
    key_len = 200: the tail instantiation only masks."""
    B, T, S, TP, SP = 2, 100, 200, 128, 256
    q, kv, dctx = _cross_inputs(B, T, S)
    ctx, lse, dq, dkv = _run(q, kv, dctx, B, T, S, [S, S])
    q_p = torch.zeros(B, TP, C, dtype=torch.bfloat16, device=DEV)
    kv_p = torch.zeros(B, SP, 2 * C, dtype=torch.bfloat16, device=DEV)
    dctx_p = torch.zeros(B, TP, C, dtype=torch.bfloat16, device=DEV)
    q_p[:, :T] = q.view(B, T, -1)
    kv_p[:, :S] = kv.view(B, S, -1)
    dctx_p[:, :T] = dctx.view(B, T, -1)
    ctx_p, lse_p, dq_p, dkv_p = _run(q_p.view(B * TP, -1), kv_p.view(B * SP, -1), dctx_p.view(B * TP, -1), B, TP, SP,
                                     [S, S])
    assert torch.equal(ctx.view(B, T, -1), ctx_p.view(B, TP, -1)[:, :T])
    assert torch.equal(lse, lse_p[:, :, :T])
    assert torch.equal(dq.view(B, T, -1), dq_p.view(B, TP, -1)[:, :T])
    dp = dkv_p.view(B, SP, -1)
    assert torch.equal(dkv.view(B, S, -1), dp[:, :S])
    assert (dp[:, S:] == 0).all(), "dK / dV rows of the padding must be exactly zero"


def test_key_blocks_past_key_len_are_not_read():
    """(T, S) = (70, 192), key_len = [64, 128]; K and V rows from 128 on are NaN.  A kernel that
    masks the third key block instead of skipping it multiplies 0 by NaN.  (Ordinary reads of
    allocated memory.)"""
    B, T, S, p = 2, 70, 192, 0.1
    key_len = [64, 128]
    q, kv, dctx = _cross_inputs(B, T, S)
    ctx1, lse1, dq1, dkv1 = _run(q, kv, dctx, B, T, S, key_len, p)
    kv2 = kv.clone().view(B, S, -1)
    kv2[:, 128:] = float("nan")
    ctx2, lse2, dq2, dkv2 = _run(q, kv2.view(B * S, -1), dctx, B, T, S, key_len, p)
    assert torch.equal(ctx1, ctx2) and torch.equal(lse1, lse2) and torch.equal(dq1, dq2)
    assert torch.equal(dkv1, dkv2)
    for d in (dkv1, dkv2):
        d3 = d.view(B, S, -1)
        assert (d3[0, 64:] == 0).all() and (d3[1, 128:] == 0).all()
        assert (d3[0, :64] != 0).any() and (d3[1, :128] != 0).any()


def test_batch_entries_do_not_see_each_other():
    B, T, S, p = 3, 70, 100, 0.1
    q, kv, dctx = _cross_inputs(B, T, S)
    ctx3, lse3, dq3, dkv3 = _run(q, kv, dctx, B, T, S, [100, 64, 37], p, seed=99)
    ctx1, lse1, dq1, dkv1 = _run(q[:T].contiguous(), kv[:S].contiguous(), dctx[:T].contiguous(), 1, T, S, [100], p,
                                 seed=99)
    assert torch.equal(ctx3[:T], ctx1)
    assert torch.equal(lse3[:1], lse1)
    assert torch.equal(dq3[:T], dq1)
    assert torch.equal(dkv3[:S], dkv1)


def test_ops_cross_attention_matches_raw():
    from cloud_amd.ops import cross_attention

    B, T, S, p, seed = 2, 70, 100, 0.1, 1234
    q, kv, dctx = _cross_inputs(B, T, S)
    ctx_r, _, dq_r, dkv_r = _run(q, kv, dctx, B, T, S, [100, 61], p, seed)
    x = q.view(B, T, -1).clone().requires_grad_()
    y = kv.view(B, S, -1).clone().requires_grad_()
    out = cross_attention(x, y, H, _kl([100, 61]), dropout_p=p, seed=seed)
    assert out.shape == (B, T, C) and out.dtype == torch.bfloat16
    out.backward(dctx.view(B, T, -1))
    torch.cuda.synchronize()
    assert torch.equal(out.detach().view(B * T, -1), ctx_r)
    assert torch.equal(x.grad.view(B * T, -1), dq_r)
    assert torch.equal(y.grad.view(B * S, -1), dkv_r)
    # non-contiguous inputs are made contiguous first
    wide = torch.zeros(B, S, 2 * C + 8, dtype=torch.bfloat16, device=DEV)
    wide[..., :2 * C] = kv.view(B, S, -1)
    out2 = cross_attention(q.view(B, T, -1), wide[..., :2 * C], H, _kl([100, 61]), dropout_p=p, seed=seed)
    assert torch.equal(out2, out.detach())
    # training=False turns dropout off
    ctx_0, _, _, _ = _run(q, kv, dctx, B, T, S, [100, 61], 0.0, 0)
    out3 = cross_attention(q.view(B, T, -1), kv.view(B, S, -1), H, _kl([100, 61]), dropout_p=p, training=False)
    assert torch.equal(out3.view(B * T, -1), ctx_0) and not torch.equal(ctx_0, ctx_r)


def test_key_len_and_scale_contract():
    """key_len=None means all keys; key_len is clamped to [1, S]; a non-default scale reaches
    every kernel."""
    B, T, S, p, seed = 2, 70, 100, 0.1, 77
    q, kv, dctx = _cross_inputs(B, T, S, seed=3)
    for a, b in ((None, [S, S]), ([0, S + 5], [1, S])):
        for x, y in zip(_run(q, kv, dctx, B, T, S, a, p, seed), _run(q, kv, dctx, B, T, S, b, p, seed)):
            assert torch.equal(x, y), (a, b)
    B = 3
    q, kv, dctx = _cross_inputs(B, T, S, seed=3)
    ctx, _, _, _ = _check_vs_fp64(q, kv, dctx, B, T, S, [S, S - 21, 7], p, scale=0.2, tag="cross-scale")
    ctx_d, _, _, _ = _run(q, kv, dctx, B, T, S, [S, S - 21, 7], p)
    assert not torch.equal(ctx, ctx_d)

    from cloud_amd.ops import cross_attention

    out = cross_attention(q.view(B, T, -1), kv.view(B, S, -1), H, _kl([S, S - 21, 7]), dropout_p=p, seed=1234,
                          scale=0.2)
    assert torch.equal(out.view(B * T, -1), ctx)
