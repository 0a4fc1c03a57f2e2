"""Attention masks in the cross-attention kernels of attn.hip (``raw.attn_cross_fwd`` /
``raw.attn_cross_bwd`` with ``mask=``), ``ops.cross_attention(mask=)`` and ``ops.attention(mask=)``:
a byte mask ``[B|1, H|1, T|1, S]`` read through broadcast strides; query q sees key iff
``key < key_len[b]`` and its byte is non-zero.  A query that sees no key has context exactly 0, a
finite lse (0) and sends exactly 0 to dQ, dK and dV; a key no query sees gets exact-zero dK / dV.

Built like test_attention_cross_gpu: inputs from a seeded host generator (``randn * 0.5`` in
bf16), an fp64 reference on the same bf16 inputs with the kernels' dropout mask from
``raw.dropout_mask``, the per-(batch, head) block metric and the bounds of
test_bert_kernel_edges_gpu (CTX_BOUND 1e-2, DQKV_BOUND 2e-2, LSE_BOUND 1e-3).  They carry over
because the arithmetic and the operation order of the visible elements are those of the unmasked
kernels: an all-True mask stores the same bits as no mask (test_all_true_mask_is_bitwise_no_mask).

Rows with 2 - 4 visible keys make dS = P (dP - Dv) cancel, and the bf16 rounding of the context
then dominates the metric (the notes of the sibling files), so every case asserts on the host
that each live row has at least 8 visible keys below ``key_len``; designed dead rows are exempt
from the metric (their reference is exactly zero too) and are checked exactly.

Worst per-block figures observed on an MI355X (each test prints its own before asserting):

    T    S    key_len          p     mask         dead rows  ctx       dQ        dK        dV        lse abs
    1    200  None             0     [3,2,1,200]  0          2.53e-3   3.03e-3   2.54e-3   2.45e-3   4.9e-7
    63   129  None             0     [2,2,63,129] 0          2.27e-3   2.38e-3   2.39e-3   2.38e-3   7.3e-7
    64   64   None             0     [2,2,64,64]  0          2.29e-3   2.39e-3   2.38e-3   2.36e-3   7.4e-7
    65   63   None             0     [3,2,65,63]  0          2.37e-3   2.42e-3   2.45e-3   2.40e-3   7.4e-7
    130  65   None             0.1   [2,2,130,65] 0          2.32e-3   2.43e-3   2.43e-3   2.35e-3   7.4e-7
    70   100  [100, 60, 77]    0.1   [3,2,70,100] 0          2.44e-3   2.50e-3   2.40e-3   2.37e-3   7.0e-7
    65   200  None             0     blocks       2          2.28e-3   2.37e-3   2.36e-3   2.34e-3   7.6e-7
    65   200  None             0.1   blocks       2          2.31e-3   2.35e-3   2.39e-3   2.33e-3   7.6e-7
    65   200  [200, 64]        0.1   blocks       18         2.42e-3   2.42e-3   2.35e-3   2.43e-3   7.6e-7
    bounds                                                   1e-2      2e-2      2e-2      2e-2      1e-3

    mask=tril against causal=True at S = 130 (kernels against kernels): ctx 1.39e-3, dqkv 2.77e-3.

No case came near a bound.  ("blocks" is the designed mask of test_block_structure_and_dead_rows.)
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


def _rand_mask(shape, seed=1, density=0.5):
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.rand(*shape, generator=g) < density  # host tensor


def _allowed(mask, B, T, S, key_len):
    """The full [B, H, T, S] visibility (host or device, like ``mask``): mask AND key < key_len."""
    a = mask.expand(B, H, T, S)
    if key_len is not None:
        kl = torch.tensor(key_len, device=mask.device).clamp(1, S)
        a = a & (torch.arange(S, device=mask.device)[None, :] < kl[:, None])[:, None, None, :]
    return a


def _run(q, kv, dctx, B, T, S, key_len, mask, p=0.0, seed=1234, scale=None):
    from cloud_amd.ops import raw

    kl = _kl(key_len)
    ctx, lse = raw.attn_cross_fwd(q, kv, B, T, S, H, kl, p, seed, scale=scale, mask=mask)
    dq, dkv = raw.attn_cross_bwd(q, kv, ctx, dctx, lse, B, T, S, H, kl, p, seed, scale=scale, mask=mask)
    torch.cuda.synchronize()
    return ctx, lse, dq, dkv


def _masked_ref(q, kv, dctx, B, T, S, allowed, p, seed, scale=0.125):
    """fp64 attention of the bf16 inputs over the allowed keys.  Returns ctx [B,H,T,64], dq
    [B,H,T,64], dkv [2,B,H,S,64] (K, V) and the log2-domain log-sum-exp [B,H,T] (0 for dead rows).
    Dead rows keep finite scores and are multiplied out, so nothing is NaN."""
    from cloud_amd.ops import raw

    q_ = q.double().view(B, T, H, 64).permute(0, 2, 1, 3)
    k_, v_ = kv.double().view(B, S, 2, H, 64).permute(2, 0, 3, 1, 4)
    qd, k, v = [t.clone().requires_grad_() for t in (q_, k_, v_)]
    live = allowed.any(-1, keepdim=True)
    sc = ((qd @ k.transpose(-1, -2)) * scale).masked_fill(~allowed & live, float("-inf"))
    lse2 = (torch.logsumexp(sc, -1) / math.log(2.0)).detach() * live[..., 0]
    att = sc.softmax(-1) * (allowed & live)
    if p > 0:
        keep = raw.dropout_mask(B * H * T * S, p, seed).view(B, H, T, S).double()
        att = att * keep / (1.0 - p)
    out = att @ v
    out.backward(dctx.double().view(B, T, H, 64).permute(0, 2, 1, 3))
    return out.detach(), qd.grad, torch.stack([k.grad, v.grad], 0), lse2


def _views(ctx, dq, dkv, B, T, S):
    return (ctx.double().view(B, T, H, 64).permute(0, 2, 1, 3), dq.double().view(B, T, H, 64).permute(0, 2, 1, 3),
            dkv.double().view(B, S, 2, H, 64).permute(2, 0, 3, 1, 4))


def _check_vs_fp64(q, kv, dctx, B, T, S, key_len, mask, p, seed=1234, tag="mask", min_visible=8):
    """``mask``: a device bool tensor [B|1, H|1, T|1, S].  Every live row must have at least
    ``min_visible`` visible keys (module docstring); dead rows and unseen keys are checked exactly."""
    allowed = _allowed(mask, B, T, S, key_len)
    vis = allowed.sum(-1)
    dead = vis == 0                                       # [B, H, T]
    assert (vis[~dead] >= min_visible).all(), f"a live row with only {int(vis[~dead].min())} visible keys"
    ctx, lse, dq, dkv = _run(q, kv, dctx, B, T, S, key_len, mask, p, seed)
    ctx_r, dq_r, dkv_r, lse_r = _masked_ref(q, kv, dctx, B, T, S, allowed, p, seed)
    ctx_g, dq_g, dkv_g = _views(ctx, dq, dkv, B, T, S)
    e_ctx = _block_err(ctx_g, ctx_r)
    e_lse = (lse.double() - lse_r).abs().max().item()
    e_dq = _block_err(dq_g, dq_r)
    e_dk, e_dv = _block_err(dkv_g, dkv_r)
    _say(f"{tag} T={T} S={S} key_len={key_len} mask={tuple(mask.shape)} p={p} dead rows={int(dead.sum())}: "
         f"ctx/block max {e_ctx.max().item():.3e} dq {e_dq.max().item():.3e} dk {e_dk.max().item():.3e} "
         f"dv {e_dv.max().item():.3e} lse abs {e_lse:.3e}")
    for t in (ctx, lse, dq, dkv):
        assert torch.isfinite(t.float()).all()
    # a row that sees nothing: context and dQ exactly zero, lse stored as 0
    assert (ctx_g[dead] == 0).all() and (dq_g[dead] == 0).all() and (lse[dead] == 0).all()
    # a key nobody sees (through the mask or key_len): dK / dV rows exactly zero
    unseen = ~allowed.any(2)                              # [B, H, S]
    assert (dkv_g[:, unseen] == 0).all(), "dK / dV rows of unseen keys must be exactly zero"
    assert e_lse < LSE_BOUND, e_lse
    assert e_ctx.max().item() < CTX_BOUND, e_ctx
    for name, e in (("dq", e_dq), ("dk", e_dk), ("dv", e_dv)):
        assert (e < DQKV_BOUND).all(), (name, e)
    return ctx, lse, dq, dkv


CASES = [
    # T, S, B, key_len, p, mask shape (None = [B, H, T, S])
    (1, 200, 3, None, 0.0, None),
    (63, 129, 2, None, 0.0, None),
    (64, 64, 2, None, 0.0, None),
    (65, 63, 3, None, 0.0, None),
    (130, 65, 2, None, 0.1, None),
    (70, 100, 3, [100, 60, 77], 0.1, None),
]


@pytest.mark.parametrize("T,S,B,key_len,p,mshape", CASES)
def test_masked_cross_attention_vs_fp64(T, S, B, key_len, p, mshape):
    """Density-0.5 random per-head masks; forward and backward once, every output against the
    fp64 reference per (batch, head) block."""
    assert key_len is None or (all(v >= 60 for v in key_len) and any(v < S for v in key_len))
    q, kv, dctx = _cross_inputs(B, T, S)
    mask = _rand_mask(mshape or (B, H, T, S)).to(DEV)
    _check_vs_fp64(q, kv, dctx, B, T, S, key_len, mask, p)


def _block_structure_mask(B, T, S):
    m = _rand_mask((B, H, T, S), seed=2)
    m[:, :, 0:8, :64] = False           # nothing in the first key block, everything after
    m[:, :, 0:8, 64:] = True
    m[:, :, 8:16, :64] = True           # only the first key block
    m[:, :, 8:16, 64:] = False
    m[:, :, 16:24, 64:128] = False      # the middle block dead
    m[:, :, 64, :] = True               # (the tail query block has a live row ...)
    m[:, :, 64, 128:] = False
    m[0, 1, 30, :] = False              # one row dead entirely
    m[1, 0, 64, :] = False              # ... and a dead one in one (batch, head)
    m[:, :, :, 77] = False              # keys no query sees: the middle block and the tail block
    m[:, :, :, 199] = False
    m[0, 0, :, 3] = False
    return m


def test_block_structure_and_dead_rows():
    """T = 65, S = 200 (two query blocks, four key blocks, both with a tail).  Rows whose first
    key block is dead reach the first visible key with m = -inf (the -inf - -inf guard of the
    forward), a dead middle block leaves m untouched, a dead row stores zeros everywhere."""
    B, T, S = 2, 65, 200
    q, kv, dctx = _cross_inputs(B, T, S)
    m = _block_structure_mask(B, T, S)
    for p in (0.0, 0.1):
        ctx, lse, dq, dkv = _check_vs_fp64(q, kv, dctx, B, T, S, None, m.to(DEV), p, tag="blocks")
        c4, q4 = ctx.view(B, T, H, 64), dq.view(B, T, H, 64)
        for b, h, t in ((0, 1, 30), (1, 0, 64)):
            assert (c4[b, t, h] == 0).all() and (q4[b, t, h] == 0).all() and lse[b, h, t] == 0
            assert (c4[b, t, 1 - h] != 0).any() and (q4[b, t, 1 - h] != 0).any()
        d5 = dkv.view(B, S, 2, H, 64)
        assert (d5[:, 77] == 0).all() and (d5[:, 199] == 0).all() and (d5[0, 3, :, 0] == 0).all()
        assert (d5[0, 3, :, 1] != 0).any() and (d5[:, 78] != 0).any()
    # with key_len the middle-block rows of batch 1 keep keys 0..63 only; rows 0..7 die there
    _check_vs_fp64(q, kv, dctx, B, T, S, [200, 64], m.to(DEV), 0.1, tag="blocks+key_len")


@pytest.mark.parametrize("key_len", [None, [130, 77, 64]])
def test_all_true_mask_is_bitwise_no_mask(key_len):
    """The masked instantiations with every byte set store what the unmasked ones store: same
    arithmetic, same order, same dropout index.  As bool and as uint8 (any non-zero byte)."""
    from cloud_amd.ops import raw

    B, T, S, p = 3, 65, 130, 0.1
    q, kv, dctx = _cross_inputs(B, T, S)
    kl = _kl(key_len)
    ctx0, lse0 = raw.attn_cross_fwd(q, kv, B, T, S, H, kl, p, 77)
    dq0, dkv0 = raw.attn_cross_bwd(q, kv, ctx0, dctx, lse0, B, T, S, H, kl, p, 77)
    ones = torch.ones(B, H, T, S, dtype=torch.bool, device=DEV)
    for mask in (ones, ones[:1, :1, :1], ones.to(torch.uint8) * 255):
        got = _run(q, kv, dctx, B, T, S, key_len, mask, p, 77)
        for a, b in zip(got, (ctx0, lse0, dq0, dkv0)):
            assert torch.equal(a, b)
    # full blocks only (the non-tail instantiations)
    q, kv, dctx = _cross_inputs(B, 128, 192)
    kl2 = None if key_len is None else [192, 77, 64]
    ref = _run(q, kv, dctx, B, 128, 192, kl2, None, p, 77)
    got = _run(q, kv, dctx, B, 128, 192, kl2, torch.ones(1, 1, 1, 192, dtype=torch.bool, device=DEV), p, 77)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.parametrize("T,S", [(65, 130), (64, 128)])
def test_broadcast_masks_equal_materialised_ones_bitwise(T, S):
    """Stride-0 axes: [B,1,1,S], [1,1,T,S] and [B,1,T,S] against their [B,H,T,S] expansion; a
    per-head mask against two runs with each head's mask broadcast over the heads."""
    B, p = 2, 0.1
    q, kv, dctx = _cross_inputs(B, T, S)
    for i, shape in enumerate(((B, 1, 1, S), (1, 1, T, S), (B, 1, T, S))):
        m = _rand_mask(shape, seed=10 + i).to(DEV)
        full = m.expand(B, H, T, S).contiguous()
        for a, b in zip(_run(q, kv, dctx, B, T, S, [S, 70], m, p), _run(q, kv, dctx, B, T, S, [S, 70], full, p)):
            assert torch.equal(a, b), shape
    m = _rand_mask((B, H, T, S), seed=20).to(DEV)
    assert not torch.equal(m[:, 0], m[:, 1])
    ctx, lse, dq, dkv = _run(q, kv, dctx, B, T, S, None, m, p)
    for h in range(H):
        ctx_h, lse_h, dq_h, dkv_h = _run(q, kv, dctx, B, T, S, None, m[:, h:h + 1], p)
        sl = slice(h * 64, (h + 1) * 64)
        assert torch.equal(ctx[:, sl], ctx_h[:, sl]) and torch.equal(lse[:, h], lse_h[:, h])
        assert torch.equal(dq[:, sl], dq_h[:, sl])
        assert torch.equal(dkv.view(B * S, 2, C)[:, :, sl], dkv_h.view(B * S, 2, C)[:, :, sl])
        other = slice((1 - h) * 64, (2 - h) * 64)
        assert not torch.equal(ctx[:, other], ctx_h[:, other])


def test_pitched_operands_and_mask_views_equal_contiguous_ones_bitwise():
    """q and kv inside wider NaN buffers, the mask a view into a wider buffer of ones with an
    odd row pitch (rows at every byte alignment): base pointers and pitches are all the kernels
    take."""
    B, T, S, p = 2, 65, 130, 0.1
    q, kv, dctx = _cross_inputs(B, T, S)
    m = _rand_mask((B, H, T, S), seed=30).to(DEV)
    qbuf = torch.full((B * T, C + 64), float("nan"), dtype=torch.bfloat16, device=DEV)
    kvbuf = torch.full((B * S, 2 * C + 8), float("nan"), dtype=torch.bfloat16, device=DEV)
    mbuf = torch.ones(B, H, T + 3, S + 7, dtype=torch.bool, device=DEV)
    qv, kvv, mv = qbuf[:, 64:], kvbuf[:, 8:], mbuf[:, :, 2:2 + T, 5:5 + S]
    qv.copy_(q)
    kvv.copy_(kv)
    mv.copy_(m)
    assert mv.stride() == ((H * (T + 3)) * (S + 7), (T + 3) * (S + 7), S + 7, 1) and not mv.is_contiguous()
    ref = _run(q, kv, dctx, B, T, S, [130, 77], m, p)
    for a, b in zip(_run(qv, kvv, dctx, B, T, S, [130, 77], mv, p), ref):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_mask_contract_raises():
    from cloud_amd.ops import raw

    B, T, S = 2, 3, 5
    q, kv, dctx = _cross_inputs(B, T, S)
    ok = torch.ones(B, H, T, S, dtype=torch.bool, device=DEV)
    bad = [
        ok[0],                                                                   # not 4-D
        ok[..., :4],                                                             # keys
        ok[:, :, :2],                                                            # queries: neither 1 nor T
        torch.ones(B + 1, H, T, S, dtype=torch.bool, device=DEV),                # batch
        ok.float(),                                                              # dtype
        ok.cpu(),                                                                # device
        torch.ones(B, H, S, T, dtype=torch.bool, device=DEV).transpose(2, 3),    # key stride != 1
    ]
    for m in bad:
        with pytest.raises(ValueError):
            raw.attn_cross_fwd(q, kv, B, T, S, H, mask=m)
    ctx, lse = raw.attn_cross_fwd(q, kv, B, T, S, H, mask=ok)
    with pytest.raises(ValueError):
        raw.attn_cross_bwd(q, kv, ctx, dctx, lse, B, T, S, H, mask=ok[..., :4])
    with pytest.raises(TypeError):  # keyword only: positional callers cannot pass it by accident
        raw.attn_cross_fwd(q, kv, B, T, S, H, None, 0.0, 0, None, ok)


def test_ops_attention_mask_equals_cross_attention_on_views_bitwise():
    from cloud_amd.ops import attention, cross_attention

    B, S, p, seed = 2, 130, 0.1, 4321
    qkv, dctx = _attn_inputs(B, S, H)
    m = _rand_mask((B, 1, S, S), seed=40).to(DEV)
    kl = _kl([S, 99])
    x = qkv.view(B, S, -1).clone().requires_grad_()
    out = attention(x, H, kl, dropout_p=p, seed=seed, mask=m)
    out.backward(dctx.view(B, S, -1))
    x2 = qkv.view(B, S, -1).clone()
    a, b = x2[..., :C].clone().requires_grad_(), x2[..., C:].clone().requires_grad_()
    out2 = cross_attention(a, b, H, kl, dropout_p=p, seed=seed, mask=m[:, 0])
    out2.backward(dctx.view(B, S, -1))
    torch.cuda.synchronize()
    assert out.dtype == torch.bfloat16 and out.shape == (B, S, C)
    assert torch.equal(out.detach(), out2.detach())
    assert x.grad.shape == (B, S, 3 * C)
    assert torch.equal(x.grad[..., :C], a.grad) and torch.equal(x.grad[..., C:], b.grad)
    # every accepted rank reaches the kernels as the same mask
    m2 = _rand_mask((S, S), seed=41).to(DEV)
    ref = attention(qkv.view(B, S, -1), H, None, mask=m2[None, None].expand(B, H, S, S).contiguous())
    for form in (m2, m2[None], m2[None, None], m2.t().contiguous().t()):
        assert torch.equal(attention(qkv.view(B, S, -1), H, None, mask=form), ref)


def test_ops_attention_tril_mask_agrees_with_causal():
    """``mask=tril`` on the mask kernels against ``causal=True`` on the causal kernels: another
    block loop, so within the bounds (of each other), not bitwise.  S = 130: three key blocks.
    Rows 0 - 7 have fewer than 8 visible keys, by construction the same in both routes."""
    from cloud_amd.ops import attention

    B, S = 2, 130
    qkv, dctx = _attn_inputs(B, S, H)
    tril = torch.ones(S, S, dtype=torch.bool, device=DEV).tril()
    outs = []
    for kw in (dict(mask=tril), dict(causal=True), dict(mask=tril, causal=True)):
        x = qkv.view(B, S, -1).clone().requires_grad_()
        y = attention(x, H, _kl([S, 101]), **kw)
        y.backward(dctx.view(B, S, -1))
        outs.append((y.detach(), x.grad))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[0][1], outs[2][1])
    (y_m, g_m), (y_c, g_c) = outs[0], outs[1]
    blk = lambda t, n: t.double().view(B, S, n, H, 64).permute(2, 0, 3, 1, 4)  # noqa: E731
    e_ctx = _block_err(blk(y_m, 1), blk(y_c, 1)).max().item()
    e_g = _block_err(blk(g_m, 3), blk(g_c, 3)).max().item()
    _say(f"tril-vs-causal S={S}: ctx/block max {e_ctx:.3e} dqkv {e_g:.3e}")
    assert e_ctx < CTX_BOUND and e_g < DQKV_BOUND
