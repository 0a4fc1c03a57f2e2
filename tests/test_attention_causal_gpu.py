"""Causal mode of the attention kernels (attn.hip): key j is visible to query i iff j <= i and
j < key_len[b].

Inputs, the fp64 reference pattern, the per-(batch, head) block metric and the bounds are
those of test_bert_kernel_edges_gpu (CTX_BOUND 1e-2, DQKV_BOUND 2e-2, LSE_BOUND 1e-3); the
reference adds the ``key > q`` mask, and dropout uses ``raw.dropout_mask`` with the unchanged
element index ``bh*S*S + q*S + key``.  Beyond the bounds the kernels are held to what "future
blocks are skipped, the diagonal block is masked" means: nothing at or before position t
depends on anything after it, bitwise; the generic kernels do not even read the blocks in the
future; the tail variant equals zero padding; row 0 is a copy of V[0].

Worst per-block figures observed on an MI355X (each test prints its own before asserting):

    S    key_len              p     ctx       dQ        dK        dV        lse abs
    2    [2, 2, 1]            0     1.22e-3   7.25e-3   7.61e-3   2.14e-3   5.6e-8    (*)
    63   [63, 17, 1, 62]      0     1.97e-3   2.77e-3   2.87e-3   2.27e-3   7.3e-7
    63   [63, 17, 1, 62]      0.1   2.37e-3   1.21e-2   1.09e-2   2.53e-3   7.3e-7
    64   [64, 1, 33, 17]      0     1.99e-3   2.69e-3   2.74e-3   2.14e-3   7.1e-7
    64   [64, 1, 33, 17]      0.1   2.47e-3   1.01e-2   1.07e-2   2.57e-3   7.1e-7
    65   [65, 64, 1, 33]      0     1.87e-3   2.58e-3   2.56e-3   2.42e-3   7.4e-7
    128  [128, 1, 65, 64]     0     1.97e-3   2.47e-3   2.45e-3   2.39e-3   7.7e-7
    128  [128, 1, 65, 64]     0.1   2.67e-3   1.62e-2   1.61e-2   2.53e-3   7.7e-7
    129  [129, 128, 1, 65]    0     1.93e-3   2.60e-3   2.61e-3   2.45e-3   7.7e-7
    192  [192, 128, 65, 64]   0.1   2.44e-3   3.52e-3   3.38e-3   2.42e-3   7.9e-7
    200  [200, 193, 64, 130]  0.1   2.55e-3   2.68e-3   2.74e-3   2.42e-3   7.7e-7
    192  None                 0     1.99e-3   2.84e-3   2.52e-3   2.37e-3   7.8e-7
    bounds                          1e-2      2e-2      2e-2      2e-2      1e-3
    row 0 lse against scale * (q0 . k0) * log2(e): 2.4e-8 (S = 64), 1.3e-8 (S = 128, 200)

No dropout case exceeds DQKV_BOUND (the key_len = 1 entries with p = 0.1 reach 1.0e-2 .. 1.6e-2),
so no block carries an emulation-derived bound.

(*) With the context divided by the unrounded row sum, as in the non-causal kernels, this case
missed the bound on one block: dK of (batch 1, head 1) 2.006e-2 (dQ 1.911e-2), and a bf16-faithful
fp32 emulation of the same inputs gave 2.0056e-2 / 1.9106e-2.  The block has one row with two
visible keys, whose dS = P (dP - Dv) nearly cancels, and the context's weights (P rounded to bf16
over the unrounded sum) did not sum to one.  The causal forward kernels now divide by the sum of
the rounded probabilities; the emulation predicted 7.606e-3 for that block, which is what it
measures.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bert_kernel_edges_gpu as T  # noqa: E402  (inputs, metric and bounds)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_attn_inputs, _block_err, _say = T._attn_inputs, T._block_err, T._say
CTX_BOUND, DQKV_BOUND, LSE_BOUND = T.CTX_BOUND, T.DQKV_BOUND, T.LSE_BOUND
H = 2
C = H * 64


def _kl(key_len):
    return None if key_len is None else torch.tensor(key_len, dtype=torch.int32, device=DEV)


def _run(qkv, dctx, B, S, key_len, p=0.0, seed=1234, causal=True):
    from cloud_amd.ops import raw

    kl = _kl(key_len)
    ctx, lse = raw.attn_fwd(qkv, B, S, H, kl, p, seed, causal=causal)
    dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl, p, seed, causal=causal)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


def _causal_ref(qkv, dctx, B, S, key_len, p, seed, scale=0.125):
    """T._attn_ref with the causal mask added: fp64 attention of the bf16 inputs.  Returns ctx
    [B,H,S,64], grads [3,B,H,S,64], the log2-domain log-sum-exp [B,H,S] and the clamped key_len."""
    from cloud_amd.ops import raw

    kl = torch.full((B,), S, device=DEV) if key_len is None else _kl(key_len).long().clamp(1, S)
    q_, k_, v_ = qkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    q, k, v = [t.clone().requires_grad_() for t in (q_, k_, v_)]
    sc = (q @ k.transpose(-1, -2)) * scale
    pos = torch.arange(S, device=DEV)
    keymask = pos[None, :] >= kl[:, None]
    sc = sc.masked_fill(keymask[:, None, None, :], float("-inf"))
    sc = sc.masked_fill((pos[None, :] > pos[:, None])[None, None], float("-inf"))  # [q, key]: key > q
    lse2 = (torch.logsumexp(sc, -1) / math.log(2.0)).detach()
    att = sc.softmax(-1)
    if p > 0:
        keep = raw.dropout_mask(B * H * S * S, p, seed).view(B, H, S, S).double()
        att = att * keep / (1.0 - p)
    out = att @ v
    out.backward(dctx.double().view(B, S, H, 64).permute(0, 2, 1, 3))
    return out.detach(), torch.stack([q.grad, k.grad, v.grad], 0), lse2, kl


CASES = [
    (2, [2, 2, 1], 0.0),
    (63, [63, 17, 1, 62], 0.0), (63, [63, 17, 1, 62], 0.1),
    (64, [64, 1, 33, 17], 0.0), (64, [64, 1, 33, 17], 0.1),        # one-workgroup kernels
    (65, [65, 64, 1, 33], 0.0),
    (128, [128, 1, 65, 64], 0.0), (128, [128, 1, 65, 64], 0.1),    # one-workgroup kernels
    (129, [129, 128, 1, 65], 0.0),
    (192, [192, 128, 65, 64], 0.1),
    (200, [200, 193, 64, 130], 0.1),
    (192, None, 0.0),
]


@pytest.mark.parametrize("S,key_len,p", CASES)
def test_causal_attention_vs_fp64(S, key_len, p):
    """Forward and backward once, every output against the fp64 reference per (batch, head)
    block; dK / dV rows of keys >= key_len are exactly zero."""
    B = 4 if key_len is None else len(key_len)
    assert key_len is None or sum(1 for v in key_len if v <= 1) * 2 < B
    seed = 1234
    qkv, dctx = _attn_inputs(B, S, H)
    ctx, lse, dqkv = _run(qkv, dctx, B, S, key_len, p, seed)
    ctx_r, dqkv_r, lse_r, kl = _causal_ref(qkv, dctx, B, S, key_len, p, seed)
    ctx_g = ctx.double().view(B, S, H, 64).permute(0, 2, 1, 3)
    dqkv_g = dqkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4)
    e_ctx = _block_err(ctx_g, ctx_r)
    e_d = _block_err(dqkv_g, dqkv_r)
    e_lse = (lse.double() - lse_r).abs().max().item()
    _say(f"causal S={S} key_len={key_len} p={p}: ctx/block max {e_ctx.max().item():.3e} "
         f"dq {e_d[0].max().item():.3e} dk {e_d[1].max().item():.3e} dv {e_d[2].max().item():.3e} "
         f"lse abs {e_lse:.3e}")
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(dqkv.float()).all() and torch.isfinite(lse).all()
    pad = (torch.arange(S, device=DEV)[None, :] >= kl[:, None])[None, :, None, :, None].expand(2, B, H, S, 64)
    assert pad.any() or key_len is None or all(v >= S for v in key_len)
    assert (dqkv_g[1:][pad] == 0).all(), "dK / dV rows of masked keys must be exactly zero"
    assert e_lse < LSE_BOUND, e_lse
    assert e_ctx.max().item() < CTX_BOUND, e_ctx
    assert (e_d < DQKV_BOUND).all(), e_d


@pytest.mark.parametrize("S", [64, 128, 200])
def test_causal_row_zero_is_a_copy_of_v0(S):
    """Query 0 sees key 0 only: its probability is exactly 1, so ctx[b, 0] = V[b, 0] bitwise and
    lse[b, h, 0] = scale * (q0 . k0) * log2(e)."""
    B = 3
    qkv, dctx = _attn_inputs(B, S, H)
    ctx, lse, _ = _run(qkv, dctx, B, S, [S, 1, max(1, S // 2)])
    x = qkv.view(B, S, 3, H, 64)
    assert torch.equal(ctx.view(B, S, H, 64)[:, 0], x[:, 0, 2])
    ref = 0.125 * (x[:, 0, 0].double() * x[:, 0, 1].double()).sum(-1) * math.log2(math.e)  # [B, H]
    e = (lse[:, :, 0].double() - ref).abs().max().item()
    _say(f"causal row 0 S={S}: lse abs {e:.3e}")
    assert e < LSE_BOUND, e


def test_causality_by_perturbation():
    """S = 200, t = 100, dropout 0.1, the same seed twice; the second run has other (finite) Q, K
    and V rows after t.  Nothing at rows <= t may move, bitwise: masked elements are exactly
    p = 0 and dS = 0, and an exact zero times a finite operand adds nothing."""
    B, S, t, p = 2, 200, 100, 0.1
    qkv, dctx = _attn_inputs(B, S, H)
    other, _ = _attn_inputs(B, S, H, seed=7)
    ctx1, lse1, d1 = _run(qkv, dctx, B, S, [200, 150], p, seed=5)
    q2 = qkv.clone().view(B, S, -1)
    q2[:, t + 1:] = other.view(B, S, -1)[:, t + 1:]
    assert not torch.equal(q2, qkv.view(B, S, -1))
    ctx2, lse2, d2 = _run(q2.view(B * S, -1), dctx, B, S, [200, 150], p, seed=5)
    assert torch.equal(ctx1.view(B, S, -1)[:, :t + 1], ctx2.view(B, S, -1)[:, :t + 1])
    assert torch.equal(lse1[:, :, :t + 1], lse2[:, :, :t + 1])
    assert torch.equal(d1.view(B, S, -1)[:, :t + 1, :C], d2.view(B, S, -1)[:, :t + 1, :C])
    assert not torch.equal(ctx1.view(B, S, -1)[:, t + 1:], ctx2.view(B, S, -1)[:, t + 1:])


@pytest.mark.parametrize("S,first_nan", [(192, 128), (200, 192)])
def test_causal_forward_and_dq_do_not_read_future_key_blocks(S, first_nan):
    """Generic path: K and V rows from ``first_nan`` (a block boundary) on are NaN.  A kernel
    that masks these blocks instead of skipping them multiplies 0 by NaN; one that skips them
    leaves every earlier row of ctx, lse and dQ bitwise as in the clean run.  (Ordinary reads
    of finite, allocated memory.)"""
    B = 2
    qkv, dctx = _attn_inputs(B, S, H)
    ctx1, lse1, d1 = _run(qkv, dctx, B, S, None)
    q2 = qkv.clone().view(B, S, -1)
    q2[:, first_nan:, C:] = float("nan")
    ctx2, lse2, d2 = _run(q2.view(B * S, -1), dctx, B, S, None)
    n = first_nan
    assert torch.equal(ctx1.view(B, S, -1)[:, :n], ctx2.view(B, S, -1)[:, :n])
    assert torch.equal(lse1[:, :, :n], lse2[:, :, :n])
    assert torch.equal(d1.view(B, S, -1)[:, :n, :C], d2.view(B, S, -1)[:, :n, :C])


def test_causal_dkv_does_not_read_past_query_blocks():
    """Generic path, S = 192: dO rows 0..63 are NaN in the backward.  Key blocks 1 and 2 start
    their query loop at their own block, and query blocks 1 and 2 never see those rows, so dK /
    dV rows 64..191 and dQ rows 64..191 are bitwise those of the clean backward."""
    from cloud_amd.ops import raw

    B, S = 2, 192
    qkv, dctx = _attn_inputs(B, S, H)
    ctx, lse = raw.attn_fwd(qkv, B, S, H, None, 0.0, 0, causal=True)
    d1 = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, None, 0.0, 0, causal=True)
    g2 = dctx.clone().view(B, S, -1)
    g2[:, :64] = float("nan")
    d2 = raw.attn_bwd(qkv, ctx, g2.view(B * S, -1), lse, B, S, H, None, 0.0, 0, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(d1.view(B, S, -1)[:, 64:], d2.view(B, S, -1)[:, 64:])


def test_causal_tail_equals_zero_padding_bitwise():
    """The pattern of test_attention_tail_equals_zero_padding_bitwise: causal at S = 200 against
    the same rows in zero tensors of S = 256 with key_len = 200."""
    B, S, SP = 2, 200, 256
    qkv, dctx = _attn_inputs(B, S, H)
    ctx, lse, dqkv = _run(qkv, dctx, B, S, [S, S])
    qkv_p = torch.zeros(B, SP, 3 * C, dtype=torch.bfloat16, device=DEV)
    dctx_p = torch.zeros(B, SP, C, dtype=torch.bfloat16, device=DEV)
    qkv_p[:, :S] = qkv.view(B, S, -1)
    dctx_p[:, :S] = dctx.view(B, S, -1)
    ctx_p, lse_p, dqkv_p = _run(qkv_p.view(B * SP, -1), dctx_p.view(B * SP, -1), B, SP, [S, S])
    assert torch.equal(ctx.view(B, S, -1), ctx_p.view(B, SP, -1)[:, :S])
    assert torch.equal(lse, lse_p[:, :, :S])
    dp = dqkv_p.view(B, SP, -1)
    assert torch.equal(dqkv.view(B, S, -1), dp[:, :S])
    assert (dp[:, S:, C:] == 0).all(), "dK / dV rows of the padding must be exactly zero"


def test_causal_batch_entries_do_not_see_each_other():
    B, S, p = 3, 100, 0.1
    qkv, dctx = _attn_inputs(B, S, H)
    ctx3, lse3, dqkv3 = _run(qkv, dctx, B, S, [100, 64, 37], p, seed=99)
    ctx1, lse1, dqkv1 = _run(qkv[:S].contiguous(), dctx[:S].contiguous(), 1, S, [100], p, seed=99)
    assert torch.equal(ctx3[:S], ctx1)
    assert torch.equal(lse3[:1], lse1)
    assert torch.equal(dqkv3[:S], dqkv1)


def test_ops_attention_causal_matches_raw():
    from cloud_amd.ops import attention

    B, S, p, seed = 2, 100, 0.1, 1234
    qkv, dctx = _attn_inputs(B, S, H)
    ctx_r, _, dqkv_r = _run(qkv, dctx, B, S, [100, 61], p, seed)
    x = qkv.view(B, S, -1).clone().requires_grad_()
    out = attention(x, H, _kl([100, 61]), dropout_p=p, seed=seed, causal=True)
    out.backward(dctx.view(B, S, -1))
    torch.cuda.synchronize()
    assert torch.equal(out.detach().view(B * S, -1), ctx_r)
    assert torch.equal(x.grad.view(B * S, -1), dqkv_r)
    ctx_n, _, _ = _run(qkv, dctx, B, S, [100, 61], p, seed, causal=False)
    assert not torch.equal(ctx_n, ctx_r)


@pytest.mark.parametrize("S", [100, 128])
def test_causal_false_is_the_call_without_the_keyword(S):
    from cloud_amd.ops import raw

    B, p, seed = 2, 0.1, 3
    qkv, dctx = _attn_inputs(B, S, H)
    kl = _kl([S, S // 2])
    ctx0, lse0 = raw.attn_fwd(qkv, B, S, H, kl, p, seed)
    d0 = raw.attn_bwd(qkv, ctx0, dctx, lse0, B, S, H, kl, p, seed)
    ctx1, lse1, d1 = _run(qkv, dctx, B, S, [S, S // 2], p, seed, causal=False)
    assert torch.equal(ctx0, ctx1) and torch.equal(lse0, lse1) and torch.equal(d0, d1)
