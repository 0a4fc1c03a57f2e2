"""Attention, ``ops.attention`` and the native BERT path at sequence lengths that are no
multiple of 64 (the TAIL instantiation of the generic kernels of attn.hip).

Reference, inputs, metric and bounds are those of test_bert_kernel_edges_gpu: fp64 attention
of the same bf16 inputs, errors per (batch, head) block, CTX_BOUND 1e-2, DQKV_BOUND 2e-2,
LSE_BOUND 1e-3.  Beyond the bounds, the tail variant is held to what "it only masks" means:
bitwise the result of the same rows zero-padded to the next multiple of 64, nothing read
from behind the tensors, no write into a neighbouring batch entry.
"""
import contextlib
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bert_kernel_edges_gpu as T  # noqa: E402  (reference, inputs, metric and bounds)

pytestmark = pytest.mark.gpu

DEV = "cuda"
_attn_inputs, _attn_ref, _block_err, _attn_case, _say = T._attn_inputs, T._attn_ref, T._block_err, T._attn_case, T._say
CTX_BOUND, DQKV_BOUND, LSE_BOUND = T.CTX_BOUND, T.DQKV_BOUND, T.LSE_BOUND


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _run(qkv, dctx, B, S, H, key_len, p=0.0, seed=1234):
    from cloud_amd.ops import raw

    kl = None if key_len is None else torch.tensor(key_len, dtype=torch.int32, device=DEV)
    ctx, lse = raw.attn_fwd(qkv, B, S, H, kl, p, seed)
    dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl, p, seed)
    torch.cuda.synchronize()
    return ctx, lse, dqkv


@pytest.mark.parametrize("S,key_len,p", [
    (2, [2, 2, 1], 0.0),              # one wave with two live rows
    (63, [63, 17, 1, 62], 0.0),       # one partial block
    (63, [63, 17, 33, 62], 0.1),      # one partial block, with dropout
    (65, [65, 64, 1, 33], 0.0),       # second block holds one row; its waves 1-3 have no valid row
    (100, [100, 64, 65, 99], 0.1),    # between the two short-path lengths
    (129, [129, 128, 1, 65], 0.0),    # third block holds one row
    (200, [200, 193, 64, 130], 0.1),  # partial fourth block
])
def test_attention_tails_vs_fp64(S, key_len, p):
    _attn_case(S, key_len, p, tag="attn-tail")


def test_attention_single_token():
    """S = 1: the softmax over one key is exactly 1, so ctx = V and dV = dO bitwise; the true
    dQ and dK are zero, and what is left of dS = P (dP - Dv) is the difference of two fp32 sums
    of the same 64 products in different orders (<= 64 * 2^-24 ~ 3.8e-6 times |dO| |V|); 1e-4
    leaves about 25 x for the bf16 rounding of dS and of the output."""
    B, S, H = 2, 1, 2
    C = H * 64
    qkv, dctx = _attn_inputs(B, S, H)
    ctx, lse, dqkv = _run(qkv, dctx, B, S, H, None)
    assert torch.equal(ctx, qkv[:, 2 * C:])
    assert torch.equal(dqkv[:, 2 * C:], dctx)
    q, k, v = [t.double().view(B, H, 64) for t in (qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:])]
    do = dctx.double().view(B, H, 64)
    scale = 0.125
    lse_r = scale * (q * k).sum(-1) * math.log2(math.e)
    e_lse = (lse.double().view(B, H) - lse_r).abs().max().item()
    dq = dqkv[:, :C].double().view(B, H, 64).norm(dim=-1)
    dk = dqkv[:, C:2 * C].double().view(B, H, 64).norm(dim=-1)
    bq = 1e-4 * scale * do.norm(dim=-1) * v.norm(dim=-1) * k.norm(dim=-1)
    bk = 1e-4 * scale * do.norm(dim=-1) * v.norm(dim=-1) * q.norm(dim=-1)
    _say(f"attn S=1: lse abs {e_lse:.3e} dq/bound {(dq / bq).max().item():.3e} dk/bound {(dk / bk).max().item():.3e}")
    assert e_lse < LSE_BOUND, e_lse
    assert (dq <= bq).all() and (dk <= bk).all(), (dq, bq, dk, bk)


def test_attention_tail_equals_zero_padding_bitwise():
    """S = 200 against the same rows in zero tensors of S = 256 with key_len = 200: both runs
    take the generic kernels over four key and four query blocks; the padded run's extra
    query rows have dO = 0 and add exact zeros to dK / dV, so a masking-only tail variant does
    the same arithmetic in the same order."""
    B, H, S, SP = 2, 2, 200, 256
    C = H * 64
    qkv, dctx = _attn_inputs(B, S, H)
    ctx, lse, dqkv = _run(qkv, dctx, B, S, H, [S, S])
    qkv_p = torch.zeros(B, SP, 3 * C, dtype=torch.bfloat16, device=DEV)
    dctx_p = torch.zeros(B, SP, C, dtype=torch.bfloat16, device=DEV)
    qkv_p[:, :S] = qkv.view(B, S, -1)
    dctx_p[:, :S] = dctx.view(B, S, -1)
    ctx_p, lse_p, dqkv_p = _run(qkv_p.view(B * SP, -1), dctx_p.view(B * SP, -1), B, SP, H, [S, S])
    assert torch.equal(ctx.view(B, S, -1), ctx_p.view(B, SP, -1)[:, :S])
    assert torch.equal(lse, lse_p[:, :, :S])
    dp = dqkv_p.view(B, SP, -1)
    assert torch.equal(dqkv.view(B, S, -1), dp[:, :S])
    assert (dp[:, S:, C:] == 0).all(), "dK / dV rows of the padding must be exactly zero"


@pytest.mark.parametrize("B", [1, 2])
def test_attention_reads_nothing_behind_its_tensors(B):
    """qkv, dctx, ctx and lse are leading slices of buffers whose tails are NaN: the memory a
    missing guard would read is allocated, so it shows up as NaN, not as a fault."""
    from cloud_amd.ops import raw

    H, S = 2, 100
    C = H * 64
    key_len = [S, 77][:B]
    qkv0, dctx0 = _attn_inputs(B, S, H)

    def nan_tailed(t, extra):
        buf = torch.full((t.numel() + extra,), float("nan"), dtype=t.dtype, device=DEV)
        buf[:t.numel()] = t.reshape(-1)
        out = buf[:t.numel()].view(t.shape)
        assert out.data_ptr() == buf.data_ptr() and out.is_contiguous()
        return out, buf

    qkv, _qb = nan_tailed(qkv0, 64 * 3 * C)
    dctx, _db = nan_tailed(dctx0, 64 * C)
    kl = torch.tensor(key_len, dtype=torch.int32, device=DEV)
    ctx0, lse0 = raw.attn_fwd(qkv, B, S, H, kl, 0.0, 0)
    ctx, _cb = nan_tailed(ctx0, 64 * C)
    lse, _lb = nan_tailed(lse0, 64)
    dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl, 0.0, 0)
    torch.cuda.synchronize()
    assert torch.isfinite(ctx.float()).all() and torch.isfinite(lse).all() and torch.isfinite(dqkv.float()).all()
    ctx_r, dqkv_r, lse_r, _ = _attn_ref(qkv, dctx, B, S, H, kl, 0.0, 0, 0.125)
    e_ctx = _block_err(ctx.double().view(B, S, H, 64).permute(0, 2, 1, 3), ctx_r)
    e_d = _block_err(dqkv.double().view(B, S, 3, H, 64).permute(2, 0, 3, 1, 4), dqkv_r)
    e_lse = (lse.double() - lse_r).abs().max().item()
    _say(f"attn NaN-tails B={B}: ctx/block {e_ctx.max().item():.3e} dqkv/block {e_d.max().item():.3e} "
         f"lse abs {e_lse:.3e}")
    assert e_lse < LSE_BOUND and e_ctx.max().item() < CTX_BOUND and e_d.max().item() < DQKV_BOUND


def test_attention_batch_entries_do_not_see_each_other():
    """Entry 0 of a B = 3 run equals a B = 1 run on its rows bitwise (same bh indices and S,
    so the same dropout indices): no tail store or load crosses into the next entry."""
    B, S, H, p = 3, 100, 2, 0.1
    qkv, dctx = _attn_inputs(B, S, H)
    ctx3, lse3, dqkv3 = _run(qkv, dctx, B, S, H, [100, 64, 37], p, seed=99)
    ctx1, lse1, dqkv1 = _run(qkv[:S].contiguous(), dctx[:S].contiguous(), 1, S, H, [100], p, seed=99)
    assert torch.equal(ctx3[:S], ctx1)
    assert torch.equal(lse3[:1], lse1)
    assert torch.equal(dqkv3[:S], dqkv1)


def test_ops_attention_native_matches_raw():
    from cloud_amd.ops import attention, raw

    B, S, H, p, seed = 2, 100, 2, 0.1, 1234
    qkv, dctx = _attn_inputs(B, S, H)
    key_len = torch.tensor([100, 61], dtype=torch.int32, device=DEV)
    ctx_r, lse_r = raw.attn_fwd(qkv, B, S, H, key_len, p, seed)
    dqkv_r = raw.attn_bwd(qkv, ctx_r, dctx, lse_r, B, S, H, key_len, p, seed)
    x = qkv.view(B, S, -1).clone().requires_grad_()
    out = attention(x, H, key_len, dropout_p=p, seed=seed)
    assert out.shape == (B, S, H * 64) and out.dtype == torch.bfloat16
    out.backward(dctx.view(B, S, -1))
    torch.cuda.synchronize()
    assert torch.equal(out.detach().view(B * S, -1), ctx_r)
    assert torch.equal(x.grad.view(B * S, -1), dqkv_r)
    with torch.no_grad():
        a = attention(x, H, key_len, dropout_p=0.5, training=False)
        b = attention(x, H, key_len, dropout_p=0.0)
    assert torch.equal(a, b)


def test_ops_attention_other_head_dim_takes_reference():
    from cloud_amd.ops import attention

    B, S, H, D = 2, 100, 2, 32
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B, S, 3 * H * D, generator=g) * 0.5).to(torch.bfloat16).to(DEV)
    key_len = torch.tensor([100, 61], device=DEV)
    out = attention(qkv, H, key_len)
    q, k, v = qkv.double().view(B, S, 3, H, D).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-1, -2)) / math.sqrt(D)
    pad = torch.arange(S, device=DEV)[None, :] >= key_len[:, None]
    sc = sc + torch.zeros(B, 1, 1, S, dtype=torch.float64, device=DEV).masked_fill(pad[:, None, None, :], float("-inf"))
    ref = (sc.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B, S, H * D)
    e = ((out.double() - ref).norm() / ref.norm()).item()
    _say(f"ops.attention D=32 reference path: rel {e:.3e}")
    assert out.shape == (B, S, H * D) and e < 3e-2, e


# --------------------------------------------------------------------------- BERT


@pytest.mark.parametrize("arena", [False, True])
@pytest.mark.parametrize("B,S,cuts", [(4, 100, (100, 77, 64, 100)), (3, 50, (50, 33, 17))])
def test_bert_tiny_native_matches_torch_any_length(B, S, cuts, arena):
    """The pattern and bounds of test_bert_tiny_native_matches_torch at sequence lengths that
    are no multiple of 64 (B * S = 150 is no multiple of 8 either)."""
    from cloud_amd.models.bert import BertConfig, BertForSequenceClassification
    from cloud_amd.optim import AdamW

    torch.manual_seed(7)
    cfg = BertConfig.tiny(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, num_labels=3)
    m = BertForSequenceClassification(cfg, device=DEV)
    opt = AdamW(m, learning_rate=0.0) if arena else None
    ids = torch.randint(0, cfg.vocab_size, (B, S), device=DEV)
    tts = torch.randint(0, 2, (B, S), device=DEV)
    am = torch.ones(B, S, device=DEV, dtype=torch.long)
    for b, c in enumerate(cuts):
        am[b, c:] = 0
    labels = torch.randint(0, 3, (B,), device=DEV)
    native = bool(m._native_ok(ids))
    _say(f"bert tiny B={B} S={S}: {'native' if native else 'torch'} path")
    if S == 100:
        assert native

    def grads():
        return {n: (p.grad.detach().float().clone() if p.grad is not None else None) for n, p in m.named_parameters()}

    if opt is not None:
        opt.zero_grad()
    logits = m(ids, tts, am)
    F.cross_entropy(logits, labels).backward()
    g_nat = grads()
    if opt is not None:
        opt.zero_grad()
    else:
        m.zero_grad(set_to_none=True)
    logits_r = m._torch_forward(ids, tts, am)
    F.cross_entropy(logits_r, labels).backward()
    g_ref = grads()
    assert rel(logits, logits_r) < 3e-2
    for n in g_ref:
        assert g_nat[n] is not None, n
        assert rel(g_nat[n], g_ref[n]) < 8e-2, (n, rel(g_nat[n], g_ref[n]))


@contextlib.contextmanager
def counted(monkeypatch):
    from cloud_amd.ops import raw

    calls = {}

    def wrap(owner, name):
        orig = getattr(owner, name)

        def f(*a, **k):
            calls[name] = calls.get(name, 0) + 1
            return orig(*a, **k)

        monkeypatch.setattr(owner, name, f)

    for name in ("mm", "matmul", "bmm", "addmm", "conv2d"):
        wrap(torch, name)
    for name in ("linear", "conv2d"):
        wrap(F, name)
    wrap(raw, "_plain_lib")
    yield calls


def test_bert_step_at_length_100_uses_no_library_gemm(monkeypatch):
    from cloud_amd.models.bert import BertConfig, BertForSequenceClassification
    from cloud_amd.ops import softmax_cross_entropy
    from cloud_amd.optim import AdamW

    torch.manual_seed(0)
    cfg = BertConfig.base(num_hidden_layers=2, num_labels=2)
    m = BertForSequenceClassification(cfg, device="cuda")
    opt = AdamW(m, learning_rate=2e-5, weight_decay=0.01)
    ids = torch.randint(1000, 30522, (16, 100), device="cuda")
    tts = torch.zeros_like(ids)
    am = torch.ones_like(ids)
    labels = torch.randint(0, 2, (16,), device="cuda")
    assert m._native_ok(ids)
    with counted(monkeypatch) as calls:
        for _ in range(2):
            opt.zero_grad()
            loss, _ = softmax_cross_entropy(m(ids, tts, am), labels, denom=16)
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
    assert not calls, calls
    assert math.isfinite(float(loss.detach()))
