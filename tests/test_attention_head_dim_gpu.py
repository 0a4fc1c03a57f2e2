"""Attention kernels of attn.hip at head dimensions 32 and 128 (``raw.attn_*`` / ``raw.attn_cross_*``
with ``head_dim=``, ``ops.attention`` and ``ops.cross_attention``): the generic kernel family with
the head dimension as a compile-time parameter.  D = 32 runs with H = 3 (C = 96, packed pitch 288,
head offsets that are no powers of two), D = 128 with H = 2.

Inputs follow test_attention_cross_gpu (seeded host generator, ``randn * 0.5`` in bf16,
``dctx = randn``); the per-(batch, head) block metric ``_block_err`` and the bounds (CTX_BOUND 1e-2,
DQKV_BOUND 2e-2, LSE_BOUND 1e-3) are those of test_bert_kernel_edges_gpu, the reference is fp64
attention of the same bf16 inputs with the kernels' dropout mask (``raw.dropout_mask``).  The causal
cases follow test_attention_causal_gpu, the masked ones test_attention_mask_gpu (exact zeros for
hidden rows and unseen keys).  As there, no case has ``key_len = 1`` together with dropout, and
outside the causal test no live row sees fewer than 5 keys (the masked cases: at least 8).

S = T = 1 is the one case the block metric cannot take for dQ and dK (the only probability is 1, both
are exactly zero in every block): as in test_attention_cross_gpu they are held to DQKV_BOUND of the
magnitude of the terms that cancel, scale * |dO| |V| |K| per block.

Beyond the bounds the new head dimensions are held to bitwise statements that need no tolerance:
a problem embedded in the next wider head dimension with zero columns gives the same bits (the
extra k-steps and output tiles only add exact zeros, in ascending k-step order, so a difference is
an indexing error and not rounding); self-attention equals cross-attention on the column views
(at S = 64 and 128 too: no head dimension but 64 reaches the one-workgroup kernels); the tail
variant equals zero padding; the ops return the raw results.

Before the first run on a GPU a bf16-faithful fp32 emulation of the kernels (P * mask and dS rounded
to bf16 before their matmuls; ctx, dQ, dK, dV rounded to bf16; Dv from the rounded context; the
causal context divided by the sum of the rounded probabilities; the same dropout hash) was run on the
CPU for every case of this module.  Its worst per-block figures:

    group                    D     ctx       dQ        dK        dV        lse abs
    self                     32    2.63e-03  2.62e-03  2.88e-03  2.79e-03  6.1e-07
    self                     128   2.58e-03  2.58e-03  2.62e-03  2.63e-03  7.8e-07
    cross                    32    2.64e-03  2.67e-03  2.98e-03  2.71e-03  5.7e-07
    cross                    128   2.45e-03  3.53e-03  3.39e-03  2.52e-03  6.0e-07
    causal                   32    2.65e-03  4.60e-03  3.82e-03  2.69e-03  6.8e-07
    causal                   128   2.49e-03  3.61e-03  3.84e-03  2.52e-03  6.2e-07
    masked                   32    2.36e-03  2.46e-03  2.44e-03  2.44e-03  6.5e-07
    masked                   128   2.36e-03  2.44e-03  2.45e-03  2.40e-03  5.8e-07
    bounds                         1e-2      2e-2      2e-2      2e-2      1e-3

("self" includes the explicit-scale case, "causal" the causal runs at S = 64 / 100 / 128 of
test_self_equals_cross_attention_bitwise; the emulation takes one pass over the whole key row where
the kernels rescale per 64-key block.)  Every block of every case stays within the bounds -- the
worst, 4.6e-3, is a causal dQ block with dropout -- so no block carries an emulation-derived bound.
For S = T = 1 the emulation gives 4.6e-9 (D = 32) and 1.6e-8 (D = 128) for dQ and dK in the units
above at p = 0, and 1.0e-3 / 3.0e-4 at p = 0.1.

Worst per-block figures observed on an MI355X (each test prints its own before asserting):

    group                    D     ctx       dQ        dK        dV        lse abs
    self                     32    2.63e-03  2.62e-03  2.88e-03  2.79e-03  8.3e-07
    self                     128   2.58e-03  2.58e-03  2.62e-03  2.63e-03  8.2e-07
    cross                    32    2.64e-03  2.67e-03  2.98e-03  2.71e-03  7.8e-07
    cross                    128   2.45e-03  3.53e-03  3.39e-03  2.52e-03  7.7e-07
    causal                   32    2.65e-03  4.64e-03  3.96e-03  2.58e-03  8.1e-07
    causal                   128   2.47e-03  3.61e-03  3.84e-03  2.49e-03  8.1e-07
    masked                   32    2.37e-03  2.45e-03  2.45e-03  2.44e-03  7.9e-07
    masked                   128   2.35e-03  2.44e-03  2.45e-03  2.40e-03  7.4e-07
    bounds                         1e-2      2e-2      2e-2      2e-2      1e-3

The kernels' figures are the emulation's to two digits in every group; the log-sum-exp differs by
the kernels' exp2f / log2f (7.4e-7 .. 8.3e-7 against 5.7e-7 .. 7.8e-7).  The Keras layer's figures are
in test_keras_mha_head_dim_gpu.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CTX_BOUND, DQKV_BOUND, LSE_BOUND = 1e-2, 2e-2, 1e-3  # test_bert_kernel_edges_gpu
HEADS = {32: 3, 128: 2}
DIMS = [32, 128]


def _say(*a):
    print("[head-dim]", *a, flush=True)


def _block_err(got, ref):
    """test_bert_kernel_edges_gpu._block_err: per (batch, head) block
    ||got - ref|| / max(||ref||, median block ||ref||)."""
    d = (got - ref).flatten(-2).norm(dim=-1)
    n = ref.flatten(-2).norm(dim=-1)
    med = torch.quantile(n.flatten(-2), 0.5, dim=-1)
    assert (med > 0).all(), "median block norm is zero"
    return d / torch.maximum(n, med[..., None, None])


def _kl(key_len):
    return None if key_len is None else torch.tensor(key_len, dtype=torch.int32, device=DEV)


def _cross_inputs(B, T, S, D, seed=1):
    C = HEADS[D] * D
    g = torch.Generator().manual_seed(seed)  # host generator: the same inputs on every machine
    q = (torch.randn(B * T, C, generator=g) * 0.5).to(torch.bfloat16)
    kv = (torch.randn(B * S, 2 * C, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B * T, C, generator=g).to(torch.bfloat16)
    return q.to(DEV), kv.to(DEV), dctx.to(DEV)


def _self_inputs(B, S, D, seed=1):
    C = HEADS[D] * D
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(B * S, 3 * C, generator=g) * 0.5).to(torch.bfloat16)
    dctx = torch.randn(B * S, C, generator=g).to(torch.bfloat16)
    return qkv.to(DEV), dctx.to(DEV)


def _keep(B, H, T, S, p, seed):
    """The kernels' keep mask [B, H, T, S] (element index (b*H + h)*T*S + q*S + key)."""
    from cloud_amd.ops import raw

    return raw.dropout_mask(B * H * T * S, p, seed, device=DEV).view(B, H, T, S)


def _allowed(B, H, T, S, key_len, causal=False, mask=None):
    """The full visibility [B, H, T, S]: key < key_len (clamped to [1, S]), key <= q, mask."""
    pos = torch.arange(S, device=DEV)
    a = torch.ones(B, H, T, S, dtype=torch.bool, device=DEV)
    if key_len is not None:
        kl = torch.tensor(key_len, device=DEV).clamp(1, S)
        a = a & (pos[None, :] < kl[:, None])[:, None, None, :]
    if causal:
        a = a & (pos[None, :] <= torch.arange(T, device=DEV)[:, None])[None, None]
    if mask is not None:
        a = a & mask.to(DEV)
    return a


def _heads(x, B, L, H, D):
    return x.reshape(B, L, H, D).permute(0, 2, 1, 3)


def _ref(q, kv, dctx, B, T, S, D, allowed, p, seed, scale):
    """fp64 attention of the bf16 inputs over the allowed keys: q [B*T, >= C] and kv [B*S, >= 2C]
    may be column views.  Returns ctx [B,H,T,D], dq [B,H,T,D], dkv [2,B,H,S,D] (K, V) and the
    log2-domain log-sum-exp [B,H,T] (0 for a row that sees nothing)."""
    H = HEADS[D]
    q_ = _heads(q.double(), B, T, H, D)
    k_, v_ = kv.double().reshape(B, S, 2, H, D).permute(2, 0, 3, 1, 4)
    qd, k, v = [t.clone().requires_grad_() for t in (q_, k_, v_)]
    live = allowed.any(-1, keepdim=True)
    sc = ((qd @ k.transpose(-1, -2)) * scale).masked_fill(~allowed & live, float("-inf"))
    lse2 = (torch.logsumexp(sc, -1) / math.log(2.0)).detach() * live[..., 0]
    att = sc.softmax(-1) * (allowed & live)
    if p > 0:
        att = att * _keep(B, H, T, S, p, seed).double() / (1.0 - p)
    out = att @ v
    out.backward(_heads(dctx.double(), B, T, H, D))
    return out.detach(), qd.grad, torch.stack([k.grad, v.grad], 0), lse2


def _run_cross(q, kv, dctx, B, T, S, D, key_len, p=0.0, seed=1234, scale=None, mask=None):
    from cloud_amd.ops import raw

    H, kl = HEADS[D], _kl(key_len)
    ctx, lse = raw.attn_cross_fwd(q, kv, B, T, S, H, kl, p, seed, scale=scale, mask=mask, head_dim=D)
    dq, dkv = raw.attn_cross_bwd(q, kv, ctx, dctx, lse, B, T, S, H, kl, p, seed, scale=scale, mask=mask, head_dim=D)
    torch.cuda.synchronize()
    return ctx, lse, dq, dkv


def _run_self(qkv, dctx, B, S, D, key_len, p=0.0, seed=1234, scale=None, causal=False):
    """-> ctx, lse, dq, dkv (the column views of dqkv)"""
    from cloud_amd.ops import raw

    H, kl = HEADS[D], _kl(key_len)
    C = H * D
    ctx, lse = raw.attn_fwd(qkv, B, S, H, kl, p, seed, scale=scale, causal=causal, head_dim=D)
    dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl, p, seed, scale=scale, causal=causal, head_dim=D)
    torch.cuda.synchronize()
    return ctx, lse, dqkv[:, :C], dqkv[:, C:]


def _check(got, q, kv, dctx, B, T, S, D, allowed, p, seed, scale, tag):
    """Hold ctx, lse, dq, dkv (``got``) to the fp64 reference; exact zeros where nothing is seen."""
    H = HEADS[D]
    ctx, lse, dq, dkv = got
    sc = 1.0 / math.sqrt(D) if scale is None else scale
    ctx_r, dq_r, dkv_r, lse_r = _ref(q, kv, dctx, B, T, S, D, allowed, p, seed, sc)
    ctx_g, dq_g = _heads(ctx.double(), B, T, H, D), _heads(dq.double(), B, T, H, D)
    dkv_g = dkv.double().reshape(B, S, 2, H, D).permute(2, 0, 3, 1, 4)
    e_ctx = _block_err(ctx_g, ctx_r)
    e_lse = (lse.double() - lse_r).abs().max().item()
    if T == 1 and S == 1:
        # dQ = dK = 0 exactly (module docstring): in units of the terms that cancel, per block
        nrm = lambda t: t.flatten(-2).norm(dim=-1)  # noqa: E731
        g = _heads(dctx.double(), B, T, H, D)
        k_r, v_r = kv.double().reshape(B, S, 2, H, D).permute(2, 0, 3, 1, 4)
        q_r = _heads(q.double(), B, T, H, D)
        assert (dq_r == 0).all() and (dkv_r[0] == 0).all()
        e_dq = nrm(dq_g) / (sc * nrm(g) * nrm(v_r) * nrm(k_r))
        e_dk = nrm(dkv_g[0]) / (sc * nrm(g) * nrm(v_r) * nrm(q_r))
        e_dv = _block_err(dkv_g[1], dkv_r[1])
    else:
        e_dq = _block_err(dq_g, dq_r)
        e_dk, e_dv = _block_err(dkv_g, dkv_r)
    _say(f"{tag}: ctx/block max {e_ctx.max().item():.3e} dq {e_dq.max().item():.3e} dk {e_dk.max().item():.3e} "
         f"dv {e_dv.max().item():.3e} lse abs {e_lse:.3e}")
    for t in (ctx, lse, dq, dkv):
        assert torch.isfinite(t.float()).all()
    dead = ~allowed.any(-1)                                # [B, H, T]
    assert (ctx_g[dead] == 0).all() and (dq_g[dead] == 0).all() and (lse[dead] == 0).all()
    unseen = ~allowed.any(2)                               # [B, H, S]: through key_len or the mask
    assert (dkv_g[:, unseen] == 0).all(), "dK / dV rows of unseen keys must be exactly zero"
    assert e_lse < LSE_BOUND, e_lse
    assert e_ctx.max().item() < CTX_BOUND, e_ctx
    for name, e in (("dq", e_dq), ("dk", e_dk), ("dv", e_dv)):
        assert (e < DQKV_BOUND).all(), (name, e)
    return e_ctx.max().item(), e_dq.max().item(), e_dk.max().item(), e_dv.max().item(), e_lse


# key_len puts a boundary inside a block and on a block edge wherever S has one
SELF_CASES = [
    (1, None),
    (64, [64, 33, 17]),
    (65, [65, 64, 17]),
    (128, [128, 64, 65, 100]),
    (129, [129, 128, 65, 17]),
    (200, [200, 64, 130, 7]),
]


def _self_case(D, S, key_len, p, scale=None, causal=False, tag="self"):
    B = 4 if key_len is None else len(key_len)
    H, C, seed = HEADS[D], HEADS[D] * D, 1234
    assert key_len is None or not (p > 0 and 1 in key_len)
    assert causal or key_len is None or min(key_len) >= 5
    qkv, dctx = _self_inputs(B, S, D)
    got = _run_self(qkv, dctx, B, S, D, key_len, p, seed, scale, causal)
    allowed = _allowed(B, H, S, S, key_len, causal)
    return _check(got, qkv[:, :C], qkv[:, C:], dctx, B, S, S, D, allowed, p, seed, scale,
                  f"{tag} D={D} S={S} key_len={key_len} p={p} scale={scale}")


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,key_len", SELF_CASES)
@pytest.mark.parametrize("D", DIMS)
def test_self_attention_vs_fp64(D, S, key_len, p):
    """The generic forward, prep, dK/dV and dQ kernels on the packed projection at every S (no
    head dimension but 64 has one-workgroup kernels); dK / dV rows of keys >= key_len are zero."""
    _self_case(D, S, key_len, p)


@pytest.mark.parametrize("D", DIMS)
def test_self_attention_explicit_scale(D):
    from cloud_amd.ops import raw

    S, key_len, p = 200, [200, 179, 7], 0.1
    _self_case(D, S, key_len, p, scale=0.2, tag="self-scale")
    qkv, _ = _self_inputs(3, S, D)
    a, _ = raw.attn_fwd(qkv, 3, S, HEADS[D], _kl(key_len), p, 1234, scale=0.2, head_dim=D)
    b, _ = raw.attn_fwd(qkv, 3, S, HEADS[D], _kl(key_len), p, 1234, head_dim=D)
    c, _ = raw.attn_fwd(qkv, 3, S, HEADS[D], _kl(key_len), p, 1234, scale=1.0 / math.sqrt(D), head_dim=D)
    assert not torch.equal(a, b) and torch.equal(b, c)  # the default scale is 1 / sqrt(D)


CROSS_CASES = [
    (1, 200, [200, 65, 7]),
    (65, 63, [63, 17, 62]),
    (128, 64, [64, 5, 33]),
    (70, 100, [100, 79, 7]),
]


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("T,S,key_len", CROSS_CASES)
@pytest.mark.parametrize("D", DIMS)
def test_cross_attention_vs_fp64(D, T, S, key_len, p):
    B, H, seed = len(key_len), HEADS[D], 1234
    assert min(key_len) >= 5
    q, kv, dctx = _cross_inputs(B, T, S, D)
    got = _run_cross(q, kv, dctx, B, T, S, D, key_len, p, seed)
    _check(got, q, kv, dctx, B, T, S, D, _allowed(B, H, T, S, key_len), p, seed, None,
           f"cross D={D} T={T} S={S} key_len={key_len} p={p}")


CAUSAL_CASES = [
    (65, None, 0.0), (65, [65, 64, 33, 17], 0.1),
    (129, None, 0.0), (129, [129, 128, 65, 17], 0.1),
    (200, None, 0.0), (200, [200, 193, 64, 130], 0.1),
]


@pytest.mark.parametrize("S,key_len,p", CAUSAL_CASES)
@pytest.mark.parametrize("D", DIMS)
def test_causal_attention_vs_fp64(D, S, key_len, p):
    """Block skipping and the diagonal block do not depend on the head dimension; bounds and
    notes of test_attention_causal_gpu (rows with one or two visible keys are part of it)."""
    _self_case(D, S, key_len, p, causal=True, tag="causal")


def _designed_mask(shape, T, S):
    """Density 0.5, query 30 sees nothing, no query sees key 77; every other row has >= 8 keys."""
    g = torch.Generator().manual_seed(1001)
    m = torch.rand(*shape, generator=g) < 0.5
    m[..., 30, :] = False
    m[..., :, 77] = False
    return m


@pytest.mark.parametrize("per_head", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_masked_attention_vs_fp64(D, per_head):
    """A [B, 1, T, S] and a per-head [1, H, T, S] byte mask, read through broadcast strides."""
    B, T, S, p, seed, H = 2, 70, 100, 0.1, 1234, HEADS[D]
    key_len = [100, 83]
    q, kv, dctx = _cross_inputs(B, T, S, D)
    mask = _designed_mask((1, H, T, S) if per_head else (B, 1, T, S), T, S).to(DEV)
    allowed = _allowed(B, H, T, S, key_len, mask=mask)
    vis = allowed.sum(-1)
    assert (vis[vis > 0] >= 8).all() and (vis == 0).any() and (~allowed.any(2)).any()
    got = _run_cross(q, kv, dctx, B, T, S, D, key_len, p, seed, mask=mask)
    _check(got, q, kv, dctx, B, T, S, D, allowed, p, seed, None, f"masked D={D} mask={tuple(mask.shape)} p={p}")
    ctx, lse, dq, dkv = got
    assert (ctx.view(B, T, -1)[:, 30] == 0).all() and (dq.view(B, T, -1)[:, 30] == 0).all()
    assert (lse[:, :, 30] == 0).all() and (dkv.view(B, S, -1)[:, 77] == 0).all()
    assert (ctx.view(B, T, -1)[:, 31] != 0).any() and (dkv.view(B, S, -1)[:, 76] != 0).any()


# --------------------------------------------------------------------------- bitwise statements

def _widen(x, H, D, DW):
    """[rows, n*H*D] -> [rows, n*H*DW]: every head's D columns followed by DW - D zero columns."""
    rows = x.shape[0]
    w = torch.zeros(rows, x.shape[1] // D, DW, dtype=x.dtype, device=x.device)
    w[:, :, :D] = x.view(rows, -1, D)
    return w.view(rows, -1)


def _narrow(x, D, DW):
    """-> (the D data columns of every head, the DW - D extension columns)"""
    v = x.reshape(x.shape[0], -1, DW)
    return v[:, :, :D].reshape(x.shape[0], -1), v[:, :, D:]


def _raw_cross(q, kv, dctx, B, T, S, H, D, kl, p, seed, scale):
    from cloud_amd.ops import raw

    ctx, lse = raw.attn_cross_fwd(q, kv, B, T, S, H, kl, p, seed, scale=scale, head_dim=D)
    dq, dkv = raw.attn_cross_bwd(q, kv, ctx, dctx, lse, B, T, S, H, kl, p, seed, scale=scale, head_dim=D)
    return ctx, lse, dq, dkv


def _raw_self(qkv, dctx, B, S, H, D, kl, p, seed, scale, causal):
    from cloud_amd.ops import raw

    ctx, lse = raw.attn_fwd(qkv, B, S, H, kl, p, seed, scale=scale, causal=causal, head_dim=D)
    dqkv = raw.attn_bwd(qkv, ctx, dctx, lse, B, S, H, kl, p, seed, scale=scale, causal=causal, head_dim=D)
    return ctx, lse, dqkv


def _rand_bf16(g, rows, cols, mul=0.5):
    return (torch.randn(rows, cols, generator=g) * mul).to(torch.bfloat16).to(DEV)


@pytest.mark.parametrize("D,DW,H", [(64, 128, 2), (32, 64, 3)])
def test_zero_extension_equals_the_narrower_kernel_cross(D, DW, H):
    """A head-dim D problem inside head dim DW (columns D .. DW - 1 of every head of Q, K, V and dO
    zero, the narrow problem's scale passed explicitly), at a tail shape with key_len and dropout:
    the data columns and the log-sum-exp are bit-equal to the D kernels' output, the extension
    columns exactly zero."""
    B, T, S, p, seed, scale = 2, 70, 100, 0.1, 4321, 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(5)
    q, kv, dctx = _rand_bf16(g, B * T, H * D), _rand_bf16(g, B * S, 2 * H * D), _rand_bf16(g, B * T, H * D, 1.0)
    kl = _kl([100, 61])
    ctx, lse, dq, dkv = _raw_cross(q, kv, dctx, B, T, S, H, D, kl, p, seed, scale)
    ctx_w, lse_w, dq_w, dkv_w = _raw_cross(_widen(q, H, D, DW), _widen(kv, H, D, DW), _widen(dctx, H, D, DW), B, T, S,
                                           H, DW, kl, p, seed, scale)
    torch.cuda.synchronize()
    assert torch.equal(lse_w, lse)
    for name, narrow, wide in (("ctx", ctx, ctx_w), ("dq", dq, dq_w), ("dkv", dkv, dkv_w)):
        data, ext = _narrow(wide, D, DW)
        assert torch.equal(data, narrow), name
        assert (ext == 0).all(), name
        assert (narrow != 0).any()


@pytest.mark.parametrize("D,DW,H", [(64, 128, 2), (32, 64, 3)])
def test_zero_extension_equals_the_narrower_kernel_causal_self(D, DW, H):
    """The same statement for causal self-attention on the packed projection at S = 129."""
    B, S, p, seed, scale = 2, 129, 0.1, 4321, 1.0 / math.sqrt(D)
    g = torch.Generator().manual_seed(6)
    qkv, dctx = _rand_bf16(g, B * S, 3 * H * D), _rand_bf16(g, B * S, H * D, 1.0)
    kl = _kl([129, 70])
    ctx, lse, dqkv = _raw_self(qkv, dctx, B, S, H, D, kl, p, seed, scale, True)
    ctx_w, lse_w, dqkv_w = _raw_self(_widen(qkv, H, D, DW), _widen(dctx, H, D, DW), B, S, H, DW, kl, p, seed, scale,
                                     True)
    torch.cuda.synchronize()
    assert torch.equal(lse_w, lse)
    for name, narrow, wide in (("ctx", ctx, ctx_w), ("dqkv", dqkv, dqkv_w)):
        data, ext = _narrow(wide, D, DW)
        assert torch.equal(data, narrow), name
        assert (ext == 0).all(), name
        assert (narrow != 0).any()


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("S", [64, 100, 128])
@pytest.mark.parametrize("D", DIMS)
def test_self_equals_cross_attention_bitwise(D, S, causal):
    """``raw.attn_fwd`` / ``raw.attn_bwd`` against ``raw.attn_cross_*`` on ``qkv[:, :C]`` /
    ``qkv[:, C:]``: the same generic instantiation, so the same bits -- at S = 64 and 128 as well,
    where head dim 64 would take the one-workgroup kernels (which sum in another order, and index
    64-wide heads).  Cross-attention has no causal mode, so the causal runs at these lengths are
    held to the fp64 reference instead."""
    B, p, seed, H = 3, 0.1, 4321, HEADS[D]
    C = H * D
    qkv, dctx = _self_inputs(B, S, D)
    key_len = [S, S // 2 + 1, 37]
    ctx0, lse0, dq0, dkv0 = _run_self(qkv, dctx, B, S, D, key_len, p, seed, causal=causal)
    q, kv = qkv[:, :C], qkv[:, C:]
    assert q.stride(0) == 3 * C and kv.stride(0) == 3 * C and not kv.is_contiguous()
    if not causal:
        ctx, lse, dq, dkv = _run_cross(q, kv, dctx, B, S, S, D, key_len, p, seed)
        assert torch.equal(ctx, ctx0) and torch.equal(lse, lse0)
        assert torch.equal(dq, dq0) and torch.equal(dkv, dkv0)
        assert dq.is_contiguous() and dkv.is_contiguous()
    else:
        allowed = _allowed(B, H, S, S, key_len, causal=True)
        _check((ctx0, lse0, dq0, dkv0), q, kv, dctx, B, S, S, D, allowed, p, seed, None,
               f"causal-short D={D} S={S} key_len={key_len} p={p}")


@pytest.mark.parametrize("D", DIMS)
def test_tail_equals_zero_padding_bitwise(D):
    """S = 65 against the same rows inside zero tensors of 128 rows with key_len = 65."""
    B, S, SP, H = 2, 65, 128, HEADS[D]
    C = H * D
    qkv, dctx = _self_inputs(B, S, D)
    ctx, lse, dq, dkv = _run_self(qkv, dctx, B, S, D, [S, S], 0.0)
    qkv_p = torch.zeros(B, SP, 3 * C, dtype=torch.bfloat16, device=DEV)
    dctx_p = torch.zeros(B, SP, C, dtype=torch.bfloat16, device=DEV)
    qkv_p[:, :S] = qkv.view(B, S, -1)
    dctx_p[:, :S] = dctx.view(B, S, -1)
    ctx_p, lse_p, dq_p, dkv_p = _run_self(qkv_p.view(B * SP, -1), dctx_p.view(B * SP, -1), B, SP, D, [S, S], 0.0)
    assert torch.equal(ctx.view(B, S, -1), ctx_p.view(B, SP, -1)[:, :S])
    assert torch.equal(lse, lse_p[:, :, :S])
    assert torch.equal(dq.reshape(B, S, -1), dq_p.reshape(B, SP, -1)[:, :S])
    dp = dkv_p.reshape(B, SP, -1)
    assert torch.equal(dkv.reshape(B, S, -1), dp[:, :S])
    assert (dp[:, S:] == 0).all(), "dK / dV rows of the padding must be exactly zero"


# --------------------------------------------------------------------------- ops level

@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_ops_attention_native_matches_raw(D, causal):
    from cloud_amd.ops import attention

    B, S, p, seed, H = 2, 100, 0.1, 1234, HEADS[D]
    qkv, dctx = _self_inputs(B, S, D)
    ctx_r, _, dq_r, dkv_r = _run_self(qkv, dctx, B, S, D, [100, 61], p, seed, causal=causal)
    x = qkv.view(B, S, -1).clone().requires_grad_()
    out = attention(x, H, _kl([100, 61]), dropout_p=p, seed=seed, causal=causal)
    assert out.shape == (B, S, H * D) and out.dtype == torch.bfloat16
    out.backward(dctx.view(B, S, -1))
    torch.cuda.synchronize()
    assert torch.equal(out.detach().view(B * S, -1), ctx_r)
    assert torch.equal(x.grad.view(B * S, -1), torch.cat([dq_r, dkv_r], dim=1))


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("D", DIMS)
def test_ops_cross_attention_native_matches_raw(D, masked):
    from cloud_amd.ops import cross_attention

    B, T, S, p, seed, H = 2, 70, 100, 0.1, 1234, HEADS[D]
    q, kv, dctx = _cross_inputs(B, T, S, D)
    mask = _designed_mask((B, 1, T, S), T, S).to(DEV) if masked else None
    ctx_r, _, dq_r, dkv_r = _run_cross(q, kv, dctx, B, T, S, D, [100, 61], p, seed, mask=mask)
    x = q.view(B, T, -1).clone().requires_grad_()
    y = kv.view(B, S, -1).clone().requires_grad_()
    out = cross_attention(x, y, H, _kl([100, 61]), dropout_p=p, seed=seed, mask=mask)
    assert out.shape == (B, T, H * D) and out.dtype == torch.bfloat16
    out.backward(dctx.view(B, T, -1))
    torch.cuda.synchronize()
    assert torch.equal(out.detach().view(B * T, -1), ctx_r)
    assert torch.equal(x.grad.view(B * T, -1), dq_r)
    assert torch.equal(y.grad.view(B * S, -1), dkv_r)
