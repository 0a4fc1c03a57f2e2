"""The 256 x 256 two-phase GEMM core (csrc/include/ca_gemm256p8.h, core kind 6 = vp8) forced on
every GEMM with M, N >= 256 -- against a plain PyTorch fp32
GEMM of the same bf16 operands: forward (NT), input grad (NN), weight grad (TN, split-K fp32
slabs), the fused bias + activation and BN-statistics epilogues, ragged M / N / K (partial
tiles, K tails read as zeros through the buffer range check), one to many K tiles -- plus
the default dispatch (core kind 5) on a shape that selects the 256 core by itself, and the core
kinds and transform-A mode that no longer exist."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[6], ids=["p8"])
def core256(request):
    """Force the 256 x 256 two-phase core (6 = vp8, csrc/include/ca_gemm256p8.h) on every GEMM
    with M, N >= 256."""
    from cloud_amd.ops import _ext

    ext = _ext.load(required=True)
    prev = ext.gemm_set_core(request.param)
    assert prev >= 0
    yield request.param
    ext.gemm_set_core(prev)


def _rel(a, b):
    return float((a.float() - b).norm() / b.norm())


@pytest.mark.parametrize("M,N,K", [(512, 512, 64), (1024, 768, 2048), (300, 264, 200), (4096, 256, 1024),
                                   (777, 1032, 4104)])
def test_256_forward_and_input_grad(core256, M, N, K):
    from cloud_amd.ops import raw

    torch.manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(N, K, device="cuda").to(torch.bfloat16)
    y = raw.gemm(a, w)
    assert _rel(y, a.float() @ w.float().t()) < 5e-3
    dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    dx = raw.gemm(dy, w, layout=raw.NN)
    assert _rel(dx, dy.float() @ w.float()) < 5e-3


@pytest.mark.parametrize("M,N,K", [(8192, 512, 256), (2000, 1024, 512)])
def test_256_weight_grad_splitk(core256, M, N, K):
    from cloud_amd.ops import raw

    torch.manual_seed(M + N)
    dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    x = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    gw = torch.zeros(N, K, device="cuda", dtype=torch.bfloat16)
    raw.wgrad_into(dy, x, gw, beta=0.0)
    assert _rel(gw, dy.float().t() @ x.float()) < 5e-3


def test_256_bias_act_and_stats_epilogues(core256):
    from cloud_amd.ops import raw

    torch.manual_seed(7)
    M, N, K = 1024, 512, 320
    a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(N, K, device="cuda").to(torch.bfloat16)
    bias = torch.randn(N, device="cuda")
    ref = a.float() @ w.float().t() + bias
    y = raw.gemm(a, w, bias=bias, act="relu")
    assert _rel(y, torch.relu(ref)) < 5e-3
    st = raw.stats_buffer(M, N, a.device)
    y2 = raw.gemm(a, w, stats=st)
    z = (a.float() @ w.float().t())
    s_sum = st.view(-1, 2, N)[:, 0].sum(0)
    s_sq = st.view(-1, 2, N)[:, 1].sum(0)
    assert _rel(y2, z) < 5e-3
    assert _rel(s_sum, y2.float().sum(0)) < 1e-3
    assert _rel(s_sq, (y2.float() ** 2).sum(0)) < 1e-3


def test_default_dispatch_selects_256_on_large_gemm():
    """8192 x 2048 x 1024: 256 tiles of 256 x 256 (one full round), 32 K tiles -> the default
    dispatch (kind 5) uses the two-phase 256 core; result checked against fp32."""
    from cloud_amd.ops import _ext, raw

    ext = _ext.load(required=True)
    prev = ext.gemm_set_core(5)
    try:
        torch.manual_seed(3)
        a = torch.randn(8192, 1024, device="cuda").to(torch.bfloat16)
        w = torch.randn(2048, 1024, device="cuda").to(torch.bfloat16)
        y = raw.gemm(a, w)
        assert _rel(y[:1024], a[:1024].float() @ w.float().t()) < 5e-3
    finally:
        ext.gemm_set_core(prev)


def test_removed_core_kinds_are_rejected():
    """Core kinds 2-4 and transform-A mode 2 named experiment-only cores that are gone:
    selecting one returns -1 and leaves the active kind alone (gemm_set_core(-1) only reads
    it), and the default dispatch still computes a ragged GEMM (partial M and N tiles, K tail)."""
    from cloud_amd.ops import _ext, raw

    ext = _ext.load(required=True)
    kind = ext.gemm_set_core(-1)
    for k in (2, 3, 4):
        assert ext.gemm_set_core(k) == -1
        assert ext.gemm_set_core(-1) == kind
    assert ext.gemm_set_xa_n256(2) == -1
    M, N, K = 300, 264, 200
    torch.manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda").to(torch.bfloat16)
    w = torch.randn(N, K, device="cuda").to(torch.bfloat16)
    assert _rel(raw.gemm(a, w), a.float() @ w.float().t()) < 5e-3
    dy = torch.randn(M, N, device="cuda").to(torch.bfloat16)
    assert _rel(raw.gemm(dy, w, layout=raw.NN), dy.float() @ w.float()) < 5e-3
