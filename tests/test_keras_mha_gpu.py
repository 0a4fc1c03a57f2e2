"""``keras.layers.MultiHeadAttention`` under ``mixed_bfloat16`` on the GPU: with key_dim = 64 the
self-attention path is the packed projection, ``ops.attention`` and the output projection, all
on in-tree kernels.  It is held to the same layer's float32 PyTorch path with the bounds of the
BERT native-vs-torch tests (relative norm 3e-2 for outputs, 8e-2 for parameter gradients), and
a training step of it may not reach a library GEMM."""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, S, H, D = 2, 100, 2, 64
DIM = H * D


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _pair(causal):
    """The same weights as a mixed_bfloat16 and as a float32 layer."""
    from cloud_amd.keras import layers

    torch.manual_seed(3)
    mixed = layers.MultiHeadAttention(H, D, use_causal_mask=causal, dtype="mixed_bfloat16")
    ref = layers.MultiHeadAttention(H, D, use_causal_mask=causal, dtype="float32")
    for layer in (mixed, ref):
        layer._maybe_build([(None, S, DIM), (None, S, DIM)], torch.device(DEV))
    w = mixed.get_weights()
    w[1::2] = [torch.randn(*a.shape).mul_(0.1).numpy() for a in w[1::2]]  # non-zero biases
    mixed.set_weights(w)
    ref.set_weights(mixed.get_weights())  # the bf16-rounded kernels
    assert mixed.qkv_kernel.dtype == torch.bfloat16 and mixed.qkv_bias.dtype == torch.float32
    assert ref.qkv_kernel.dtype == torch.float32 and mixed.qkv_kernel.is_cuda
    return mixed, ref


@pytest.mark.parametrize("causal", [False, True])
def test_mha_mixed_matches_float32_path(causal):
    mixed, ref = _pair(causal)
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, S, DIM, generator=g).to(DEV)
    dy = torch.randn(B, S, DIM, generator=g).to(DEV)
    y = mixed(x, x, training=True)
    assert y.dtype == torch.bfloat16 and y.shape == (B, S, DIM)
    (y.float() * dy).sum().backward()
    xr = x.to(torch.bfloat16).float()  # what the mixed layer's projection reads
    y_r = ref(xr, xr, training=True)
    (y_r * dy).sum().backward()
    torch.cuda.synchronize()
    e = rel(y, y_r)
    print(f"[mha] causal={causal}: out {e:.3e}", flush=True)
    worst = {}
    for (n, p), (_, p_r) in zip(mixed.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, n
        worst[n] = rel(p.grad, p_r.grad)
    print(f"[mha] causal={causal}: grads {worst}", flush=True)
    assert e < 3e-2, e
    assert all(v < 8e-2 for v in worst.values()), worst
    if causal:  # the flag reached the kernels: the non-causal layer computes something else
        other, _ = _pair(False)
        assert rel(other(x, x, training=True), y_r) > 0.1


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


@pytest.mark.parametrize("causal", [False, True])
def test_mha_training_step_uses_no_library_gemm(monkeypatch, causal):
    from cloud_amd.keras import layers

    torch.manual_seed(0)
    layer = layers.MultiHeadAttention(H, D, dropout=0.1, use_causal_mask=causal, dtype="mixed_bfloat16")
    x = torch.randn(B, S, DIM, device=DEV)
    layer._maybe_build([(None, S, DIM), (None, S, DIM)], torch.device(DEV))
    opt = torch.optim.SGD(layer.parameters(), lr=1e-3)
    layer.train()
    with counted(monkeypatch) as calls:
        opt.zero_grad()
        loss = layer([x, x], training=True).float().square().mean()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
    assert not calls, calls
    assert math.isfinite(float(loss.detach()))
    assert all(p.grad is not None and torch.isfinite(p.grad.float()).all() for p in layer.parameters())
