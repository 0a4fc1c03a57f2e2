"""``ops.layer_norm`` and ``keras.layers.LayerNormalization`` without a GPU: the reference path
is ``F.layer_norm`` bit for bit (fp32 and bf16, with and without a residual, 2-D and 4-D), its
gradients pass ``gradcheck`` in fp64, ``gamma=None`` / ``beta=None`` mean ones / zeros, wrong
shapes raise before anything runs, and the Keras layer keeps its float32 outputs while gaining
``center`` / ``scale``."""
import pytest
import torch
import torch.nn.functional as F

from cloud_amd import ops


def _inputs(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = shape[-1]
    x = torch.randn(*shape, generator=g).to(dtype)
    r = torch.randn(*shape, generator=g).to(dtype)
    gamma = 1.0 + 0.3 * torch.randn(C, generator=g)
    beta = 0.2 * torch.randn(C, generator=g)
    return x, r, gamma, beta


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("shape", [(7, 33), (2, 3, 5, 12)])
def test_cpu_path_is_f_layer_norm_bitwise(dtype, with_res, shape):
    x, r, gamma, beta = _inputs(shape, dtype)
    y = ops.layer_norm(x, gamma, beta, eps=1e-3, residual=r if with_res else None)
    h = x + r if with_res else x
    want = F.layer_norm(h.float(), (shape[-1],), gamma, beta, 1e-3).to(dtype)
    assert y.dtype == dtype and y.shape == x.shape
    assert torch.equal(y, want)


def test_default_eps_is_keras():
    x, _, gamma, beta = _inputs((4, 9), torch.float32)
    assert torch.equal(ops.layer_norm(x, gamma, beta), F.layer_norm(x, (9,), gamma, beta, 1e-3))


def test_gradcheck_fp64():
    x, r, gamma, beta = (t.double().requires_grad_() for t in _inputs((3, 2, 6), torch.float64, seed=1))
    assert torch.autograd.gradcheck(lambda a, b, c, d: ops.layer_norm(a, c, d, 1e-3, residual=b), (x, r, gamma, beta))
    assert torch.autograd.gradcheck(lambda a, c, d: ops.layer_norm(a, c, d, 1e-3), (x, gamma, beta))
    y = ops.layer_norm(x, gamma, beta, 1e-3, residual=r)
    assert y.dtype == torch.float64
    assert torch.equal(y, F.layer_norm(x + r, (6,), gamma, beta, 1e-3))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_none_gamma_beta_are_ones_zeros(dtype):
    x, _, gamma, beta = _inputs((5, 10), dtype)
    ones, zeros = torch.ones(10), torch.zeros(10)
    # the reference hands a None on to F.layer_norm, whose kernel without a scale or an offset
    # rounds differently in the last fp32 bit (|y| < 8: 1e-6), which can move a bf16 result by
    # one bf16 step (2^-6 below 4, 2^-5 below 8)
    tol = dict(rtol=0, atol=1e-6 if dtype == torch.float32 else 2.0 ** -5)

    def same(a, b):
        return a.dtype == b.dtype and torch.allclose(a.float(), b.float(), **tol)

    assert same(ops.layer_norm(x), ops.layer_norm(x, ones, zeros))
    assert same(ops.layer_norm(x, gamma, None), ops.layer_norm(x, gamma, zeros))
    assert same(ops.layer_norm(x, None, beta), ops.layer_norm(x, ones, beta))
    assert torch.equal(ops.layer_norm(x, None, beta), F.layer_norm(x.float(), (10,), None, beta, 1e-3).to(dtype))
    xg = x.float().requires_grad_()
    ops.layer_norm(xg).square().sum().backward()
    assert xg.grad is not None and torch.isfinite(xg.grad).all()


def test_shape_and_dtype_errors():
    x, r, gamma, beta = _inputs((4, 8), torch.float32)
    with pytest.raises(ValueError, match="gamma"):
        ops.layer_norm(x, gamma[:7], beta)
    with pytest.raises(ValueError, match="gamma"):
        ops.layer_norm(x, gamma.view(1, 8), beta)
    with pytest.raises(ValueError, match="beta"):
        ops.layer_norm(x, gamma, torch.zeros(9))
    with pytest.raises(ValueError, match="residual"):
        ops.layer_norm(x, gamma, beta, residual=r[:3])
    with pytest.raises(ValueError, match="residual"):
        ops.layer_norm(x, gamma, beta, residual=r.to(torch.bfloat16))
    with pytest.raises(ValueError, match="residual"):
        ops.layer_norm(x.view(2, 2, 8), gamma, beta, residual=r)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_empty_tensor(dtype):
    x = torch.empty(0, 8, dtype=dtype)
    y = ops.layer_norm(x, torch.ones(8), torch.zeros(8), residual=torch.empty(0, 8, dtype=dtype))
    assert y.shape == (0, 8) and y.dtype == dtype
    assert ops.layer_norm(torch.empty(3, 0, 8, dtype=dtype)).shape == (3, 0, 8)


def test_keras_center_scale_and_config():
    from cloud_amd.keras import layers

    bare = layers.LayerNormalization(center=False, scale=False, epsilon=1e-5)
    x, _, _, _ = _inputs((2, 5, 16), torch.float32)
    y = bare(x)
    assert list(bare.parameters()) == [] and bare.get_weights() == []
    assert torch.equal(y, F.layer_norm(x, (16,), None, None, 1e-5))
    cfg = bare.get_config()
    assert cfg["center"] is False and cfg["scale"] is False and cfg["epsilon"] == 1e-5
    again = layers.LayerNormalization.from_config(cfg)
    assert again.get_config() == cfg and (again.center, again.scale) == (False, False)

    full = layers.LayerNormalization()
    full(x)
    assert [tuple(p.shape) for p in full.parameters()] == [(16,), (16,)]
    cfg = full.get_config()
    assert cfg["center"] is True and cfg["scale"] is True
    assert layers.LayerNormalization.from_config(cfg).get_config() == cfg

    for kw, names in (({"center": False}, ["gamma"]), ({"scale": False}, ["beta"])):
        one = layers.LayerNormalization(**kw)
        one(x)
        assert [n for n, _ in one.named_parameters()] == names


def test_keras_float32_output_is_the_old_expression():
    from cloud_amd.keras import layers

    layer = layers.LayerNormalization(epsilon=1e-3, dtype="float32")
    x, _, gamma, beta = _inputs((3, 4, 24), torch.float32, seed=2)
    layer(x)
    with torch.no_grad():
        layer.gamma.copy_(gamma)
        layer.beta.copy_(beta)
    for t in (x, x.to(torch.bfloat16)):
        y = layer(t)
        old = F.layer_norm(t.float(), (t.shape[-1],), layer.gamma, layer.beta, layer.epsilon).to(t.dtype)
        assert y.dtype == t.dtype and torch.equal(y, old)
    xg = x.clone().requires_grad_()
    layer(xg).square().sum().backward()
    assert xg.grad is not None and layer.gamma.grad is not None and layer.beta.grad is not None
