"""``cloud_amd.keras.layers.MultiHeadAttention`` on the CPU (float32 policy): the weight layout
against a hand-written einsum implementation of Keras's layer, the calling conventions, the
functional API and the arguments that are refused."""
import math

import numpy as np
import pytest
import torch

from cloud_amd import keras
from cloud_amd.keras import layers

B, T, S, DIM, H, D = 2, 7, 5, 12, 3, 4


@pytest.fixture(autouse=True)
def _float32_policy():
    from cloud_amd.keras import engine

    old = engine._POLICY
    engine.set_global_policy("float32")
    yield
    engine._POLICY = old


def _keras_weights(seed=0):
    r = np.random.RandomState(seed)
    shapes = [(DIM, H, D), (H, D), (DIM, H, D), (H, D), (DIM, H, D), (H, D), (H, D, DIM), (DIM,)]
    return [r.randn(*s).astype(np.float32) * 0.3 for s in shapes]


def _keras_mha(w, query, value, key=None, mask=None, causal=False):
    """Keras's MultiHeadAttention in its own einsum equations (float64)."""
    wq, bq, wk, bk, wv, bv, wo, bo = [torch.as_tensor(a).double() for a in w]
    key = value if key is None else key
    q = torch.einsum("abc,cde->abde", query.double(), wq) + bq  # [B, T, H, D]
    k = torch.einsum("abc,cde->abde", key.double(), wk) + bk
    v = torch.einsum("abc,cde->abde", value.double(), wv) + bv
    q = q * (1.0 / math.sqrt(D))
    sc = torch.einsum("aecd,abcd->acbe", k, q)  # [B, H, T, S]
    allowed = torch.ones(query.shape[0], query.shape[1], key.shape[1], dtype=torch.bool)
    if mask is not None:
        allowed = allowed & mask
    if causal:
        allowed = allowed & torch.ones(query.shape[1], key.shape[1], dtype=torch.bool).tril()
    sc = sc.masked_fill(~allowed[:, None], -1e9)
    p = sc.softmax(-1)
    o = torch.einsum("acbe,aecd->abcd", p, v)  # [B, T, H, D]
    return torch.einsum("abcd,cde->abe", o, wo) + bo, p


def _layer(**kw):
    layer = layers.MultiHeadAttention(H, D, **kw)
    layer._maybe_build([(None, T, DIM), (None, S, DIM)])
    layer.set_weights(_keras_weights())
    layer.eval()
    return layer


def _x(n, seed):
    return torch.randn(B, n, DIM, generator=torch.Generator().manual_seed(seed))


def _close(a, b, tol=1e-5):
    e = ((a.double() - b).norm() / b.norm()).item()
    assert e < tol, e


def test_weight_layout_self_attention():
    x = _x(T, 1)
    _close(_layer()(x, x), _keras_mha(_keras_weights(), x, x)[0])
    _close(_layer()([x, x]), _keras_mha(_keras_weights(), x, x)[0])


def test_weight_layout_causal_self_attention():
    x = _x(T, 1)
    ref = _keras_mha(_keras_weights(), x, x, causal=True)[0]
    _close(_layer()(x, x, use_causal_mask=True), ref)
    _close(_layer(use_causal_mask=True)(x, x), ref)
    _close(_layer(use_causal_mask=True)([x, x]), ref)
    assert not torch.allclose(_layer()(x, x).double(), ref, atol=1e-4)


def test_weight_layout_cross_attention_with_mask_and_scores():
    q, v, k = _x(T, 1), _x(S, 2), _x(S, 3)
    mask = torch.rand(B, T, S, generator=torch.Generator().manual_seed(4)) < 0.6
    mask[:, :, 0] = True
    ref, p = _keras_mha(_keras_weights(), q, v, k, mask=mask)
    _close(_layer()(q, v, k, attention_mask=mask), ref)
    _close(_layer()(q, v, key=k, attention_mask=mask.numpy()), ref)
    out, scores = _layer()(q, v, k, attention_mask=mask, return_attention_scores=True)
    assert scores.shape == (B, H, T, S)
    _close(out, ref)
    _close(scores, p)
    ref2, p2 = _keras_mha(_keras_weights(), q, v)
    out2, scores2 = _layer()([q, v], return_attention_scores=True)
    _close(out2, ref2)
    _close(scores2, p2)


def test_get_weights_round_trips_keras_arrays():
    w = _keras_weights(3)
    layer = _layer()
    layer.set_weights(w)
    got = layer.get_weights()
    assert len(got) == 8
    for a, b in zip(got, w):
        assert a.shape == b.shape and np.array_equal(a, b)
    nb = layers.MultiHeadAttention(H, D, use_bias=False)
    nb._maybe_build([(None, T, DIM), (None, T, DIM)])
    nb.set_weights(w[0::2])
    assert [a.shape for a in nb.get_weights()] == [b.shape for b in w[0::2]]
    with pytest.raises(ValueError):
        nb.set_weights(w)


def test_packed_parameters_follow_dense():
    layer = _layer()
    assert layer.qkv_kernel.shape == (3 * H * D, DIM) and layer.qkv_bias.shape == (3 * H * D,)
    assert layer.out_kernel.shape == (DIM, H * D) and layer.out_bias.shape == (DIM,)
    assert layer.count_params() == 4 * H * D * DIM + 3 * H * D + DIM


def _functional_model(vocab=11, seq=6):
    inp = keras.Input(shape=(seq,))
    x = layers.Embedding(vocab, DIM)(inp)
    a = layers.MultiHeadAttention(H, D, use_causal_mask=True, name="mha")([x, x])
    x = layers.Add()([x, a])
    x = layers.LayerNormalization()(x)
    out = layers.Dense(vocab)(x)
    return keras.Model(inp, out)


def test_functional_model_fits_and_is_causal():
    torch.manual_seed(0)
    vocab, seq = 11, 6
    model = _functional_model(vocab, seq)
    mha = model.get_layer("mha")
    cfg = mha.get_config()
    assert cfg["use_causal_mask"] is True and cfg["num_heads"] == H and cfg["key_dim"] == D
    clone = layers.MultiHeadAttention.from_config(cfg)
    assert clone.use_causal_mask and clone.get_config() == cfg
    assert layers.LAYERS["MultiHeadAttention"] is layers.MultiHeadAttention

    r = np.random.RandomState(0)
    x = r.randint(0, vocab, size=(8, seq)).astype(np.int64)
    y = r.randn(8, seq, vocab).astype(np.float32)
    model.compile(optimizer="adam", loss="mse")
    before = [p.detach().clone() for p in mha.parameters()]
    hist = model.fit(x, y, batch_size=8, epochs=1, verbose=0)
    assert math.isfinite(hist.history["loss"][0])
    assert any(not torch.equal(a, b) for a, b in zip(before, mha.parameters()))

    x2 = x.copy()
    x2[:, -1] = (x2[:, -1] + 1) % vocab
    p1, p2 = model.predict(x, verbose=0), model.predict(x2, verbose=0)
    assert np.array_equal(p1[:, :-1], p2[:, :-1])
    assert not np.array_equal(p1[:, -1], p2[:, -1])


def test_symbolic_keras_style_call_records_causality():
    inp = keras.Input(shape=(6,))
    x = layers.Embedding(11, DIM)(inp)
    layer = layers.MultiHeadAttention(H, D)
    out = layer(x, x, use_causal_mask=True)
    assert layer.use_causal_mask and out.shape == (None, 6, DIM) and out.inputs == (x, x)
    with pytest.raises(ValueError, match="attention_mask"):
        layers.MultiHeadAttention(H, D)(x, x, attention_mask=np.ones((6, 6), bool))


def test_exported_under_tf_keras_layers():
    from cloud_amd import tf

    assert tf.keras.layers.MultiHeadAttention is layers.MultiHeadAttention


@pytest.mark.parametrize("kw", [{"value_dim": D + 1}, {"output_shape": 8}, {"attention_axes": (1,)}])
def test_unsupported_arguments_raise(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        layers.MultiHeadAttention(H, D, **kw)


def test_value_is_required():
    with pytest.raises(ValueError, match="value"):
        layers.MultiHeadAttention(H, D)(_x(T, 1))
