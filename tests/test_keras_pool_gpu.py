"""Keras pooling layers under ``mixed_bfloat16`` on the GPU: a two-branch functional model
(``Conv2D -> MaxPooling2D((2, 3), "same")`` and ``Conv2D -> AveragePooling2D(3, 2, "same")``,
concatenated, ``GlobalAveragePooling2D -> Dense``) against the same model on the PyTorch route in
float32, one ``fit`` step of it, and the bag-of-embeddings text model of
examples/workloads/text_avgpool.py on the native global average pool.

The comparison uses the row metric of test_depthwise_conv_gpu.py (per row over the last axis,
``||got - ref|| / max(||ref||, median row ||ref||)``) with the project's bf16 bound 1e-2.  The
convolution kernels and the input hold small integers, so both models' convolution outputs are
exact and the max pool routes its gradient to the same pixels in both: what is compared is the
arithmetic, not which of two values a bf16 rounding apart counts as the larger.

Observed on an MI355X: outputs 2.92e-3 per row, input gradients 7.99e-3 per row (rows of three
channels behind five bf16 roundings: Dense, global pool, the two pools, the convolutions' sum);
the text model's loss 1.3859 -> 0.9966 in 20 steps.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROW_BOUND = 1e-2


def _say(*a):
    print("[keras-pool]", *a, flush=True)


def _row_err(got, ref):
    C = ref.shape[-1]
    g, r = got.detach().double().cpu().reshape(-1, C), ref.detach().double().cpu().reshape(-1, C)
    assert g.shape == r.shape and torch.isfinite(g).all()
    n = r.norm(dim=-1)
    return ((g - r).norm(dim=-1) / torch.maximum(n, n.median())).max().item()


def _two_branch_model():
    from cloud_amd import keras

    L = keras.layers
    inp = keras.Input(shape=(12, 12, 3))
    a = L.MaxPooling2D((2, 3), padding="same")(L.Conv2D(8, 3)(inp))        # 10x10 -> 5x4 (W pads 1 | 1)
    b = L.AveragePooling2D(3, 2, "same")(L.Conv2D(8, 3)(inp))              # 10x10 -> 5x5 (pads 0 | 1)
    x = L.Concatenate(axis=2)([a, b])                                      # along W: 5x9x8
    out = L.Dense(10)(L.GlobalAveragePooling2D()(x))
    return keras.Model(inp, out)


def test_two_branch_pool_model_vs_float32_torch_route(monkeypatch):
    from cloud_amd import keras
    from cloud_amd.keras import engine
    from cloud_amd.ops import _ext, raw

    g = torch.Generator().manual_seed(0)
    x = torch.randint(-2, 3, (4, 12, 12, 3), generator=g).float()
    dy = torch.randn(4, 10, generator=g)
    native = {}
    for name in ("pool2d_max_fwd", "pool2d_max_bwd", "pool2d_avg_fwd", "pool2d_avg_bwd"):
        def f(*a, _orig=getattr(raw, name), _name=name, **k):
            native[_name] = native.get(_name, 0) + 1
            return _orig(*a, **k)

        monkeypatch.setattr(raw, name, f)
    old = engine._POLICY
    try:
        engine.set_global_policy("mixed_bfloat16")
        torch.manual_seed(0)
        model = _two_branch_model()
        model.predict(x.numpy(), batch_size=4, verbose=0)  # builds the layers
        convs = [l for l in model.layers if type(l).__name__ == "Conv2D"]
        assert len(convs) == 2
        with torch.no_grad():
            for conv in convs:  # kernels in {-1, 0, 1}: 27-term integer sums, exact in bf16 and in float32
                conv.kernel.copy_(torch.randint(-1, 2, conv.kernel.shape, generator=g).to(conv.kernel.dtype))
        weights = model.get_weights()
        native.clear()
        xd = x.to(DEV).requires_grad_()
        y = model(xd)
        y.backward(dy.to(DEV).to(y.dtype))
        torch.cuda.synchronize()
        assert native == {"pool2d_max_fwd": 1, "pool2d_max_bwd": 1, "pool2d_avg_fwd": 1, "pool2d_avg_bwd": 1}, native

        engine.set_global_policy("float32")
        monkeypatch.setattr(_ext, "_OPS_MODE", ["torch"])
        ref = _two_branch_model().to(DEV)  # a functional model builds its layers on the host
        xr = x.to(DEV).requires_grad_()
        with torch.no_grad():
            ref(xr)
            ref.set_weights(weights)
        yr = ref(xr)
        assert yr.dtype == torch.float32
        yr.backward(dy.to(DEV))
        torch.cuda.synchronize()
        monkeypatch.setattr(_ext, "_OPS_MODE", ["native"])

        e_y, e_dx = _row_err(y, yr), _row_err(xd.grad, xr.grad)
        _say(f"two-branch model vs float32 torch route: y/row {e_y:.3e} dx/row {e_dx:.3e}")

        engine.set_global_policy("mixed_bfloat16")
        model.compile(optimizer="adam", loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
        labels = torch.randint(0, 10, (4,), generator=g).numpy()
        hist = model.fit(x.numpy(), labels, batch_size=4, epochs=1, verbose=0)
        torch.cuda.synchronize()
        assert np.isfinite(hist.history["loss"][0])
    finally:
        engine._POLICY = old
    assert e_y < ROW_BOUND and e_dx < ROW_BOUND, (e_y, e_dx)


def test_text_model_trains_on_the_native_global_pool(monkeypatch):
    """Embedding -> GlobalAveragePooling1D -> Dense -> Dense (the example's model) under
    mixed_bfloat16: every step pools on the gap kernels through the [B, 1, T, C] view, and 20
    steps lower the loss."""
    from cloud_amd import keras
    from cloud_amd.keras import engine
    from cloud_amd.ops import _ext

    ext = _ext.load(required=True)
    ran = {}
    for name in ("gap_fwd", "gap_bwd"):
        def f(*a, _orig=getattr(ext, name), _name=name, **k):
            ran[_name] = ran.get(_name, 0) + 1
            return _orig(*a, **k)

        monkeypatch.setattr(ext, name, f)
    vocab, seq, classes, batch, steps = 120, 16, 4, 16, 20
    r = np.random.RandomState(0)
    labels = r.randint(0, classes, size=batch * steps)
    own = labels[:, None] * (vocab // classes) + r.randint(0, vocab // classes, size=(batch * steps, seq))
    tokens = np.where(r.rand(batch * steps, seq) < 0.5, own, r.randint(0, vocab, size=(batch * steps, seq)))
    old = engine._POLICY
    try:
        engine.set_global_policy("mixed_bfloat16")
        torch.manual_seed(0)
        L = keras.layers
        model = keras.Sequential([L.Embedding(vocab, 16, input_shape=(seq,)), L.GlobalAveragePooling1D(),
                                  L.Dense(16, activation="relu"), L.Dense(classes)])
        model.compile(optimizer=keras.optimizers.Adam(1e-2),
                      loss=keras.losses.SparseCategoricalCrossentropy(from_logits=True))
        before = float(model.evaluate(tokens, labels, batch_size=batch * steps, verbose=0))
        ran.clear()
        hist = model.fit(tokens, labels, batch_size=batch, epochs=1, verbose=0, shuffle=False)
        torch.cuda.synchronize()
        assert ran == {"gap_fwd": steps, "gap_bwd": steps}, ran
        after = float(model.evaluate(tokens, labels, batch_size=batch * steps, verbose=0))
    finally:
        engine._POLICY = old
    _say(f"text model: loss {before:.4f} -> {after:.4f} after {steps} steps (fit mean {hist.history['loss'][0]:.4f})")
    assert np.isfinite(after) and after < before, (before, after)
