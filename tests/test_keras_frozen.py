"""Keras semantics of ``trainable = False`` (CPU): a frozen layer runs in inference mode, in
``fit`` too.  A frozen ``BatchNormalization`` normalises with its moving statistics and leaves them
alone; a frozen ``ResNet50`` base keeps every parameter and buffer bit for bit while the head
trains; ``ResNet50(weights=<path>)`` loads a ``save_weights`` file."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cloud_amd import tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = tf.keras.layers


@pytest.fixture(autouse=True)
def _cpu_float32():
    """These are CPU tests wherever they run: one CPU device, float32 policy."""
    from cloud_amd.keras import engine
    from cloud_amd.parallel import strategy as S

    old = engine._POLICY
    engine.set_global_policy("float32")
    S.experimental_set_strategy(S.OneDeviceStrategy("/cpu:0"))
    yield
    S.experimental_set_strategy(None)
    engine._POLICY = old


def _snapshot(module):
    return {k: v.detach().clone() for k, v in module.state_dict().items()}


def _small_bn_model():
    torch.manual_seed(0)
    model = tf.keras.Sequential([
        L.Conv2D(8, 3, padding="same", input_shape=(8, 8, 3)),
        L.BatchNormalization(),
        L.Flatten(),
        L.Dense(4),
    ])
    model.compile(optimizer=tf.keras.optimizers.SGD(learning_rate=0.05),
                  loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((24, 8, 8, 3)) * 2 + 1).astype(np.float32)
    y = rng.integers(0, 4, 24)
    model.predict(x[:2], verbose=0)  # builds the weights
    bn = model.layers[1]
    with torch.no_grad():  # non-trivial moving statistics and affine
        bn.moving_mean.copy_(torch.linspace(-0.5, 0.5, 8))
        bn.moving_variance.copy_(torch.linspace(0.5, 2.0, 8))
        bn.gamma.copy_(torch.linspace(0.7, 1.3, 8))
        bn.beta.copy_(torch.linspace(-0.2, 0.2, 8))
    return model, bn, x, y


def test_frozen_batchnorm_runs_in_inference_mode_during_fit():
    model, bn, x, y = _small_bn_model()
    bn.trainable = False
    before = _snapshot(bn)
    dense_before = model.layers[3].kernel.detach().clone()
    model.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False)  # 3 steps
    after = _snapshot(bn)
    for k in ("moving_mean", "moving_variance", "gamma", "beta"):
        assert torch.equal(before[k], after[k]), f"{k} of a frozen BatchNormalization moved"
    assert not torch.equal(dense_before, model.layers[3].kernel.detach()), "the Dense kernel did not train"
    model.train()
    assert not bn.training, "train() must leave a frozen BatchNormalization in inference mode"
    assert model.layers[3].training
    h = torch.as_tensor(x[:8]) @ torch.ones(3, 8)  # any [8, 8, 8, 8] activation
    with torch.no_grad():
        assert torch.equal(bn(h, training=True), bn(h, training=False))
    assert torch.equal(before["moving_mean"], bn.moving_mean)


def test_unfreezing_restores_batch_statistics():
    model, bn, x, y = _small_bn_model()
    bn.trainable = False
    model.train()
    assert not bn.training
    bn.trainable = True
    model.train()
    assert bn.training and bn.gamma.requires_grad
    h = torch.as_tensor(x[:8]) @ torch.ones(3, 8)
    mean0 = bn.moving_mean.clone()
    with torch.no_grad():
        out_train, out_infer = bn(h, training=True), bn(h, training=False)
    assert not torch.equal(out_train, out_infer), "a trainable BatchNormalization uses batch statistics"
    assert not torch.equal(mean0, bn.moving_mean), "and updates its moving mean"
    gamma0 = bn.gamma.detach().clone()
    model.fit(x, y, batch_size=8, epochs=1, verbose=0, shuffle=False)
    assert not torch.equal(gamma0, bn.gamma.detach())


def test_trainable_reaches_nested_layers():
    inner = tf.keras.Sequential([L.Dense(4, input_shape=(3,)), L.BatchNormalization()])
    outer = tf.keras.Sequential([inner, L.Dense(2)])
    outer.predict(np.zeros((2, 3), np.float32), verbose=0)
    inner.trainable = False
    assert all(not layer.trainable for layer in inner.layers)
    assert outer.layers[1].trainable and len(outer.trainable_weights) == 2
    outer.train()
    assert not inner.layers[1].training and outer.layers[1].training


def _frozen_resnet_model(weights=None):
    torch.manual_seed(1)
    base = tf.keras.applications.ResNet50(include_top=False, weights=weights, input_shape=(32, 32, 3))
    return base


def test_frozen_resnet50_base_end_to_end():
    base = _frozen_resnet_model()
    with torch.no_grad():  # running statistics away from their initial identity
        for m in base.body.net.modules():
            if hasattr(m, "running_var"):
                m.running_mean.normal_(0.0, 0.1)
                m.running_var.uniform_(0.8, 1.2)
    base.trainable = False
    model = tf.keras.Sequential([base, L.GlobalAveragePooling2D(), L.Dense(5)])
    model.compile(optimizer=tf.keras.optimizers.SGD(learning_rate=0.1),
                  loss=tf.keras.losses.SparseCategoricalCrossentropy(from_logits=True))
    rng = np.random.default_rng(1)
    x = rng.standard_normal((8, 32, 32, 3)).astype(np.float32)
    y = rng.integers(0, 5, 8)
    model.predict(x[:2], verbose=0)
    before = _snapshot(base)
    head = model.layers[2]
    k0, b0 = head.kernel.detach().clone(), head.bias.detach().clone()
    assert len(model.trainable_weights) == 2
    model.fit(x, y, batch_size=4, epochs=2, verbose=0)
    after = _snapshot(base)
    assert before.keys() == after.keys() and len(before) == 267  # 53 convs, 53 x 4 BN tensors, fc
    for k in before:
        assert torch.equal(before[k], after[k]), f"frozen base tensor {k} changed"
    assert not torch.equal(k0, head.kernel.detach()) and not torch.equal(b0, head.bias.detach())
    assert len(model.trainable_weights) == 2
    model.train()
    assert not base.body.net.training and not any(m.training for m in base.body.net.modules())
    lines = []
    model.summary(print_fn=lines.append)
    non_trainable = [ln for ln in lines if ln.startswith("Non-trainable params")][0]
    assert int(non_trainable.split(":")[1].replace(",", "")) == base.count_params()
    # the frozen base builds no autograd graph: its output is a leaf for the head
    out = base(torch.as_tensor(x[:2]))
    assert not out.requires_grad and out.grad_fn is None


def test_resnet50_weights_path_round_trip(tmp_path):
    src = _frozen_resnet_model()
    with torch.no_grad():
        for p in src.parameters():
            p.add_(0.01)
    path = str(tmp_path / "base.weights")
    src.save_weights(path)
    dst = tf.keras.applications.ResNet50(include_top=False, weights=path, input_shape=(32, 32, 3))
    a, b = src.state_dict(), dst.state_dict()
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    with pytest.raises(ValueError):
        tf.keras.applications.ResNet50(include_top=False, weights="imagenet", input_shape=(32, 32, 3))
    with pytest.raises(ValueError):
        tf.keras.applications.ResNet50(include_top=False, weights=str(tmp_path / "missing"), input_shape=(32, 32, 3))


def test_folded_batchnorm_cache_follows_its_tensors():
    from cloud_amd.models.layers import BatchNormAct

    bn = BatchNormAct(8, relu=False)
    bn.eval()
    a = bn.folded()
    assert bn.folded() is a, "steady state: the cached tensor"
    assert torch.allclose(a[:8], torch.full((8,), (1 + bn.eps) ** -0.5)) and torch.equal(a[8:], torch.zeros(8))
    with torch.no_grad():
        bn.running_mean.fill_(2.0)  # in-place write: version bump
    b = bn.folded()
    assert b is not a and torch.allclose(b[8:], -2.0 * b[:8])
    bn.weight.data = torch.full((8,), 3.0)  # replaced storage: data_ptr change
    c = bn.folded()
    assert c is not b and torch.allclose(c[:8], 3.0 * b[:8])
    bn.train()
    bn.eval()
    assert bn.folded() is not c, "entering training mode drops the cache"


def test_transfer_example_runs():
    env = dict(os.environ, CLOUD_AMD_DEVICE="cpu", CLOUD_AMD_PRECISION="float32")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "workloads", "resnet50_transfer.py")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "RESULT resnet50_transfer trainable_weights=2" in r.stdout
    assert "Non-trainable params: 25,5" in r.stdout
