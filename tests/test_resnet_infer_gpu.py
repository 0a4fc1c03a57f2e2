"""The fused inference route of the ResNet model (CLOUD_AMD_INFER_FUSE=1: every BatchNorm in
the epilogue of its convolution, ops.conv_bn_act_infer) against the per-layer route
(CLOUD_AMD_INFER_FUSE=0: convolution with statistics partials, then bn_apply) on an MI355X.

Model: resnet18_like_small (one bottleneck per stage), batch 2, 64 x 64, bf16, with random running
statistics and gamma / beta (not the initial identity).  The switch is read on every forward
(cloud_amd.config.get), so both routes run in this process.

Accuracy: both routes' eval logits are compared with the fp32 torch path (CLOUD_AMD_OPS=torch on
fp32 copies of the same weights).  With e1 / e0 the relative L2 errors of the fused / per-layer
route, the test requires e1 <= 2 e0: both routes round every activation to bf16 twice per conv + BN
and differ only in where, so they should be equal in distribution; the factor 2 is for
seed-to-seed spread.  Observed on an MI355X: e1 = 3.38e-3, e0 = 3.77e-3
(the two routes differ from each other by 5.5e-3).

Launch counts (torch.profiler): the fused eval forward of one bottleneck with projection issues 4
kernels and no bn_apply; the per-layer route issues more (observed: 32).

Frozen body: a frozen Keras ResNet50 base gives bitwise the same output in train() and eval() mode
and leaves its running statistics bit for bit alone.
"""
import pytest
import torch

DEV = "cuda"
BF16 = torch.bfloat16


def _randomize_bn(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if hasattr(m, "running_var"):
                c = m.running_var.numel()
                m.running_mean.copy_(0.3 * torch.randn(c, generator=g))
                m.running_var.copy_(0.5 + torch.rand(c, generator=g))
                m.weight.copy_(0.5 + torch.rand(c, generator=g))
                m.bias.copy_(0.2 * torch.randn(c, generator=g))


@pytest.fixture(scope="module")
def small_model():
    from cloud_amd.models.resnet import resnet18_like_small

    torch.manual_seed(0)
    model = resnet18_like_small(num_classes=16, dtype=BF16, device=DEV)
    _randomize_bn(model, 1)
    model.eval()
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(2)).to(BF16).to(DEV)
    return model, x


def _rel_l2(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return float((a - ref).norm() / ref.norm())


@pytest.mark.gpu
def test_fused_eval_logits_as_accurate_as_per_layer_route(small_model, monkeypatch):
    from cloud_amd.models.resnet import resnet18_like_small
    from cloud_amd.ops import _ext

    model, x = small_model
    with torch.no_grad():
        monkeypatch.setenv("CLOUD_AMD_INFER_FUSE", "1")
        y1 = model(x)
        monkeypatch.setenv("CLOUD_AMD_INFER_FUSE", "0")
        y0 = model(x)
        # the reference: stock torch ops (CLOUD_AMD_OPS=torch) on fp32 copies of the same weights
        ref_model = resnet18_like_small(num_classes=16, dtype=torch.float32, device=DEV)
        ref_model.load_state_dict(model.state_dict())
        ref_model.eval()
        monkeypatch.setattr(_ext, "_OPS_MODE", ["torch"])
        yr = ref_model(x.float())
    torch.cuda.synchronize()
    assert yr.dtype == torch.float32 and torch.isfinite(yr).all() and float(yr.abs().max()) > 0
    e1, e0 = _rel_l2(y1, yr), _rel_l2(y0, yr)
    print(f"[infer] eval logits vs fp32 torch: fused e1 {e1:.3e}, per-layer e0 {e0:.3e}, "
          f"fused vs per-layer {_rel_l2(y1, y0):.3e}", flush=True)
    assert e1 <= 2 * e0, (e1, e0)


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile

    fn()  # warm: folded() coefficients cached, modules loaded
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    return [n for n in names if "memcpy" not in n.lower() and "memset" not in n.lower()]


@pytest.mark.gpu
def test_fused_projection_block_is_four_kernels(small_model, monkeypatch):
    model, _ = small_model
    blk = model.layers[1]  # stage 2: strided 3x3 and a strided projection shortcut
    assert blk.downsample is not None and not blk.training
    x = torch.randn(2, 16, 16, 256, generator=torch.Generator().manual_seed(3)).to(BF16).to(DEV)

    def run():
        with torch.no_grad():
            return blk(x)

    monkeypatch.setenv("CLOUD_AMD_INFER_FUSE", "1")
    fused = _kernel_names(run)
    monkeypatch.setenv("CLOUD_AMD_INFER_FUSE", "0")
    plain = _kernel_names(run)
    print(f"[infer] projection block: fused {len(fused)} kernels {fused}; per-layer route {len(plain)}", flush=True)
    assert len(fused) == 4, fused
    assert not any("bn_apply" in n for n in fused)
    assert len(plain) > 4 and any("bn_apply" in n for n in plain), plain


@pytest.mark.gpu
def test_frozen_keras_base_is_bitwise_inference(monkeypatch):
    from cloud_amd import tf
    from cloud_amd.keras import engine

    monkeypatch.setattr(engine, "_POLICY", engine.Policy("mixed_bfloat16"))
    torch.manual_seed(4)
    base = tf.keras.applications.ResNet50(include_top=False, weights=None, input_shape=(64, 64, 3))
    _randomize_bn(base, 5)
    base.to(DEV)
    base.trainable = False
    x = torch.randn(2, 64, 64, 3, generator=torch.Generator().manual_seed(6)).to(DEV)
    stats = {k: v.clone() for k, v in base.state_dict().items() if "running_" in k}
    assert len(stats) == 2 * 53
    base.train()
    assert not base.body.net.training
    y_train = base(x)
    base.eval()
    y_eval = base(x)
    torch.cuda.synchronize()
    assert not y_train.requires_grad and y_train.shape == (2, 2, 2, 2048)
    assert torch.isfinite(y_train).all() and float(y_train.abs().max()) > 0
    assert torch.equal(y_train, y_eval)
    now = base.state_dict()
    for k, v in stats.items():
        assert torch.equal(v, now[k]), f"{k} of a frozen base moved"
