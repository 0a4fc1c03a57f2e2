"""BatchNorm folded into the consuming 1x1 convolution (csrc/include/ca_gemm_xa.h).

* Kernel level: ``raw.conv1x1_dgrad_bnbwd`` against a plain PyTorch fp32 reference of the
  same op -- dz = A*(dy*relu') + B*z + D, dx = dz W -- for the plain, BN-statistics and
  residual-gated epilogues, including M and channel counts that are not tile multiples.
* Model level: a ResNet trained a few steps with the folds on against off (the separate BN
  passes): the fused kernels use the BN kernels' arithmetic and the GEMM's accumulation
  order, so every conv weight gradient of the first step is BITWISE equal.
"""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _mask_bits(m):
    """[M, C] bool -> [M, C/8] uint8 bitmask (bit j = channel 8c+j)."""
    M, C = m.shape
    w = (1 << torch.arange(8, device=m.device, dtype=torch.int32))
    return (m.view(M, C // 8, 8).int() * w).sum(-1).to(torch.uint8)


@pytest.mark.parametrize("M,Cout,Cin", [(4096, 256, 64), (1000, 128, 64), (777, 64, 256), (2048, 512, 128),
                                        (300, 72, 40),
                                        # N a multiple of 256: the 128 x 256 16-wave tiles (ResNet stages 3-4)
                                        (3000, 1024, 256), (777, 2048, 512)])
@pytest.mark.parametrize("epi", ["plain", "bn", "res"])
def test_dgrad_bnbwd_vs_fp32(M, Cout, Cin, epi):
    from cloud_amd.ops import raw

    torch.manual_seed(M + Cout)
    dy = torch.randn(M, Cout, device=DEV).to(torch.bfloat16)
    z = torch.randn(M, Cout, device=DEV).to(torch.bfloat16)
    act = torch.rand(M, Cout, device=DEV) > 0.4
    mask = _mask_bits(act)
    coef = torch.randn(3 * Cout, device=DEV) * torch.tensor([1.0, 0.1, 0.01], device=DEV).repeat_interleave(Cout)
    w = (torch.randn(Cout, 1, 1, Cin, device=DEV) * 0.05).to(torch.bfloat16)
    A, B, D = coef[:Cout], coef[Cout:2 * Cout], coef[2 * Cout:]
    g = dy.float() * act.float()
    dz_ref = A * g + B * z.float() + D
    dx_ref = dz_ref.to(torch.bfloat16).float() @ w.view(Cout, Cin).float()
    side = torch.empty(1, 1, M, Cout, device=DEV, dtype=torch.bfloat16)
    shp = lambda t: t.view(1, 1, M, -1)  # noqa: E731  (NHWC view of the row-major matrix)
    kw = {}
    zb = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    act_b = torch.rand(M, Cin, device=DEV) > 0.5
    src = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    act_r = torch.rand(M, Cin, device=DEV) > 0.5
    if epi == "bn":
        kw["bn"] = (shp(zb), _mask_bits(act_b))
    if epi == "res":
        kw.update(res=(shp(src), _mask_bits(act_r)), beta=1.0, out=torch.empty(1, 1, M, Cin, device=DEV,
                                                                                dtype=torch.bfloat16))
    r = raw.conv1x1_dgrad_bnbwd(shp(dy), shp(z), mask, coef, w, side, **kw)
    dx = r[0] if isinstance(r, tuple) else r
    assert rel(side.view(M, Cout), dz_ref) < 1e-2
    want = dx_ref + (src.float() * act_r.float() if epi == "res" else 0.0)
    assert rel(dx.view(M, Cin), want) < 2e-2, rel(dx.view(M, Cin), want)
    if epi == "bn":
        part = r[1]
        gd = dx.view(M, Cin).float() * act_b.float()
        s = part[:, 0].sum(0)
        q = part[:, 1].sum(0)
        assert rel(s, gd.sum(0)) < 1e-3 and rel(q, (gd * zb.float()).sum(0)) < 1e-3


DW_CASES = [(4096, 256, 64, "bn"), (1000, 128, 64, "bn"), (777, 64, 64, "plain"), (70000, 256, 64, "bn"),
            (4096, 256, 64, "plain"), (3000, 64, 256, "res2"), (1000, 64, 256, "res"), (777, 64, 256, "bn"),
            (300, 64, 64, "res"), (5000, 64, 256, "plain"), (5000, 512, 128, "bn"), (777, 512, 128, "plain"),
            (100000, 512, 128, "bn"), (777, 256, 64, "bn"), (777, 256, 64, "plain0"), (70000, 256, 64, "plain0")]
# K 256 -> N 64 with beta 0 ("bn", "plain0": a fresh output, the projection shortcut's form) runs
# the deep-stream kernel (mfma_gemm_xa_dw_deep); the other epilogues the one-step form


@pytest.mark.parametrize("M,Cout,Cin,epi", DW_CASES)
@pytest.mark.parametrize("blocks", [None, 3])
@pytest.mark.parametrize("dw_dtype", [torch.bfloat16, torch.float32])
def test_dgrad_wgrad_bnbwd_vs_fp32(M, Cout, Cin, epi, blocks, dw_dtype):
    """Input AND weight gradient of the BN-folded 1x1 conv in one pass (mfma_gemm_xa_dw):
    dz = A*(dy*relu') + B*z + D is never written; dx = dz W (+ beta * old / residual-gated
    source) with the BN-statistics epilogues, dw = dz^T y + dw_old -- each against a plain fp32
    PyTorch reference.  conv3 shapes (Cin 64, K chunks) and conv1 shapes (Cout 64, N chunks)."""
    from cloud_amd.ops import raw

    torch.manual_seed(M + Cout + Cin)
    dy = torch.randn(M, Cout, device=DEV).to(torch.bfloat16)
    z = torch.randn(M, Cout, device=DEV).to(torch.bfloat16)
    act = torch.rand(M, Cout, device=DEV) > 0.4
    coef = torch.randn(3 * Cout, device=DEV) * torch.tensor([1.0, 0.1, 0.01], device=DEV).repeat_interleave(Cout)
    w = (torch.randn(Cout, 1, 1, Cin, device=DEV) * 0.05).to(torch.bfloat16)
    y = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    zb = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    z2 = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    act_b = torch.rand(M, Cin, device=DEV) > 0.5
    src = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    act_r = torch.rand(M, Cin, device=DEV) > 0.5
    old = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    dw0 = (torch.randn(Cout, 1, 1, Cin, device=DEV) * 0.1).to(dw_dtype)
    dw = dw0.clone()
    A, B, D = coef[:Cout], coef[Cout:2 * Cout], coef[2 * Cout:]
    dz = (A * dy.float() * act.float() + B * z.float() + D).to(torch.bfloat16).float()
    shp = lambda t: t.view(1, 1, M, -1)  # noqa: E731
    kw = {}
    want = dz @ w.view(Cout, Cin).float()
    if epi in ("bn", "res", "res2"):
        kw["bn"] = (shp(zb), _mask_bits(act_b)) + ((shp(z2),) if epi == "res2" else ())
    if epi in ("res", "res2"):
        kw.update(res=(shp(src), _mask_bits(act_r)), beta=1.0)
        want = want + src.float() * act_r.float()
    if epi == "plain":  # beta accumulate into an existing dx
        kw.update(out=shp(old.clone()), beta=1.0)
        want = want + old.float()
    r = raw.conv1x1_dgrad_wgrad_bnbwd(shp(dy), shp(z), _mask_bits(act), coef, w, shp(y), dw, dw_beta=1.0,
                                      blocks=blocks, **kw)
    dx = r[0] if isinstance(r, tuple) else r
    assert rel(dx.view(M, Cin), want) < 2e-2, rel(dx.view(M, Cin), want)
    dw_ref = dz.t() @ y.float() + dw0.view(Cout, Cin).float()
    assert rel(dw.view(Cout, Cin), dw_ref) < 1e-2, rel(dw.view(Cout, Cin), dw_ref)
    if "bn" in kw:
        gd = dx.view(M, Cin).float() * act_b.float()
        part = r[1]
        assert rel(part[:, 0].sum(0), gd.sum(0)) < 1e-3 and rel(part[:, 1].sum(0), (gd * zb.float()).sum(0)) < 1e-3
        if epi == "res2":
            p2 = r[2]
            assert rel(p2[:, 0].sum(0), gd.sum(0)) < 1e-3 and rel(p2[:, 1].sum(0), (gd * z2.float()).sum(0)) < 1e-3


@pytest.mark.parametrize("M,Cin,Cout", [(4096, 256, 64), (1000, 512, 128), (777, 64, 256), (300, 40, 72),
                                        (3000, 1024, 256), (777, 2048, 512)])
@pytest.mark.parametrize("mode", ["bn", "res", "resbn"])
def test_fwd_bnapply_vs_fp32(M, Cin, Cout, mode):
    """Forward prologue: y = relu(z*scale + shift [+ r | + bf16(r*rscale + rshift)]) applied in
    the GEMM's operand fetch, written once (side + ReLU bitmask), out = y W^T with the BN
    statistics epilogue -- against a plain fp32 PyTorch reference of the same op."""
    from cloud_amd.ops import raw

    torch.manual_seed(M + Cin)
    z = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    r = torch.randn(M, Cin, device=DEV).to(torch.bfloat16)
    ss = torch.cat([torch.rand(Cin, device=DEV) + 0.5, torch.randn(Cin, device=DEV) * 0.1])
    rss = torch.cat([torch.rand(Cin, device=DEV) + 0.5, torch.randn(Cin, device=DEV) * 0.1])
    w = (torch.randn(Cout, 1, 1, Cin, device=DEV) * 0.05).to(torch.bfloat16)
    pre = z.float() * ss[:Cin] + ss[Cin:]
    if mode == "res":
        pre = pre + r.float()
    if mode == "resbn":
        pre = pre + (r.float() * rss[:Cin] + rss[Cin:]).to(torch.bfloat16).float()
    y_ref = pre.clamp_min(0.0)
    shp = lambda t: t.view(1, 1, M, -1)  # noqa: E731
    side = torch.empty(1, 1, M, Cin, device=DEV, dtype=torch.bfloat16)
    mask = torch.empty(M, Cin // 8, device=DEV, dtype=torch.uint8)
    stats = raw.stats_buffer(M, Cout, z.device)
    out = raw.conv1x1_fwd_bnapply(shp(z), ss, w, side, mask, res=shp(r) if mode != "bn" else None,
                                  res_ss=rss if mode == "resbn" else None, stats=stats)
    y = side.view(M, Cin)
    assert rel(y, y_ref) < 1e-2
    assert torch.equal(mask, _mask_bits(y.float() > 0)), "ReLU bitmask must mark exactly the stored positives"
    of = out.view(M, Cout).float()
    ref = y_ref.to(torch.bfloat16).float() @ w.view(Cout, Cin).float().t()
    assert rel(of, ref) < 2e-2, rel(of, ref)
    st = stats.view(-1, 2, Cout)
    assert rel(st[:, 0].sum(0), of.sum(0)) < 1e-3 and rel(st[:, 1].sum(0), (of * of).sum(0)) < 1e-3


def _ext_mod():
    from cloud_amd.ops import _ext

    return _ext


def _train(fold, steps=3, wgrad_fused=False):
    os.environ["CLOUD_AMD_BN_FOLD_WGRAD"] = "1" if wgrad_fused else "0"
    os.environ["CLOUD_AMD_BN_FOLD_WGRAD1"] = "1" if wgrad_fused else "0"
    os.environ["CLOUD_AMD_BN_FOLD_WGRAD_DS"] = "1" if wgrad_fused else "0"
    os.environ["CLOUD_AMD_BN_FOLD"] = "1" if fold else "0"
    os.environ["CLOUD_AMD_BN_FOLD_FWD"] = "1" if fold else "0"
    os.environ["CLOUD_AMD_BN_FOLD_ALL"] = "1"  # every site, not only the ones the default policy keeps
    from cloud_amd.models.resnet import ResNet
    from cloud_amd.ops import softmax_cross_entropy
    from cloud_amd.optim import SGD

    torch.manual_seed(0)
    m = ResNet((2, 2, 2, 1), num_classes=10, stem_channels_pad=5, device=DEV)
    opt = SGD(m, learning_rate=0.05, momentum=0.9)
    g = torch.Generator(device=DEV).manual_seed(3)
    X = torch.randn(steps, 16, 64, 64, 3, device=DEV, generator=g).to(torch.bfloat16)
    Y = torch.randint(0, 10, (steps, 16), device=DEV, generator=g)
    grads, losses = [], []
    for i in range(steps):
        opt.zero_grad()
        loss, _ = softmax_cross_entropy(m(X[i]), Y[i], denom=16)
        loss.backward()
        torch.cuda.synchronize()
        grads.append([a.grad.detach().clone() for a in opt.arenas])
        losses.append(float(loss.detach()))
        opt.step()
    torch.cuda.synchronize()
    names = [[(s.name, s.offset, s.numel) for s in a.slots] for a in opt.arenas]
    return grads, losses, names


def test_resnet_bn_fold_bitwise(monkeypatch):
    from cloud_amd.models import fused_block
    from cloud_amd.ops import raw

    calls = {"bwd": 0, "fwd": 0}
    real_b, real_f = raw.conv1x1_dgrad_bnbwd, raw.conv1x1_fwd_bnapply

    def counting_b(*a, **k):
        calls["bwd"] += 1
        return real_b(*a, **k)

    def counting_f(*a, **k):
        calls["fwd"] += 1
        return real_f(*a, **k)

    monkeypatch.setattr(raw, "conv1x1_dgrad_bnbwd", counting_b)
    monkeypatch.setattr(raw, "conv1x1_fwd_bnapply", counting_f)
    ext = _ext_mod().load(required=True)
    # 128-wide transform-A tiles: their per-tile BN statistics happen to sum in an order that
    # reproduces the separate passes' fp32 coefficients here; the 128 x 256 tiles (the default
    # at N % 256 == 0) regroup those sums, and a 1-ulp coefficient change re-rounds a few bf16
    # dz values downstream -- checked to a tight tolerance below instead
    prev = ext.gemm_set_xa_n256(0)
    try:
        g1, l1, names = _train(True)
        n_fold = dict(calls)
        g0, l0, _ = _train(False)
        calls_off = dict(calls)
        ext.gemm_set_xa_n256(3)  # the default: two-deep 16-wave tiles
        g2, _, _ = _train(True, steps=1)
    finally:
        ext.gemm_set_xa_n256(prev)
        os.environ.pop("CLOUD_AMD_BN_FOLD", None)
        os.environ.pop("CLOUD_AMD_BN_FOLD_FWD", None)
        os.environ.pop("CLOUD_AMD_BN_FOLD_ALL", None)
        os.environ.pop("CLOUD_AMD_BN_FOLD_WGRAD", None)
        os.environ.pop("CLOUD_AMD_BN_FOLD_WGRAD1", None)
        os.environ.pop("CLOUD_AMD_BN_FOLD_WGRAD_DS", None)
    # 7 blocks: bwd folds bn3 (6 blocks get their partials from the next block) and bn1 (7);
    # fwd folds bn3 into the next conv1 (6 hand-offs) and bn2 into conv3 (all but layer 1's prw)
    assert n_fold["bwd"] > 0 and n_fold["fwd"] > 0, n_fold
    assert calls_off == n_fold, "the fused paths must run with the fold on and only then"
    # step 0 (same weights): the bf16 arena (every conv weight gradient -- it sees every dz and
    # activation the fused kernels produce) is bitwise equal; the fp32 arena (BatchNorm dgamma /
    # dbeta from fp32 finalize sums) agrees to reduction-order rounding: the 8-wave fused kernels
    # sum their per-tile BN statistics over 4-row instead of 8-row groups, and dgamma =
    # rstd * (sum g z - mean * sum g) cancels, so a slot can move by ~1e-4 relative (at most a
    # few 1e-5 absolute, measured).  Later steps are not compared
    # element-wise: a 1-ulp fp32 difference in one BN parameter re-rounds bf16 weights and
    # activations differently, and a 16-image batch amplifies that chaotically.
    for ai, (x, y) in enumerate(zip(g1[0], g0[0])):
        if x.dtype == torch.bfloat16:
            assert torch.equal(x, y), (0, ai, rel(x, y))
        else:
            bad = [(n, float((x[o:o + k] - y[o:o + k]).abs().max())) for n, o, k in names[ai]
                   if not torch.equal(x[o:o + k], y[o:o + k])]
            print("fp32 arena slots that differ at step 0:", bad)
            assert rel(x, y) < 1e-3, (0, ai, rel(x, y), bad)
    for a, b in zip(l1, l0):
        assert abs(a - b) < 0.05 * abs(b) + 1e-3, (l1, l0)
    for x, y in zip(g2[0], g1[0]):  # wide tiles: same step-0 gradients up to those re-roundings
        assert rel(x, y) < 1e-3, rel(x, y)
    assert fused_block is not None


def test_resnet_fused_dgrad_wgrad_close():
    """The fused conv3 input+weight gradient (stage 1) in a trained model: step-0 gradients
    match the unfused fold (separate weight-gradient GEMM) to bf16 / reduction-order rounding."""
    from cloud_amd.ops import raw

    calls = {"n": 0}
    real = raw.conv1x1_dgrad_wgrad_bnbwd

    def counting(*a, **k):
        calls["n"] += 1
        return real(*a, **k)

    raw.conv1x1_dgrad_wgrad_bnbwd = counting
    try:
        g1, l1, names = _train(True, steps=2, wgrad_fused=True)
        g0, l0, _ = _train(True, steps=2, wgrad_fused=False)
    finally:
        raw.conv1x1_dgrad_wgrad_bnbwd = real
        for k in ("CLOUD_AMD_BN_FOLD", "CLOUD_AMD_BN_FOLD_FWD", "CLOUD_AMD_BN_FOLD_ALL", "CLOUD_AMD_BN_FOLD_WGRAD",
                  "CLOUD_AMD_BN_FOLD_WGRAD1", "CLOUD_AMD_BN_FOLD_WGRAD_DS"):
            os.environ.pop(k, None)
    assert calls["n"] > 0
    for ai, (x, y) in enumerate(zip(g1[0], g0[0])):
        for n, o, k in names[ai]:
            assert rel(x[o:o + k], y[o:o + k]) < 2e-2, (n, rel(x[o:o + k], y[o:o + k]))
    for a, b in zip(l1, l0):
        assert abs(a - b) < 0.05 * abs(b) + 1e-3, (l1, l0)


@pytest.mark.gpu
def test_deep_fused_gradient_matches_one_step_form():
    """The deep-stream fused input+weight gradient (CLOUD_AMD_XA_DW_DEPTH=1, the default) against
    the one-step form (=0) on the stage-1 conv3 shape: the same dx bits as the one-step plain
    kernel, repeatable bits for dx and the BN statistics, weight gradients equal up to the slab
    summation order (bench/xa_dw_bench.py in one process per form: the form is read once)."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for d in ("0", "1"):
        env = dict(os.environ, CLOUD_AMD_XA_DW_DEPTH=d)
        r = subprocess.run([sys.executable, os.path.join(root, "bench", "xa_dw_bench.py"), "--batch", "8",
                            "--iters", "2"], env=env, capture_output=True, text=True, timeout=110)
        assert r.returncode == 0, r.stderr[-2000:]
        out[d] = json.loads(r.stdout.strip().splitlines()[-1])
    deep, one = out["1"], out["0"]
    assert deep["dx_repeat_equal"] and deep["stats_repeat_equal"] and deep["dx_bn_vs_plain_equal"]
    assert deep["plain"]["dx_sum"] == one["plain"]["dx_sum"] and deep["bn"]["dx_sum"] == one["plain"]["dx_sum"]
    for k in ("plain", "bn"):
        assert abs(deep[k]["dw_sum"] - one[k]["dw_sum"]) <= 1e-4 * one[k]["dw_abs"]
    assert abs(deep["bn"]["stats_sum"] - one["bn"]["stats_sum"]) <= 1e-5 * abs(one["bn"]["stats_sum"]) + 1e-3


@pytest.mark.parametrize("M,K,N", [(3000, 1024, 256), (777, 2048, 512), (1000, 512, 256)])
def test_wide_tiles_bitwise_vs_128_tiles(M, K, N):
    """The 128 x 256 transform-A tiles (16-wave, 8-wave and 16-wave two-deep forms) against the
    128 x 128 ones on
    the same inputs: the BN-backward side output dz, the forward side output y and its ReLU
    bitmask, and the GEMM results (plain, BN-statistics and residual-gated two-BN epilogues) are
    bitwise equal (same per-element K order, fixed-order BN transforms); the BN statistics
    partials agree to fp32 reduction-order rounding.  dx also equals the plain dgrad
    GEMM of the stored dz bitwise."""
    from cloud_amd.ops import _ext, raw

    ext = _ext.load(required=True)
    torch.manual_seed(M + K)
    dy = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    z = torch.randn(M, K, device=DEV).to(torch.bfloat16)
    mask = _mask_bits(torch.rand(M, K, device=DEV) > 0.4)
    coef = torch.randn(3 * K, device=DEV) * torch.tensor([1.0, 0.1, 0.01], device=DEV).repeat_interleave(K)
    w = (torch.randn(K, 1, 1, N, device=DEV) * 0.05).to(torch.bfloat16)
    zb = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    mb = _mask_bits(torch.rand(M, N, device=DEV) > 0.5)
    ss = torch.cat([torch.rand(K, device=DEV) + 0.5, torch.randn(K, device=DEV) * 0.1])
    wf = (torch.randn(N, 1, 1, K, device=DEV) * 0.05).to(torch.bfloat16)
    zr = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    src = torch.randn(M, N, device=DEV).to(torch.bfloat16)
    mr = _mask_bits(torch.rand(M, N, device=DEV) > 0.5)
    shp = lambda t: t.view(1, 1, M, -1)  # noqa: E731

    def run(mode):
        prev = ext.gemm_set_xa_n256(mode)
        try:
            side = torch.empty(1, 1, M, K, device=DEV, dtype=torch.bfloat16)
            dx, part = raw.conv1x1_dgrad_bnbwd(shp(dy), shp(z), mask, coef, w, side, bn=(shp(zb), mb))
            # residual-gated beta with a second BN (the projection shortcut's): EPI_BF16_BNR2
            side2 = torch.empty(1, 1, M, K, device=DEV, dtype=torch.bfloat16)
            out2 = torch.empty(1, 1, M, N, device=DEV, dtype=torch.bfloat16)
            r2 = raw.conv1x1_dgrad_bnbwd(shp(dy), shp(z), mask, coef, w, side2, bn=(shp(zb), mb, shp(zr)),
                                         res=(shp(src), mr), beta=1.0, out=out2)
            yside = torch.empty(1, 1, M, K, device=DEV, dtype=torch.bfloat16)
            ymask = torch.empty(M, K // 8, device=DEV, dtype=torch.uint8)
            st = raw.stats_buffer(M, N, z.device)
            out = raw.conv1x1_fwd_bnapply(shp(z), ss, wf, yside, ymask, res=shp(dy), stats=st)
            torch.cuda.synchronize()
            return side, dx, part, yside, ymask, out, st, side2, r2[0], r2[1], r2[2]
        finally:
            ext.gemm_set_xa_n256(prev)

    ref = run(0)
    for mode in ((1, 2, 3) if ext.experimental_built() else (1, 3)):  # always (1, 3): mode 2 was removed
        got = run(mode)
        for i in (0, 1, 3, 4, 5, 7, 8):
            assert torch.equal(got[i], ref[i]), (mode, i)
        # statistics partials: per 128-row tile, summed by thread groups whose row sets follow
        # the tile width -- fp32 reduction-order rounding only
        for i in (2, 6, 9, 10):
            torch.testing.assert_close(got[i], ref[i], rtol=1e-5, atol=1e-4)
    plain = raw.conv_dgrad(ref[0], w, (1, 1, M, N), 1, 0)
    assert torch.equal(plain, ref[1])
