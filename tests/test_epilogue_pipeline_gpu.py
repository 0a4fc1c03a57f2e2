"""The software-pipelined row pass of the BN-backward statistics epilogues (ca_mfma_core.h
gemm_epilogue, CLOUD_AMD_EPI_PIPE) against the one-batch-at-a-time pass it replaces.

The pipelined pass keeps every thread's rows, column group and order of additions, so the
criterion is BITWISE equality of every output and every statistics partial with the
CLOUD_AMD_EPI_PIPE=0 path -- which is the previous code, held to float64 by the edge suites
(test_dense_gemm_edges_gpu.py, test_bn_fold_edges_gpu.py, test_resnet_kernel_edges_gpu.py,
test_conv_patch_gpu.py).  No tolerance is involved.  The switch is read once per process, so the
off path runs in one child interpreter that executes the same case list from the same seeded
host inputs and saves its results.

Every case: output pre-filled with NaN (with the old values where beta reads them), followed by
guard rows that must keep their bit pattern; launched twice, the second launch bitwise the first.

Cases (the smallest that reach each way the prefetch can go wrong):
  * dense 1x1 input gradients, M = 1 / 127 / 129 / 257 (a last tile of one row: whole prefetched
    batches out of range) x N = 64 (128 x 64 tiles, four rows per thread) / 128 / 136 (an
    8-column tail tile) / 256 x K = 64 / 72, each with: statistics at beta 0 with a ReLU mask;
    beta 1 from the old output without a mask; a gated residual source with its mask; an ungated
    residual source with a second BN's statistics;
  * the sparse beta source (beta_stride 2): unstored pixels hold NaN and must never be loaded;
  * a strided 3x3 input gradient (output-parity classes: the row map);
  * a 3x3 input gradient on 256 x 64 tiles whose second partial row is zeroed;
  * the transform-A backward GEMMs: 8-wave 128 x 128 tiles and 16-wave 128 x 256 two-deep tiles;
  * the patch-fed 3x3 / stride-1 input gradient (1 x 7 x 7, 64 gathered channels), and the
    64 -> 64 channel one of the same geometry.
"""
import os
import subprocess
import sys
import tempfile
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
BF16 = torch.bfloat16
GUARD = 3  # guard rows behind every output


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _bf(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF16).to(DEV)


def _bits(g, rows, cols8):
    return torch.randint(0, 256, (rows, cols8), generator=g, dtype=torch.uint8).to(DEV)


def _raw_bytes(t):
    return t.detach().contiguous().view(torch.uint8).cpu().clone()


class _Out:
    """[rows + GUARD][cols] bf16: the first rows are the kernel's output (NaN, or `old`), the
    rest a guard pattern."""

    def __init__(self, shape, old=None):
        self.shape = shape
        self.cols = shape[-1]
        self.rows = 1
        for d in shape[:-1]:
            self.rows *= d
        self.old = old
        self.buf = torch.empty((self.rows + GUARD, self.cols), dtype=BF16, device=DEV)
        self.reset()

    def reset(self):
        self.buf[: self.rows] = float("nan") if self.old is None else self.old.view(self.rows, self.cols)
        self.buf[self.rows:] = 1.5

    @property
    def out(self):
        return self.buf[: self.rows].view(self.shape)

    def guard_ok(self):
        return bool((self.buf[self.rows:] == 1.5).all())


def _twice(name, out, launch):
    """launch() -> tuple of tensors; run twice from the same initial output, compare, return the
    first run's bytes."""
    res = []
    for _ in range(2):
        out.reset()
        r = launch()
        torch.cuda.synchronize()
        assert out.guard_ok(), f"{name}: guard rows behind the output were written"
        res.append([_raw_bytes(t) for t in r])
    for a, b in zip(*res):
        assert torch.equal(a, b), f"{name}: the second launch differs from the first"
    return res[0]


# ---- dense 1x1 input gradients
DENSE_FORMS = ("bn_mask", "beta_old", "res_gated_bn", "res_bn_z2")
DENSE = [(m, n, k) for m in (1, 127, 129, 257) for n in (64, 128, 136, 256) for k in (64, 72)]


def _dense(raw, m, n, k, form):
    name = f"dense_{m}x{n}x{k}_{form}"
    g = _gen(name)
    shape = (1, m, 1, n)
    dy = _bf(g, 1, m, 1, k)
    w = _bf(g, k, 1, 1, n, scale=k ** -0.5)
    z, z2, src, old = (_bf(g, *shape) for _ in range(4))
    mask, rmask = _bits(g, m, n // 8), _bits(g, m, n // 8)
    if form == "bn_mask":
        out = _Out(shape)
        fn = lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out.out, beta=0.0, bn=(z, mask))
    elif form == "beta_old":
        out = _Out(shape, old=old)
        fn = lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out.out, beta=1.0, bn=(z, None))
    elif form == "res_gated_bn":
        out = _Out(shape)
        fn = lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out.out, beta=1.0, bn=(z, mask), res=(src, rmask))
    else:
        out = _Out(shape)
        fn = lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out.out, beta=1.0, bn=(z, None, z2), res=(src, None))
    return name, _twice(name, out, fn)


def _sparse_beta(raw):
    name = "sparse_beta_2x5x7_c128"
    g = _gen(name)
    shape = (2, 5, 7, 128)
    m = 70
    dy, w, z = _bf(g, 2, 5, 7, 64), _bf(g, 64, 1, 1, 128, scale=0.125), _bf(g, *shape)
    old = _bf(g, *shape)
    hh = (torch.arange(5) % 2 == 0).view(1, 5, 1, 1)
    ww = (torch.arange(7) % 2 == 0).view(1, 1, 7, 1)
    stored = (hh & ww).to(DEV).expand(shape)
    old = torch.where(stored, old, torch.full_like(old, float("nan")))  # unstored pixels: never read
    out = _Out(shape, old=old)
    mask = _bits(g, m, 16)
    r = _twice(name, out, lambda: raw.conv_dgrad(dy, w, shape, 1, 0, out=out.out, beta=1.0, bn=(z, mask),
                                                 beta_stride=2))
    assert not torch.isnan(out.out.float()).any(), f"{name}: an unstored beta pixel was read"
    return name, r


def _conv3x3(raw, name, x_shape, cout, stride):
    g = _gen(name)
    nb, h, w_, cin = x_shape
    oh, ow = (h + 2 - 3) // stride + 1, (w_ + 2 - 3) // stride + 1
    dy = _bf(g, nb, oh, ow, cout)
    w = _bf(g, cout, 3, 3, cin, scale=(9 * cout) ** -0.5)
    z = _bf(g, *x_shape)
    mask = _bits(g, nb * h * w_, cin // 8)
    out = _Out(x_shape)
    return name, _twice(name, out, lambda: raw.conv_dgrad(dy, w, x_shape, stride, 1, out=out.out, bn=(z, mask)))


def _xa(raw, m, k, n, form):
    name = f"xa_{m}x{k}x{n}_{form}"
    g = _gen(name)
    shape = (1, m, 1, n)
    dy, zz = _bf(g, 1, m, 1, k), _bf(g, 1, m, 1, k)
    amask = _bits(g, m, k // 8)
    coef = (torch.randn(3 * k, generator=g) * 0.5).to(DEV)
    w = _bf(g, k, 1, 1, n, scale=k ** -0.5)
    zb, src = _bf(g, *shape), _bf(g, *shape)
    bmask, rmask = _bits(g, m, n // 8), _bits(g, m, n // 8)
    side = torch.empty_like(dy)
    out = _Out(shape)
    kw = dict(bn=(zb, bmask))
    if form == "res":
        kw.update(beta=1.0, res=(src, rmask))

    def fn():
        side.fill_(float("nan"))
        return tuple(raw.conv1x1_dgrad_bnbwd(dy, zz, amask, coef, w, side, out=out.out, **kw)) + (side,)

    return name, _twice(name, out, fn)


def run_all():
    """Every case, in a fixed order: {name: [bytes of each output / partials tensor]}."""
    from cloud_amd.ops import _ext, raw

    ext = _ext.load(required=True)
    res = {}

    def add(pair):
        res[pair[0]] = pair[1]

    for m, n, k in DENSE:
        for form in DENSE_FORMS:
            add(_dense(raw, m, n, k, form))
    add(_sparse_beta(raw))
    add(_conv3x3(raw, "conv3x3_s2_rowmap_2x9x9_c128", (2, 9, 9, 128), 64, 2))
    add(_conv3x3(raw, "conv3x3_tall256_1x17x17_c64", (1, 17, 17, 64), 64, 1))
    assert ext.conv_patch_shape(1, 7, 7, 128, 64, 3, 3, 1, 1, 1, 1, 1), "expected the patch-fed core"
    add(_conv3x3(raw, "conv3x3_patch_1x7x7_c64_to_128", (1, 7, 7, 128), 64, 1))
    add(_conv3x3(raw, "conv3x3_1x7x7_c64", (1, 7, 7, 64), 64, 1))
    for m, k, n in ((257, 64, 128), (257, 72, 256)):  # 8-wave 128 x 128; 16-wave 128 x 256 two-deep
        for form in ("bn", "res"):
            add(_xa(raw, m, k, n, form))
    return res


CASE_NAMES = ([f"dense_{m}x{n}x{k}_{f}" for m, n, k in DENSE for f in DENSE_FORMS] +
              ["sparse_beta_2x5x7_c128", "conv3x3_s2_rowmap_2x9x9_c128", "conv3x3_tall256_1x17x17_c64",
               "conv3x3_patch_1x7x7_c64_to_128", "conv3x3_1x7x7_c64"] +
              [f"xa_{m}x{k}x{n}_{f}" for m, k, n in ((257, 64, 128), (257, 72, 256)) for f in ("bn", "res")])

_CHILD = """
import sys
sys.path.insert(0, {root!r})
sys.path.insert(0, {tests!r})
import torch
import test_epilogue_pipeline_gpu as T
torch.save(T.run_all(), {path!r})
print("EPI_PIPE_CHILD_OK")
"""


@pytest.fixture(scope="module")
def both():
    """(pipelined results of this process, one-batch results of a CLOUD_AMD_EPI_PIPE=0 child)."""
    assert os.environ.get("CLOUD_AMD_EPI_PIPE", "1") not in ("0", "false", "off"), "run with the pipelined pass on"
    tests = os.path.dirname(os.path.abspath(__file__))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "off.pt")
        env = dict(os.environ, CLOUD_AMD_EPI_PIPE="0")
        code = _CHILD.format(root=os.path.dirname(tests), tests=tests, path=path)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=110)
        assert r.returncode == 0 and "EPI_PIPE_CHILD_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
        off = torch.load(path)
    on = run_all()
    return on, off


def test_case_list_complete(both):
    on, off = both
    assert list(on) == CASE_NAMES and list(off) == CASE_NAMES


@pytest.mark.parametrize("name", CASE_NAMES)
def test_pipelined_bitwise_equals_one_batch_pass(both, name):
    on, off = both
    assert len(on[name]) == len(off[name]) >= 2
    for i, (a, b) in enumerate(zip(on[name], off[name])):
        assert a.shape == b.shape, (name, i)
        assert torch.equal(a, b), f"{name}: tensor {i} differs in {int((a != b).sum())} of {a.numel()} bytes"
    dx = on[name][0].view(BF16)
    if not name.startswith("sparse_beta"):
        assert not torch.isnan(dx.float()).any(), f"{name}: output rows left unwritten"
