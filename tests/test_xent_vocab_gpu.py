"""Softmax cross-entropy at vocabulary width (csrc/kernels/xent_vocab.hip) through
``ops.softmax_cross_entropy`` and Keras, against float64.

Reference, metrics and bounds are those of ``test_bert_kernel_edges_gpu._xent_check``: fp64
``F.cross_entropy`` of the same bf16 / fp32 inputs over the rows that are not ignored; loss and
``acc[0]`` to ``atol = rtol = 1e-3``; gradient to ``rtol = tol``, ``atol = tol / denom`` with
``tol`` 2e-2 (bf16: one rounding of the stored gradient is 2^-9 relative, the bound leaves 5x)
or 1e-5 (fp32); ``correct``, ``acc[1]``, ``acc[2]`` exact (smallest index among tied maxima,
spelled out); ignored gradient rows exactly zero.  ``denom`` there is the divisor of the mean:
``2N``, or the number of valid rows under ``denom="valid"``.

The shapes are the smallest that reach every path: one column, fewer columns than one vector,
many rows (several trips of the finalising block), every (lanes, vectors per lane) instantiation
(``C`` = 130 .. 50257), ragged last vectors, odd row pitches, and per dtype the widths next to
the resident limit (bf16 65536, fp32 32768 columns), above which the streaming form runs.
``vocab_route`` sends every shape to the new kernels (by default the small ones belong to the
one-block batch kernel) and checks that they ran.

Worst figures observed on an MI355X (each test prints its own before asserting):

    quantity                                      worst observed   bound
    loss, |got - ref|, bf16 / fp32                1.42e-6 / 3.76e-6  1e-3 (+ 1e-3 relative)
    gradient bf16, max |got - ref| * denom        2.68e-3          2e-2 (+ 2e-2 relative)
    gradient fp32, max |got - ref| * denom        2.95e-7          1e-5 (+ 1e-5 relative)
    Keras fit step, |mixed_bfloat16 - fp32 torch| 2.0e-4 / 2.5e-4  1e-2
                                                  (without / with ignore_class)
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

DEV = "cuda"
ACC0 = (1.5, 2.0, 3.0)
ACC_W = 0.5
DTYPES = [torch.bfloat16, torch.float32]
# resident limits of xent_vocab.hip (the file header; ca_xent_vocab_resident_max)
RESIDENT = {torch.bfloat16: 65536, torch.float32: 32768}


def _say(*a):
    print("[xent-vocab]", *a, flush=True)


@pytest.fixture
def vocab_route(monkeypatch):
    """Every call takes the xent_vocab.hip route; yields the list of (N, C) it ran."""
    from cloud_amd.ops import losses

    ran = []
    fwd = losses._vocab_forward

    def spy(ext, logits, *a, **k):
        ran.append(tuple(logits.shape))
        return fwd(ext, logits, *a, **k)

    monkeypatch.setattr(losses, "_vocab_forward", spy)
    monkeypatch.setattr(losses, "_VOCAB_MIN_C", 1)
    monkeypatch.setattr(losses, "_BATCH_KERNEL_MAX", 0)
    return ran


def _inputs(N, C, dtype, seed=1, scale=3.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    z = (torch.randn(N, C, device=DEV, generator=g) * scale).to(dtype)
    y = torch.randint(0, C, (N,), device=DEV, generator=g)
    return z, y


def _run(z, y, ls, denom, grad_mult, pad=0, ignore_index=None):
    """One forward + backward.  pad > 0: the logits are the [:, :C] view of a [N, C + pad] leaf
    filled with 100.0 past C.  grad_mult None: unit-seed backward; else backward of
    grad_mult * loss."""
    from cloud_amd.ops import softmax_cross_entropy
    from cloud_amd.ops.losses import unit_seed

    N, C = z.shape
    if pad:
        leaf = torch.full((N, C + pad), 100.0, dtype=z.dtype, device=DEV)  # would win every argmax / sum
        leaf[:, :C] = z
        leaf.requires_grad_()
        zz = leaf[:, :C]
        assert zz.stride(0) == C + pad
    else:
        leaf = z.clone().requires_grad_()
        zz = leaf
    acc = torch.tensor(ACC0, device=DEV)
    loss, correct = softmax_cross_entropy(zz, y, denom=denom, label_smoothing=ls, acc=acc, acc_weight=ACC_W,
                                          ignore_index=ignore_index)
    if grad_mult is None:
        torch.autograd.backward(loss, grad_tensors=unit_seed(loss.device))
    else:
        (grad_mult * loss).backward()
    grad = leaf.grad
    if pad:
        assert torch.equal(grad[:, C:], torch.zeros_like(grad[:, C:]))
        grad = grad[:, :C].contiguous()
    assert grad.dtype == z.dtype and correct.shape == (N,)
    return loss.detach(), correct, grad, acc


def _check(z, y, ls, denom, pad=0, ignore_index=None, tag=""):
    """Loss, correct flags, both backward forms and the metric accumulator against fp64."""
    N, C = z.shape
    tol = 2e-2 if z.dtype == torch.bfloat16 else 1e-5
    zd = z.double()
    valid = (y >= 0) & (y < C)
    if ignore_index is not None:
        valid &= y != ignore_index
    nvalid = int(valid.sum().item())
    by_valid = denom == "valid"
    div = float(max(nvalid, 1)) if by_valid else float(denom)
    zr = zd.clone().requires_grad_()
    per = F.cross_entropy(zr[valid], y[valid], reduction="none", label_smoothing=ls)
    (per.sum() / div).backward()
    ref_loss, ref_grad = (per.sum() / div).detach(), zr.grad
    cols = torch.arange(C, device=DEV).expand(N, C)
    first = torch.where(zd == zd.max(-1, keepdim=True).values, cols, torch.full_like(cols, C)).min(-1).values
    ref_correct = ((first == y) & valid).float()
    rows = float(nvalid) if by_valid else float(N)
    ref_acc = torch.tensor(ACC0, device=DEV).double() + ACC_W * torch.stack(
        [per.sum().detach(), ref_correct.sum().double(), torch.tensor(rows, device=DEV).double()])

    loss, correct, g1, acc = _run(z, y, ls, denom, None, pad, ignore_index)
    loss3, correct3, g3, _ = _run(z, y, ls, denom, 3.0, pad, ignore_index)
    torch.cuda.synchronize()
    _say(f"{tag} N={N} C={C} pad={pad} {z.dtype} ls={ls} denom={denom}: loss err "
         f"{(loss.double() - ref_loss).abs().item():.3e} grad max abs err * denom "
         f"{((g1.double() - ref_grad).abs().max() * div).item():.3e}")
    assert math.isfinite(loss.item())
    torch.testing.assert_close(loss.double(), ref_loss, atol=1e-3, rtol=1e-3)
    assert torch.equal(loss, loss3) and torch.equal(correct, correct3)
    assert torch.equal(correct, ref_correct)
    torch.testing.assert_close(g1.double(), ref_grad, atol=tol / div, rtol=tol)
    torch.testing.assert_close(g3.double(), 3 * ref_grad, atol=tol / div, rtol=tol)
    assert torch.equal(g1[~valid], torch.zeros_like(g1[~valid]))
    assert torch.equal(g3[~valid], torch.zeros_like(g3[~valid]))
    torch.testing.assert_close(acc[0].double(), ref_acc[0], atol=1e-3, rtol=1e-3)
    assert acc[1].item() == ref_acc[1].item() and acc[2].item() == ref_acc[2].item(), (acc, ref_acc)
    return loss, correct, g1, acc


# (1, 1) .. (2053, 130): below one vector, one partial vector, many rows (three trips of the
# finalising block); then one shape per (lanes, vectors) instantiation, all with ragged or odd C
SHAPES = [(1, 1), (3, 7), (2053, 130), (5, 4099), (3, 8200), (3, 32768), (2, 50257)]


@pytest.mark.parametrize("N,C", SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_vs_fp64(vocab_route, N, C, dtype, ls):
    z, y = _inputs(N, C, dtype)
    _check(z, y, ls, 2 * N)
    assert vocab_route and all(s == (N, C) for s in vocab_route)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("off", [-3, 0, 5])
def test_next_to_the_resident_limit(vocab_route, dtype, off):
    """The widest resident instantiation and the streaming form, 3 rows, one of them ignored."""
    from cloud_amd.ops import _ext

    limit = RESIDENT[dtype]
    assert _ext.load(required=True).xent_vocab_resident_max(int(dtype == torch.bfloat16)) == limit
    C = limit + off
    z, y = _inputs(3, C, dtype, seed=4)
    y[0] = C - 1
    _check(z, y, 0.1, 6, tag="limit")
    y[1] = -1
    _check(z, y, 0.0, "valid", tag="limit")
    assert len(vocab_route) == 4


@pytest.mark.parametrize("N,C", [(2053, 130), (5, 4099), (3, 8200), (2, 50257)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_padded_head_view(vocab_route, N, C, dtype):
    """The [:, :C] view of a C + 7 wide buffer (odd pitches: rows on 2- / 4-byte boundaries),
    100.0 past C: the padding never wins the arg-max nor enters a sum, and its gradient columns
    come back zero through autograd."""
    z, y = _inputs(N, C, dtype, seed=5)
    y[0] = -1
    for ls in (0.0, 0.1):
        _check(z, y, ls, 2 * N, pad=7, tag="padded")
    _check(z, y, 0.0, "valid", pad=7, tag="padded")


@pytest.mark.parametrize("N,C", [(3, 7), (2053, 130), (5, 4099), (3, 32768)])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mode", ["2N", "valid", "valid-ignore_index"])
def test_ignored_rows(vocab_route, N, C, dtype, mode):
    """A third of the labels -1 or C, or equal to an in-range ignore_index: zero loss, zero
    correct, exactly zero gradient rows; counted in 2N and acc[2], not under 'valid'."""
    z, y = _inputs(N, C, dtype, seed=2)
    ig = None
    if mode == "valid-ignore_index":
        ig = 2
        y[1::3] = ig
    else:
        y[1::6] = -1
        y[4::6] = C
    gone = (y < 0) | (y >= C) | (y == (-7 if ig is None else ig))
    assert N // 3 <= gone.sum().item() < N
    for ls in (0.0, 0.1):
        _, correct, _, _ = _check(z, y, ls, 2 * N if mode == "2N" else "valid", ignore_index=ig, tag=mode)
        assert correct[gone].sum().item() == 0


@pytest.mark.parametrize("N,C", [(3, 7), (3, 8200)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_all_ignored_batch_under_valid(vocab_route, N, C, dtype):
    z, _ = _inputs(N, C, dtype, seed=3)
    y = torch.tensor([-1, C, 5][:N], device=DEV)
    loss, correct, g, acc = _check(z, y, 0.1, "valid", ignore_index=5, tag="all-ignored")
    assert loss.item() == 0.0 and correct.sum().item() == 0
    assert torch.equal(g, torch.zeros_like(g))
    assert acc.tolist() == list(ACC0)


@pytest.mark.parametrize("N,C", [(3, 130), (3, 8200), (2, 32768 + 5)])
def test_large_magnitude_fp32(vocab_route, N, C):
    """Logits of magnitude 60: exp() of the raw values overflows fp32, the max-subtracted form
    (and the streaming form's rescaling) does not."""
    g = torch.Generator(device=DEV).manual_seed(3)
    z = (torch.rand(N, C, device=DEV, generator=g) * 2 - 1) * 60
    y = torch.randint(0, C, (N,), device=DEV, generator=g)
    z[0, y[0]] = -60.0  # a large loss
    z[1, y[1]] = 60.0
    for ls in (0.0, 0.1):
        _check(z, y, ls, 2 * N, tag="magnitude")


@pytest.mark.parametrize("C", [4099, 8200 + 3, None])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tied_maxima_go_to_the_smallest_index(vocab_route, C, dtype):
    """The row maximum at columns 700 and 1500 (different waves of every instantiation used)
    and once more in the ragged last vector (which belongs to a LOW lane: wave order is not
    column order): 700 wins, whichever of the three the label names."""
    C = RESIDENT[dtype] + 5 if C is None else C
    z, _ = _inputs(4, C, dtype, seed=6)
    tied = [700, 1500, C - 1]
    z[:, tied] = 50.0
    y = torch.tensor(tied + [3], device=DEV)
    _, correct, _, _ = _check(z, y, 0.0, 8, tag="ties")
    assert correct.tolist() == [1.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("C", [7, 130, 4099, 50257, None])
@pytest.mark.parametrize("dtype", DTYPES)
def test_maximum_in_the_last_column(vocab_route, C, dtype):
    C = RESIDENT[dtype] + 5 if C is None else C
    z, y = _inputs(2, C, dtype, seed=7)
    z[:, C - 1] = 40.0
    y[0], y[1] = C - 1, 0
    _, correct, _, _ = _check(z, y, 0.1, 4, tag="last-column")
    assert correct.tolist() == [1.0, 0.0]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("denom", [None, "valid"])
def test_3d_input_equals_the_flattened_call_bitwise(vocab_route, dtype, denom):
    from cloud_amd.ops import softmax_cross_entropy

    C = 4099
    z, y = _inputs(10, C, dtype, seed=8)
    y[3] = -1
    outs = []
    for shape in ((2, 5), (10,)):
        leaf = z.reshape(shape + (C,)).clone().requires_grad_()
        acc = torch.tensor(ACC0, device=DEV)
        loss, correct = softmax_cross_entropy(leaf, y.reshape(shape), denom=denom, label_smoothing=0.1, acc=acc)
        loss.backward()
        assert leaf.grad.shape == shape + (C,) and correct.shape == (10,)
        outs.append((loss.detach(), correct, leaf.grad.reshape(10, C), acc))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert vocab_route == [(10, C), (10, C)]


@pytest.mark.parametrize("N,C", [(2053, 130), (3, 8200), (2, 65536 + 5)])
@pytest.mark.parametrize("denom", [None, "valid"])
def test_two_identical_calls_are_bitwise_equal(vocab_route, N, C, denom):
    z, y = _inputs(N, C, torch.bfloat16, seed=9)
    y[1] = -1
    a = _run(z, y, 0.1, N if denom is None else denom, None)
    b = _run(z, y, 0.1, N if denom is None else denom, None)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.parametrize("dtype", DTYPES)
def test_default_routing(monkeypatch, dtype):
    """With the default threshold (130, 1009) and (64, 1000) stay on the kernels they ran on
    before, bitwise; a batch past the one-block kernel at C >= the threshold takes the new ones,
    and denom='valid' does at any size."""
    from cloud_amd import config
    from cloud_amd.ops import _ext, losses

    assert losses._VOCAB_MIN_C == config.get("CLOUD_AMD_XENT_VOCAB_MIN_C") > 1009
    ran = []
    fwd = losses._vocab_forward
    monkeypatch.setattr(losses, "_vocab_forward", lambda ext, z, *a, **k: (ran.append(tuple(z.shape)), fwd(ext, z, *a, **k))[1])
    ext = _ext.load(required=True)
    st = _ext.stream_handle(torch.device(DEV, torch.cuda.current_device()))
    bf = int(dtype == torch.bfloat16)

    B, C = 130, 1009  # past _BATCH_KERNEL_MAX: the row-parallel kernel
    assert B * C > losses._BATCH_KERNEL_MAX
    z, y = _inputs(B, C, dtype, seed=10)
    loss, correct, g, _ = _run(z, y, 0.1, 2 * B, None)
    rows, flags, dz = torch.empty(B, device=DEV), torch.empty(B, device=DEV), torch.empty_like(z)
    ext.softmax_xent(z.data_ptr(), bf, y.data_ptr(), B, C, 1.0 / (2 * B), 0.1, rows.data_ptr(), flags.data_ptr(),
                     dz.data_ptr(), st)
    assert torch.equal(loss, rows.sum() / float(2 * B)) and torch.equal(correct, flags) and torch.equal(g, dz)

    B, C = 64, 1000  # the one-block batch kernel
    z, y = _inputs(B, C, dtype, seed=11)
    loss, correct, g, acc = _run(z, y, 0.1, 2 * B, None)
    mean, flags, dz = torch.empty(1, device=DEV), torch.empty(B, device=DEV), torch.empty_like(z)
    acc2 = torch.tensor(ACC0, device=DEV)
    ext.softmax_xent_batch(z.data_ptr(), C, bf, y.data_ptr(), B, C, 1.0 / (2 * B), 0.1, mean.data_ptr(),
                           flags.data_ptr(), dz.data_ptr(), acc2.data_ptr(), ACC_W, st)
    assert torch.equal(loss, mean[0]) and torch.equal(correct, flags) and torch.equal(g, dz) and torch.equal(acc, acc2)
    assert ran == []

    thr = losses._VOCAB_MIN_C
    B = losses._BATCH_KERNEL_MAX // thr + 1
    z, y = _inputs(B, thr, dtype, seed=12)
    _check(z, y, 0.0, 2 * B, tag="default-route")
    assert ran == [(B, thr)] * 2
    z, y = _inputs(3, 7, dtype, seed=13)
    _check(z, y, 0.0, "valid", tag="default-route")
    assert ran[2:] == [(3, 7)] * 2


# ---------------------------------------------------------------- Keras

VOCAB, SEQ, DIM, BATCH, HOT = 4099, 16, 64, 4, 5


def _decoder():
    from cloud_amd import keras
    from cloud_amd.keras import layers

    inp = keras.Input(shape=(SEQ,))
    x = layers.Embedding(VOCAB, DIM)(inp)
    a = layers.MultiHeadAttention(2, DIM // 2, use_causal_mask=True)([x, x])
    x = layers.Add()([x, a])
    x = layers.LayerNormalization()(x)
    x = layers.Dense(128, activation="relu")(x)
    return keras.Model(inp, layers.Dense(VOCAB)(x))


@pytest.mark.parametrize("ignore_class", [None, 0])
def test_keras_fit_step_mixed_bfloat16(monkeypatch, ignore_class):
    """One fit step of the tiny decoder under mixed_bfloat16 (64 tokens x 4099 logits: past the
    one-block kernel and the default threshold): the logged loss is within 1e-2 of the float32
    torch route on the same weights, the logged accuracy is SparseCategoricalAccuracy of the
    logits the step saw (all positions, padding included)."""
    from cloud_amd import keras
    from cloud_amd.keras import engine, losses, metrics
    from cloud_amd.ops import losses as ops_losses

    r = np.random.RandomState(0)
    x = r.randint(1, VOCAB, size=(BATCH, SEQ)).astype(np.int64)
    y = r.randint(1, VOCAB, size=(BATCH, SEQ)).astype(np.int64)
    y[:, ::2] = HOT       # the class the head's bias favours: a non-trivial accuracy
    y[:, 11:] = 0         # padding; class 0 is scored as any other class unless ignored
    ran, seen = [], []
    fwd = ops_losses._vocab_forward
    monkeypatch.setattr(ops_losses, "_vocab_forward",
                        lambda ext, z, *a, **k: (ran.append(tuple(z.shape)), fwd(ext, z, *a, **k))[1])
    old = engine._POLICY
    try:
        engine.set_global_policy("mixed_bfloat16")
        torch.manual_seed(0)
        model = _decoder()
        model.predict(x, batch_size=BATCH, verbose=0)  # builds the layers
        with torch.no_grad():
            model.layers[-1].bias[HOT] = 2.0
        weights = model.get_weights()
        loss_obj = losses.SparseCategoricalCrossentropy(from_logits=True, ignore_class=ignore_class)
        fused = loss_obj.fused_logits_loss
        monkeypatch.setattr(loss_obj, "fused_logits_loss",
                            lambda logits, *a, **k: (seen.append(logits.detach().clone()), fused(logits, *a, **k))[1])
        model.compile(optimizer=keras.optimizers.SGD(1e-3), loss=loss_obj, metrics=["accuracy"])
        hist = model.fit(x, y, batch_size=BATCH, epochs=1, verbose=0, shuffle=False)
        loss, acc = hist.history["loss"][0], hist.history["accuracy"][0]

        engine.set_global_policy("float32")
        ref = _decoder()
        xc, yc = torch.as_tensor(x), torch.as_tensor(y)
        with torch.no_grad():
            ref(xc)  # builds on the CPU: the torch route
            ref.set_weights(weights)
            ref_loss = losses.SparseCategoricalCrossentropy(from_logits=True, ignore_class=ignore_class)(
                yc, ref(xc).double()).item()
    finally:
        engine._POLICY = old
    assert len(seen) == 1 and seen[0].shape == (BATCH, SEQ, VOCAB) and seen[0].dtype == torch.bfloat16
    assert ran == [(BATCH * SEQ, VOCAB)]
    m = metrics.SparseCategoricalAccuracy()
    m.update_state(torch.as_tensor(y, device=DEV), seen[0])
    by_hand = float((seen[0].float().argmax(-1).cpu().numpy() == y).mean())
    _say(f"keras fit step ignore_class={ignore_class}: loss {loss:.5f} fp32 torch {ref_loss:.5f} "
         f"diff {abs(loss - ref_loss):.3e}; accuracy {acc:.4f} by hand {by_hand:.4f}")
    assert math.isfinite(loss) and abs(loss - ref_loss) <= 1e-2
    assert 0.3 < by_hand < 0.7
    assert abs(acc - float(m.result())) < 1e-7 and abs(acc - by_hand) < 1e-7
