"""Edge-case reference tests for the fused optimizer and grad-norm kernels
(csrc/kernels/optim.hip: ca_sgd_step, ca_adam_step, ca_rmsprop_step, ca_sumsq, ca_scale), called
through the ``ext.*`` bindings directly, and for what cloud_amd/optim/fused.py builds on them
(``step()``, ``prepare_step()`` + ``step_kernels()``, ``sliced_update``, the fused zero-grad
bookkeeping, ``clipnorm``).

The float64 reference, the criterion |got - ref| <= PART_BOUND * S with its derivation (rounding
counts per rule), the inputs and the hyper-parameter grids are those of
test_optim_reference_cpu.py, which proves them on the CPU; nothing here is tuned to a run.
Inputs come from a host ``torch.Generator`` with a fixed seed per case.

Every tensor a kernel may write (p, g, the state tensors, p16, the sumsq accumulator) is a window
[lo, lo + n) behind GUARD = 256 elements of a larger allocation that is pre-filled with the NaN
SENTINEL patterns of test_bn_fold_edges_gpu.py and carries 256 more after the window.  ``lo`` is
always a multiple of 8 elements: 16-byte alignment of every pointer is the kernels' contract (the
arena pads every slot to 64), and a misaligned pointer would provoke a fault on purpose, which no
test here does.

    what                                     criterion (origin)
    p, m, v, ms, buf after one launch        per element <= PART_BOUND * S (derived: <= 16 counted
                                             fp32 roundings per rule, test_optim_reference_cpu.py)
    p16                                      bit-identical to p_after.to(bfloat16) (f2bf is RNE)
    g                                        zero_g 1: all-zero bits, tail included; 0: bits unchanged
    guards, both sides, every tensor         the sentinel, bit for bit
    a second launch from the same inputs     identical bits
    hp from a device tensor vs by value      identical bits (one kernel, one arithmetic)
    g * 2^10 with grad_scale 2^-10           identical bits to g with grad_scale 1 (exact scaling)
    momentum with ``first``                  m window left at the NaN sentinel: finite, m = g gs + wd p
    Adam, g = m = v = 0                      coupled, wd 0: p bit-identical; decoupled: the criterion
    sumsq, integers in {-2..2}               torch.equal with 3 + the float64 sum (every partial sum is
                                             an integer below 2^24: any order of the atomics is exact)
    sumsq, non-integer, n <= 1279            |err| <= PART_BOUND * sum g^2 (derived: 1 square, 1 add
                                             per trip, 6 wave_sum levels, 3 adds of the wave sums, one
                                             atomic per block: 1 + 1 + 6 + 3 + 5 = 16 at 5 blocks; a
                                             chain of 2048 atomics has no 16-rounding bound, so the
                                             sizes past one grid are covered by the integer cases)
    scale                                    bit-identical to the host's fp32 multiply (+ RNE to bf16)
    step() over five steps                   the one-step criterion from a device snapshot before each
                                             step; padding exactly 0; model copy = RNE(master)
    sliced_update                            the criterion inside [lo, hi) with each side's weight
                                             decay; every bit outside unchanged
    clipnorm                                 below: bits unchanged; above: 2^-8 |ref| + 2^-20 |g| (one
                                             bf16 rounding + the fp32 norm), fp32 arenas 2^-20 |g|

Sizes.  SGD and Adam move 8 elements per lane (``n / 8`` vectors, then a scalar tail) on a grid
that ``ca_stream_grid`` caps at 2048 blocks of 256: N_VEC below are nothing, tail only (1, 7), one
vector, one vector + tail, a partial block + tail, and a partly filled second grid-stride trip +
tail.  RMSprop, sumsq and scale move one element per lane: N_SCALAR.

Worst figures observed on an MI355X (each test prints its figures with ``[edges]`` before
asserting; they are reported, never used to set a bound):

    what                                                  worst err / bound                  bound
    sizes, SGD (worst at 4 200 453): p, m                 0.178, 0.173                       1
    sizes, Adam (worst at 4 200 453): p, m, v             0.269, 0.163, 0.288                1
    sizes, RMSprop (worst at 525 065): p, ms, buf         0.196, 0.248, 0.232                1
    offsets 0 / 8 / 64: SGD p, m; Adam p, m, v            0.133, 0.143; 0.199, 0.137, 0.238  1
    offsets 0 / 8 / 64: RMSprop p, ms, buf                0.160, 0.215, 0.192                1
    SGD grid x dtype x p16 x zero_g: p, m                 0.158, 0.144                       1
    Adam grid x dtype x p16 x zero_g: p, m, v             0.291, 0.148, 0.241                1
    RMSprop grid x dtype x p16 x zero_g: p, ms, buf       0.193, 0.238, 0.197                1
    repeat launch; device hp; 2^10 grad_scale             0 bits differ                      identical
    p16 against RNE(p); g zeroed / kept; guards           0 bits differ                      identical
    sumsq integers, all sizes, both dtypes                0 (e.g. 1 052 035 at n = 525 065)  exact
    sumsq non-integer n = 1 / 255 / 257 / 1279            0.021, 0.104, 0.034, 0.069         1
    scale, k = 0.5, 1/3, 0, all sizes                     0 bits differ                      identical
    five steps: SGD p, m; Adam p, m, v                    0.125, 0.129; 0.180, 0.133, 0.210  1
    five steps: AdamW p, m, v; RMSprop p, ms, buf         0.189, 0.106, 0.113; 0.183, 0.217, 0.193  1
    device hp path, worst of the four: p, state           0.218, 0.226; bits = step()        1; identical
    sliced_update, worst of the four: p, state            0.141, 0.184; outside 0 bits       1; identical
    clipnorm above (norm 3 and 1.5): gradient; then p, m  0.700; 0.102, 0.098                1

No kernel defect showed.  The 0.700 of clipnorm is the one bf16 rounding of the rescaled
gradient; everything else sits at a fifth to a third of the 16 roundings allowed, as the fp32 CPU
path does (0.16 - 0.26 in test_optim_reference_cpu.py).
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_bn_fold_edges_gpu as B  # noqa: E402  (NaN sentinels of the BN-fold edge tests)
import test_optim_reference_cpu as O  # noqa: E402  (fp64 reference, criterion, inputs, grids)

pytestmark = pytest.mark.gpu

PART_BOUND, SENTINEL, _say, _D = O.PART_BOUND, B.SENTINEL, O._say, O._D
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
GUARD = 256

# csrc/include/ca_common.h ca_stream_grid: at most GRID_CAP blocks; optim.hip: BLOCK lanes per
# block, VEC elements per lane in the SGD / Adam vector loops (``nv = n / 8``).  If any of the
# three changes, re-pick the sizes below.
GRID_CAP, BLOCK, VEC = 2048, 256, 8
N_VEC_LARGE = GRID_CAP * BLOCK * VEC + VEC * BLOCK * 3 + 5  # a 2nd trip of 3 blocks, + a tail of 5
N_SCALAR_LARGE = GRID_CAP * BLOCK + 777                     # a 2nd trip of 777 lanes
N_VEC = [0, 1, 7, 8, 9, 2047, N_VEC_LARGE]
N_SCALAR = [0, 1, 255, 257, N_SCALAR_LARGE]
N_EDGE, LO_EDGE = 2047, 64


def _ext():
    from cloud_amd.ops import _ext as e

    return e.load(required=True)


def _st():
    from cloud_amd.ops import _ext as e

    return e.stream_handle(torch.device(DEV, torch.cuda.current_device()))


def _bits(t):
    return t.contiguous().view(SENTINEL[t.dtype][0])


def _same(a, b):
    return (a is None and b is None) or torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------- guarded windows


class _Win:
    """A window [lo, lo + n) behind GUARD elements of a flat allocation filled with the NaN
    sentinel of its type, with GUARD more after it; ``src`` (host) is copied into the window."""

    def __init__(self, name, dtype, lo, n, src=None):
        assert lo % VEC == 0, "16-byte alignment is the kernels' contract"
        it, pat = SENTINEL[dtype]
        self.name, self.it, self.pat = name, it, pat
        self.a, self.b = GUARD + lo, GUARD + lo + n
        self.buf = torch.empty(self.b + GUARD, dtype=dtype, device=DEV)
        self.buf.view(it).fill_(pat)
        if src is not None and n:
            self.buf[self.a:self.b].copy_(src.to(dtype))
        self.ptr = self.buf.data_ptr() + self.a * self.buf.element_size()
        assert self.ptr % 16 == 0

    def host(self):
        """The window on the host, after asserting that both guards still hold the sentinel."""
        raw = self.buf.cpu()
        v = raw.view(self.it)
        assert bool((v[:self.a] == self.pat).all()), f"{self.name}: written before the window"
        assert bool((v[self.b:] == self.pat).all()), f"{self.name}: written past the window"
        return raw[self.a:self.b]


def _ptr(w):
    return 0 if w is None else w.ptr


def _launch(kind, d, c, lo=LO_EDGE, p16=True, zero_g=1, hp_dev=False):
    """One launch of ``kind`` over the inputs ``d`` with the grid case ``c``; every tensor in a
    fresh guarded window.  Returns the windows' contents on the host (guards checked)."""
    ext, n, gbf = _ext(), d.n, int(d.gdtype == BF16)
    w = _D(p=_Win("p", F32, lo, n, d.p), g=_Win("g", d.gdtype, lo, n, d.g),
           p16=_Win("p16", BF16, lo, n) if p16 else None)
    hp = torch.tensor(c.hv, dtype=F32, device=DEV) if hp_dev else None
    hpp, hv = (hp.data_ptr(), []) if hp_dev else (0, list(c.hv))
    if kind == "sgd":
        w.m = None if c.m == "null" else _Win("m", F32, lo, n, d.m if c.m == "rand" else None)
        ext.sgd_step(w.p.ptr, w.g.ptr, gbf, _ptr(w.m), _ptr(w.p16), hpp, hv, n, int(c.nesterov), zero_g, _st())
    elif kind == "adam":
        w.m, w.v = _Win("m", F32, lo, n, d.m), _Win("v", F32, lo, n, d.v)
        ext.adam_step(w.p.ptr, w.g.ptr, gbf, w.m.ptr, w.v.ptr, _ptr(w.p16), hpp, hv, n, int(c.decoupled), zero_g,
                      _st())
    else:
        w.ms = _Win("ms", F32, lo, n, d.v)
        w.buf = _Win("buf", F32, lo, n, d.buf) if c.mom != 0.0 else None
        ext.rmsprop_step(w.p.ptr, w.g.ptr, gbf, w.ms.ptr, _ptr(w.buf), _ptr(w.p16), hpp, hv, n, zero_g, _st())
    torch.cuda.synchronize()
    return _D({k: (None if x is None else x.host()) for k, x in w.items()})


def _same_outputs(a, b):
    return all(_same(a[k], b[k]) for k in a)


def _verify(tag, d, ref, out, zero_g):
    """Window contents against the reference: the criterion per output, the model copy, the
    gradient's fused zeroing.  Returns {output: err / bound}."""
    worst = O.check_outputs(tag, out, ref, O._names(ref))
    if out.p16 is not None:
        assert _same(out.p16, out.p.to(BF16)), f"{tag}: model copy is not RNE(p)"
    if zero_g:
        assert not bool(_bits(out.g).any()), f"{tag}: consumed gradient elements not zeroed"
    else:
        assert _same(out.g, d.g), f"{tag}: gradient changed with zero_g = 0"
    return worst


REF = {"sgd": O.sgd_ref, "adam": O.adam_ref, "rms": O.rms_ref}
# the fullest line of each rule, for the size and offset sweeps
FULL = {"sgd": O._case(O.SGD_CASES, m="rand", damp=0.25, nesterov=True, wd=1e-2),
        "adam": O._case(O.ADAM_CASES, decoupled=False, wd=1e-2, eps=1e-7, t=1000),
        "rms": O._case(O.RMS_CASES, mom=0.5, wd=1e-3, gs=0.5)}
KINDS = ["sgd", "adam", "rms"]
_gd = pytest.mark.parametrize("gdtype", O.GDTYPES, ids=["bf16", "fp32"])


def _merge(worst, w):
    for k, v in w.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ------------------------------------------------------------------------------- sizes, offsets


@_gd
@pytest.mark.parametrize("kind,n", [(k, n) for k in KINDS for n in (N_SCALAR if k == "rms" else N_VEC)])
def test_sizes(kind, n, gdtype):
    c = FULL[kind]
    d = O.make_inputs(n, 1000 + n % 997, gdtype, zero_block=kind == "adam")
    ref = REF[kind](d, c)
    out = _launch(kind, d, c)
    _verify(f"{kind} n={n} {c.name}", d, ref, out, 1)
    assert _same_outputs(out, _launch(kind, d, c)), "a second launch from the same inputs differs"


@_gd
@pytest.mark.parametrize("lo", [0, 8, 64])
@pytest.mark.parametrize("kind", KINDS)
def test_window_offsets(kind, lo, gdtype):
    c = FULL[kind]
    d = O.make_inputs(N_EDGE, 1100 + lo, gdtype, zero_block=kind == "adam")
    ref = REF[kind](d, c)
    out = _launch(kind, d, c, lo=lo)
    _verify(f"{kind} lo={lo}", d, ref, out, 1)
    assert _same_outputs(out, _launch(kind, d, c, lo=lo))


# ------------------------------------------------------------------------------- the grids


def _cross(kind, c, seed, extra=None):
    """gradient dtype x p16 x zero_g at N_EDGE / LO_EDGE; each: by value, by value again, from a
    device tensor -- all three bit-identical, the first against the reference."""
    worst = {}
    for gdtype in O.GDTYPES:
        d = O.make_inputs(N_EDGE, seed, gdtype, zero_block=kind == "adam")
        ref = REF[kind](d, c)
        for p16 in (True, False):
            for zero_g in (1, 0):
                tag = f"{kind} {c.name} {'bf16' if gdtype == BF16 else 'fp32'} p16={int(p16)} zero_g={zero_g}"
                out = _launch(kind, d, c, p16=p16, zero_g=zero_g)
                _merge(worst, _verify(tag, d, ref, out, zero_g))
                assert _same_outputs(out, _launch(kind, d, c, p16=p16, zero_g=zero_g)), f"{tag}: not repeatable"
                assert _same_outputs(out, _launch(kind, d, c, p16=p16, zero_g=zero_g, hp_dev=True)), \
                    f"{tag}: device hyper-parameters give other bits than the same values by value"
                if extra is not None:
                    extra(tag, d, out)
    _say(f"{kind} {c.name}: worst err / bound over the cross product", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("c", O.SGD_CASES, ids=O._ids)
def test_sgd_grid(c):
    _cross("sgd", c, 1200 + O.SGD_CASES.index(c))


@pytest.mark.parametrize("c", O.ADAM_CASES, ids=O._ids)
def test_adam_grid(c):
    def zero_block(tag, d, out):
        if not c.decoupled and c.wd == 0.0:
            assert _same(out.p[O.ZERO_BLOCK], d.p[O.ZERO_BLOCK]), f"{tag}: p moved where g = m = v = 0"

    _cross("adam", c, 1300 + O.ADAM_CASES.index(c), zero_block)


@pytest.mark.parametrize("c", O.RMS_CASES, ids=O._ids)
def test_rmsprop_grid(c):
    _cross("rms", c, 1400 + O.RMS_CASES.index(c))


GS_INDEX = {"sgd": 4, "adam": 5, "rms": 4}


@_gd
@pytest.mark.parametrize("kind", KINDS)
def test_power_of_two_grad_scale_is_exact(kind, gdtype):
    """g * 2^10 with grad_scale 2^-10 against g with grad_scale 1: a power of two scales exactly
    (|g| in [1e-4, 30] stays normal in bf16 and fp32 either way), so every bit must agree."""
    base = FULL[kind]
    d = O.make_inputs(N_EDGE, 1500, gdtype, zero_block=kind == "adam")
    outs = []
    for gs, mul in ((1.0, 1.0), (2.0 ** -10, 2.0 ** 10)):
        hv = list(base.hv)
        hv[GS_INDEX[kind]] = gs
        dd = _D(d, g=(d.g.float() * mul).to(gdtype))
        assert torch.equal(dd.g.double() * gs, d.g.double())
        outs.append(_launch(kind, dd, _D(base, hv=hv)))
    assert all(_same(outs[0][k], outs[1][k]) for k in outs[0] if k != "g")
    _say(f"{kind} power-of-two grad_scale: identical bits")


# ------------------------------------------------------------------------------- sumsq, scale


def _sumsq(g, out0):
    ext = _ext()
    gw, ow = _Win("g", g.dtype, LO_EDGE, g.numel(), g), _Win("out", F32, 0, 1, torch.tensor([out0]))
    ext.sumsq(gw.ptr, int(g.dtype == BF16), g.numel(), ow.ptr, _st())
    torch.cuda.synchronize()
    assert _same(gw.host(), g), "sumsq wrote its input"
    return ow.host()


@_gd
@pytest.mark.parametrize("n", N_SCALAR)
def test_sumsq_integers_exact(n, gdtype):
    gen = torch.Generator().manual_seed(1600 + n % 997)
    g = torch.randint(-2, 3, (n,), generator=gen).to(gdtype)
    want = 3.0 + g.double().pow(2).sum()
    assert want.item() < 2 ** 24
    got = _sumsq(g, 3.0)
    _say(f"sumsq integers n={n}: {got.item():.0f} (exact {want.item():.0f})")
    assert torch.equal(got.double(), want.reshape(1))


@_gd
@pytest.mark.parametrize("n", [1, 255, 257, 5 * BLOCK - 1])
def test_sumsq_non_integer(n, gdtype):
    d = O.make_inputs(n, 1700 + n, gdtype)
    tot = d.g.double().pow(2).sum().item()
    got = _sumsq(d.g, 0.0).double().item()
    r = abs(got - tot) / (PART_BOUND * tot)
    _say(f"sumsq non-integer n={n}: err / bound {r:.3f} (bound 1)")
    assert math.isfinite(got) and r <= 1.0


@_gd
@pytest.mark.parametrize("k", [0.5, 1.0 / 3.0, 0.0])
@pytest.mark.parametrize("n", N_SCALAR)
def test_scale_is_one_multiply(n, k, gdtype):
    ext = _ext()
    d = O.make_inputs(n, 1800 + n % 997, gdtype)
    kk = torch.tensor([k], dtype=F32)
    want = d.g * kk if gdtype == F32 else (d.g.float() * kk).to(BF16)
    outs = []
    for _ in range(2):
        gw, kw = _Win("g", gdtype, LO_EDGE, n, d.g), kk.to(DEV)
        ext.scale(gw.ptr, int(gdtype == BF16), n, kw.data_ptr(), _st())
        torch.cuda.synchronize()
        outs.append(gw.host())
    assert _same(outs[0], want) and _same(outs[0], outs[1])


# ------------------------------------------------------------------------------- the Python classes


def _model():
    """33 -> 65 -> 7 MLP whose first layer is bf16: one bf16 and one fp32 arena, each with a
    decayed (weight) and a non-decayed (bias) segment and padded slots."""
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(33, 65), torch.nn.Linear(65, 7)).to(DEV)
    m[0].weight.data = m[0].weight.data.to(BF16)
    m[0].bias.data = m[0].bias.data.to(BF16)
    return m


def _lr(step):
    return 0.1 / (1.0 + step)


OPT_KW = {
    "sgd": dict(learning_rate=_lr, momentum=0.9, nesterov=True, dampening=0.25, weight_decay=1e-2, grad_scale=0.5),
    "adam": dict(learning_rate=_lr, weight_decay=1e-3, grad_scale=0.5, epsilon=1e-3),
    "adamw": dict(learning_rate=1e-2, weight_decay=1e-2),
    "rmsprop": dict(learning_rate=_lr, momentum=0.5, weight_decay=1e-3, epsilon=1e-3),
}
OPT_KINDS = sorted(OPT_KW)


def _make(kind, **over):
    from cloud_amd.optim import fused

    o = fused.OPTIMIZERS[kind](_model(), **dict(OPT_KW[kind], **over))
    assert {a.dtype for a in o.arenas} == {BF16, F32}
    assert all(0 < a.n_decay < a.n for a in o.arenas)
    return o


def _expected_hv(kind, kw, t, wd):
    """The hyper-parameters of step ``t`` (1-based) for a segment with weight decay ``wd``, from
    the constructor arguments alone."""
    lr = kw["learning_rate"]
    lr = lr(t) if callable(lr) else lr
    gs = kw.get("grad_scale", 1.0)
    if kind == "sgd":
        return O.hp32([lr, kw["momentum"], kw["dampening"], wd, gs, 1.0 if t == 1 else 0.0])
    if kind in ("adam", "adamw"):
        return O.hp32([lr, O.B1, O.B2, kw.get("epsilon", 1e-7), wd, gs, 1.0 - O.B1 ** t, 1.0 - O.B2 ** t])
    return O.hp32([lr, O.RHO, kw.get("epsilon", 1e-7), wd, gs, kw["momentum"]])


STATE = {"sgd": {"momentum": "m"}, "adam": {"m": "m", "v": "v"}, "adamw": {"m": "m", "v": "v"},
         "rmsprop": {"ms": "ms", "mom": "buf"}}


def _mask(a):
    m = torch.zeros(a.n, dtype=torch.bool)
    for s in a.slots:
        m[s.offset:s.offset + s.numel] = True
    return m


def _snapshot(o):
    """master, model, grad and state of every arena, on the host."""
    return [_D(master=a.master.cpu(), model=None if a.model is None else a.model.cpu(), grad=a.grad.cpu(),
               **{k: v.cpu() for k, v in st.items()}) for a, st in zip(o.arenas, o.state)]


def _fill_grads(o, seed, scale=1.0):
    """Random gradients in the parameters' elements, zeros in the padding."""
    gen = torch.Generator().manual_seed(seed)
    for a in o.arenas:
        g = torch.randn(a.n, generator=gen) * scale * _mask(a)
        a.grad.copy_(g.to(a.grad.dtype))


def _ref_range(kind, kw, t, before, lo, hi, wd):
    """The float64 step of elements [lo, hi) of one arena snapshot."""
    s = slice(lo, hi)
    hv = _expected_hv(kind, kw, t, wd)
    if kind == "sgd":
        return O.sgd64(before.master[s], before.grad[s], before.momentum[s], hv, kw["nesterov"])
    if kind in ("adam", "adamw"):
        return O.adam64(before.master[s], before.grad[s], before.m[s], before.v[s], hv, decoupled=kind == "adamw")
    return O.rms64(before.master[s], before.grad[s], before.ms[s], before.mom[s], hv)


def _check_range(tag, kind, kw, t, before, after, lo, hi, wd):
    ref = _ref_range(kind, kw, t, before, lo, hi, wd)
    got = _D(p=after.master[lo:hi], **{name: after[k][lo:hi] for k, name in STATE[kind].items()})
    return O.check_outputs(tag, got, ref, O._names(ref))


def _check_step(tag, o, kind, kw, t, before, after):
    """Every segment of every arena against the one-step reference from ``before``; padding
    stays exactly 0; the model copy is RNE(master)."""
    worst = {}
    for ai, a in enumerate(o.arenas):
        b, f = before[ai], after[ai]
        for lo, hi, wd in ((0, a.n_decay, kw.get("weight_decay", 0.0)), (a.n_decay, a.n, 0.0)):
            _merge(worst, _check_range(f"{tag} arena {ai} [{lo}, {hi}) wd {wd}", kind, kw, t, b, f, lo, hi, wd))
        pad = ~_mask(a)
        assert pad.any()
        for k in ["master"] + list(STATE[kind]):
            assert not bool(_bits(f[k][pad]).any()), f"{tag}: padding of {k} is not exactly 0"
        if a.model is not None:
            assert _same(f.model, f.master.to(BF16)), f"{tag}: model copy is not RNE(master)"
            assert not bool(_bits(f.model[pad]).any())
    return worst


@pytest.mark.parametrize("kind", OPT_KINDS)
def test_five_steps_each_within_the_one_step_bound(kind):
    kw, o, worst = OPT_KW[kind], _make(kind), {}
    for t in range(1, 6):
        _fill_grads(o, 2000 + t)
        before = _snapshot(o)
        o.step()
        torch.cuda.synchronize()
        assert o.iterations == t
        after = _snapshot(o)
        _merge(worst, _check_step(f"{kind} step {t}", o, kind, kw, t, before, after))
        assert all(not bool(_bits(f.grad).any()) for f in after), "step() left gradient bits behind"
    _say(f"{kind} five steps: worst err / bound", {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("kind", OPT_KINDS)
def test_device_hyper_parameter_path_matches_step(kind):
    """prepare_step() + step_kernels() (no graph capture; ``iterations`` bumped by hand) against
    step() from the same start: the criterion, and identical bits step by step."""
    kw, o, od, worst = OPT_KW[kind], _make(kind), _make(kind), {}
    for t in range(1, 4):
        _fill_grads(o, 2100 + t)
        _fill_grads(od, 2100 + t)
        before = _snapshot(od)
        o.step()
        od.iterations += 1
        od.prepare_step()
        od.step_kernels()
        torch.cuda.synchronize()
        after, want = _snapshot(od), _snapshot(o)
        _merge(worst, _check_step(f"{kind} device-hp step {t}", od, kind, kw, t, before, after))
        for f, w in zip(after, want):
            assert all(_same(f[k], w[k]) for k in f), f"{kind} step {t}: device-hp path differs from step()"
    _say(f"{kind} device hyper-parameters: worst err / bound", {k: round(v, 3) for k, v in worst.items()})


# hand-picked [lo, hi) per arena dtype: inside the decayed segment, straddling n_decay with an odd
# end (the scalar tail through the Python path), and a short one in the non-decayed segment
def _slices(a):
    nd = a.n_decay
    return [(8, 72), (nd - 72, nd + 37)] + ([(nd + 40, nd + 47)] if a.n >= nd + 47 else [])


@pytest.mark.parametrize("kind", OPT_KINDS)
def test_sliced_update_touches_its_range_only(kind):
    kw, o, worst = OPT_KW[kind], _make(kind), {}
    for t in (1, 2):  # the 2nd step: non-zero state, the ``first`` flag cleared
        _fill_grads(o, 2200 + t)
        before = _snapshot(o)
        o.sliced_begin()
        for a in o.arenas:
            for lo, hi in _slices(a):
                o.sliced_update(a, lo, hi)
        o.sliced_end_pending()
        o.step()
        torch.cuda.synchronize()
        assert o.iterations == t
        after = _snapshot(o)
        for ai, a in enumerate(o.arenas):
            b, f = before[ai], after[ai]
            touched = torch.zeros(a.n, dtype=torch.bool)
            for lo, hi in _slices(a):
                assert lo % VEC == 0 and not touched[lo:hi].any()
                touched[lo:hi] = True
                for slo, shi, wd in ((lo, min(hi, a.n_decay), kw.get("weight_decay", 0.0)), (max(lo, a.n_decay), hi, 0.0)):
                    if slo < shi:
                        tag = f"{kind} sliced step {t} arena {ai} [{slo}, {shi}) wd {wd}"
                        _merge(worst, _check_range(tag, kind, kw, t, b, f, slo, shi, wd))
            if a.model is not None:
                assert _same(f.model[touched], f.master[touched].to(BF16))
            assert not bool(_bits(f.grad[touched]).any()), "the slices' gradients were not zeroed"
            for k in f:
                if f[k] is not None:
                    assert _same(f[k][~touched], b[k][~touched]), f"{kind}: {k} changed outside the slices"
    _say(f"{kind} sliced_update: worst err / bound", {k: round(v, 3) for k, v in worst.items()})


def test_fused_zero_grad_contract():
    o = _make("sgd")
    _fill_grads(o, 2300)
    o.step()
    torch.cuda.synchronize()
    assert all(not bool(_bits(a.grad.cpu()).any()) for a in o.arenas), "a native step leaves all-zero gradient bits"
    for a in o.arenas:
        a.grad[5] = 2.0
    o.zero_grad()  # known clean: skips its fill once
    assert all(a.grad[5].item() == 2.0 for a in o.arenas)
    o.zero_grad()
    assert all(not bool(_bits(a.grad.cpu()).any()) for a in o.arenas)

    o = _make("sgd")
    o.fuse_zero_grad = False
    _fill_grads(o, 2301)
    want = [a.grad.cpu() for a in o.arenas]
    o.step()
    torch.cuda.synchronize()
    assert all(_same(a.grad.cpu(), w) for a, w in zip(o.arenas, want)), "step() changed the gradients"
    o.zero_grad()
    assert all(not bool(_bits(a.grad.cpu()).any()) for a in o.arenas)


@pytest.mark.parametrize("above", [False, True], ids=["below", "above"])
@pytest.mark.parametrize("gs", [1.0, 0.5])
def test_clipnorm(gs, above):
    """clipnorm 1 with gradients of norm 3 (above at either grad_scale; the factors 1/3 and 2/3
    round in bf16, where a power of two would not) or 0.8 / grad_scale (below only because the
    norm is taken after grad_scale)."""
    kind = "sgd"
    kw = dict(OPT_KW[kind], grad_scale=gs)
    o = _make(kind, grad_scale=gs, clipnorm=1.0)
    o.fuse_zero_grad = False  # keep the clipped gradients readable after the step
    _fill_grads(o, 2400)
    raw = math.sqrt(sum(a.grad.double().pow(2).sum().item() for a in o.arenas))
    _fill_grads(o, 2400, scale=(3.0 if above else 0.8 / gs) / raw)
    before = _snapshot(o)
    norm = math.sqrt(sum(b.grad.double().pow(2).sum().item() for b in before)) * gs
    if above:
        assert norm > 1.4
    else:
        assert 0.7 < norm < 0.9 and (gs == 1.0 or norm / gs > 1.0)
    o.step()
    torch.cuda.synchronize()
    after, worst = _snapshot(o), 0.0
    for a, b, f in zip(o.arenas, before, after):
        if not above:
            assert _same(f.grad, b.grad), "gradients below the threshold were rescaled"
            continue
        g = b.grad.double()
        ref = g * (1.0 / (norm + 1e-6))
        lim = 2.0 ** -20 * g.abs() + (2.0 ** -8 * ref.abs() if a.dtype == BF16 else 0.0)
        err = (f.grad.double() - ref).abs()
        assert (err[lim == 0] == 0).all(), "padding gradients must stay 0"
        worst = max(worst, (err / lim.clamp_min(1e-300)).max().item())
    _say(f"clipnorm gs={gs} {'above' if above else 'below'}: norm {norm:.3f}, clipped err / bound {worst:.3f}")
    assert worst <= 1.0
    # the update that follows, from the clipped gradients
    clipped = [_D(b, grad=f.grad) for b, f in zip(before, after)]
    w = _check_step(f"clipnorm gs={gs} step", o, kind, kw, 1, clipped, after)
    _say(f"clipnorm gs={gs} {'above' if above else 'below'}: step err / bound", {k: round(v, 3) for k, v in w.items()})
