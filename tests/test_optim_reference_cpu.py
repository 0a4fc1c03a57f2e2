"""Float64 reference, error bound and hyper-parameter grids for the fused optimizer kernels
(csrc/kernels/optim.hip: SgdOp, AdamOp, RmsOp), proved on the CPU: the bound is sound (the
project's own fp32 CPU path meets it) and it discriminates (every named mutant of a rule misses
it by more than 2x on at least 10 % of the elements).  test_optim_kernel_edges_gpu.py imports the
reference, the criterion, the inputs and the grids from here.

Reference.  ``sgd64`` / ``adam64`` / ``rms64`` take the fp32 / bf16 tensors the kernel reads,
converted to float64, and the hyper-parameters as the float32-rounded values the kernel receives
(``hp32``), and compute ONE step in float64 from the update rule.  Every output ``x`` comes with
its absolute-value companion ``Sx``: the same expression with every addend replaced by its
absolute value (sum |term|, as for the statistics partials of the other edge files).

Criterion, per element and per output:   |got - ref| <= PART_BOUND * S,   PART_BOUND = 2^-20
(the project's constant in test_resnet_kernel_edges_gpu.py) = 16 u with u = 2^-24, the unit
roundoff of fp32.  Where S is 0 the output must be exact.  The bf16 model copy must be
bit-identical to ``p_after.to(torch.bfloat16)`` (f2bf is round-to-nearest-even, as torch's cast).

Origin of the bound.  Each kernel performs a fixed number of fp32 operations per element; each
rounds once, by at most u of its own result, and that result is a partial of the expression, so
it is <= S in magnitude.  ``-ffp-contract=fast`` only fuses a multiply into an add, which removes
a rounding.  Division and square root are correctly rounded (no fast-math).  To first order the
error of an expression is then k u S, with k counted by
    k(c) = 0 for an input or a hyper-parameter,   k(a + b) = max(k(a), k(b)) + 1,
    k(a * b) = k(a / b) = k(a) + k(b) + 1,        k(sqrt(a)) = k(a) / 2 + 1;
the distance from the worst count to 16 covers the second-order terms.

    SGD      g' = g gs + wd p                                   k = 2
             m' = mom m + (1 - damp) g'      (first: m' = g')   k = max(1, 1 + 2 + 1) + 1 = 5
             u  = g' + mom m'  (nesterov)    (else u = m')      k = max(2, 6) + 1 = 7
             p' = p - lr u                                      k = 9
    Adam     g' = g gs (+ wd p, coupled)                        k = 1 (2)
             m' = b1 m + (1 - b1) g'                            k = 4 (5)
             v' = b2 v + ((1 - b2) g') g'                       k = 6 (8)
             d  = sqrt(v' / bc2) + eps                          k = 5.5 (6.5)
             w  = (m' / bc1) / d (+ wd p, decoupled)            k = 12.5 (13.5)
             p' = p - lr w                                      k = 14.5 decoupled, 15.5 coupled
    RMSprop  g' = g gs + wd p                                   k = 2
             s' = rho s + ((1 - rho) g') g'                     k = 8
             d  = sqrt(s') + eps                                k = 6
             w  = g' / d                                        k = 9
             b' = mom b + w,   p' = p - lr b'                   k = 10,  k = 12 (11 without mom)

No rule exceeds 16, so all three use PART_BOUND itself.

The denominators.  ``sqrt(v' / bc2) + eps`` and ``sqrt(s') + eps`` are sums of non-negative terms
and enter S as they are -- with one correction, because "non-negative" is not the whole story.
The counts above take the error of the root relative to v' (s') itself.  That is exact with
wd = 0, with decoupled decay and wherever the two addends of g' = g gs + wd p have one sign.
Under coupled decay the addends can cancel: the error of g' stays 2 u Sg while g' shrinks, so its
RELATIVE error is 2 u kg with kg = Sg / |g'| >= 1, and v' inherits it through the share
phi = (1 - b2) g'^2 / v' that the gradient term has in v':
    relative error of v' <= [(1 - phi) + phi (3 + 4 kg) + 1] u <= 8 kappa u,   kappa = 1 + phi (kg - 1).
The root halves it, and the denominator d dilutes it by r = sqrt(x) / d <= 1 (x the argument of
the root), so the companion of the quotient w carries the factor
    K = 1 + (kappa - 1) r,
which keeps the count: Adam 6 + [(4.5 kappa + 1) r + 1] + 1 <= 13.5 K, RMSprop
2 + [(4 kappa + 1) r + 1] + 1 <= 9 K (equal slopes or better in kappa, and true at kappa = 1).
K is exactly 1 wherever the plain reading holds; in the coupled-decay cases below it exceeds 1.01
on a sixth and 2 on 1.4 % of the elements (largest value 40 in a million).  It is needed: without it the project's own
fp32 CPU path reaches 1.12 of the bound on 3 of 4.2 M elements (Adam, coupled wd 1e-2, eps 1e-7,
|g gs| within 10^-3 of |wd p|, tiny v), which is the arithmetic, not a defect; with it that case
is printed by ``test_cpu_path_meets_the_bound_at_the_large_size``.  Nothing here is tuned to a run.

Figures observed (each test prints its own with ``[edges]``; reported, never used to set a bound):

    fp32 CPU path over the grids, err / bound     SGD p 0.16, m 0.11; Adam p 0.26, m 0.12, v 0.23;
                                                  RMSprop p 0.18, ms 0.21, buf 0.19
    the same, Adam coupled at 4.2 M elements      p 0.34, m 0.12, v 0.31 (with K = 1: p 1.12)
    mutants, share of p beyond 2x the bound       dampening, nesterov, first, grad_scale, bias
    (floor 10 %)                                  corrections, momentum buffer: 98.6 - 100 %;
                                                  decay swapped 99.4 %; eps inside the root 97 - 98.5 %;
                                                  wd applied: SGD 100 %, Adam 88 - 97 %, RMSprop 59 %;
                                                  model copy truncated: 49.7 % of the bits differ
"""
import itertools
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_resnet_kernel_edges_gpu as R  # noqa: E402  (PART_BOUND and _say of the conv edge tests)

PART_BOUND, _say = R.PART_BOUND, R._say
BF16, F32 = torch.bfloat16, torch.float32
GDTYPES = [BF16, F32]


class _D(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def hp32(vals):
    """The hyper-parameters as the kernel receives them: rounded to float32, held as floats."""
    return torch.tensor([float(v) for v in vals], dtype=torch.float32).tolist()


# ------------------------------------------------------------------------------- reference

WD_MUTANT = 1e-2  # the weight decay the "wd_applied" mutant uses where 0 was meant


def sgd64(p, g, m, hv, nesterov=False, mutant=None):
    """One SGD step in float64.  hv = hp32([lr, momentum, dampening, wd, grad_scale, first]);
    ``m`` is not read when momentum is 0 or ``first`` is set.  Returns p, Sp, m, Sm."""
    lr, mom, damp, wd, gs, first = hv
    if mutant == "damp_ignored":
        damp = 0.0
    elif mutant == "nesterov_ignored":
        nesterov = False
    elif mutant == "first_ignored":
        first = 0.0
    elif mutant == "wd_applied":
        wd = WD_MUTANT
    elif mutant == "gs_dropped":
        gs = 1.0
    p, g = p.double(), g.double()
    a, b = g * gs, wd * p
    g2, Sg = a + b, a.abs() + b.abs()
    out = _D(m=None, Sm=None)
    u, Su = g2, Sg
    if mom != 0.0:
        if first != 0.0:
            m2, Sm = g2, Sg
        else:
            a, b = mom * m.double(), (1.0 - damp) * g2
            m2, Sm = a + b, a.abs() + abs(1.0 - damp) * Sg
        out.m, out.Sm = m2, Sm
        u, Su = (g2 + mom * m2, Sg + abs(mom) * Sm) if nesterov else (m2, Sm)
    out.p, out.Sp = p - lr * u, p.abs() + abs(lr) * Su
    return out


def _root_factor(g2, Sg, part, whole, root, den):
    """K = 1 + (kappa - 1) root / den, kappa = 1 + phi (Sg / |g'| - 1), phi = part / whole: the
    growth of the root's relative error where g' cancels (module docstring, "The denominators")."""
    kg = torch.where(g2 != 0, Sg / g2.abs().clamp_min(1e-300), torch.ones_like(g2))
    phi = torch.where(whole > 0, part / whole.clamp_min(1e-300), torch.zeros_like(whole))
    return 1.0 + phi * (kg - 1.0) * root / den


def adam64(p, g, m, v, hv, decoupled=False, mutant=None):
    """One Adam / AdamW step in float64.  hv = hp32([lr, b1, b2, eps, wd, grad_scale, bc1, bc2]).
    Returns p, Sp, m, Sm, v, Sv."""
    lr, b1, b2, eps, wd, gs, bc1, bc2 = hv
    if mutant == "decay_swapped":
        decoupled = not decoupled
    elif mutant == "wd_applied":
        wd = WD_MUTANT
    elif mutant == "gs_dropped":
        gs = 1.0
    elif mutant == "bc_swapped":
        bc1, bc2 = bc2, bc1
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    g2 = g * gs
    Sg = g2.abs()
    if not decoupled:
        b = wd * p
        g2, Sg = g2 + b, Sg + b.abs()
    a, b = b1 * m, (1.0 - b1) * g2
    m2, Sm = a + b, a.abs() + abs(1.0 - b1) * Sg
    a, b = b2 * v, (1.0 - b2) * g2 * g2
    v2, Sv = a + b, a.abs() + abs(1.0 - b2) * Sg * Sg
    x = v2 / bc2
    den = (x + eps).sqrt() if mutant == "eps_in_sqrt" else x.sqrt() + eps
    w = (m2 / bc1) / den
    Sw = (Sm / abs(bc1)) / den * _root_factor(g2, Sg, b, v2, x.sqrt(), den)
    if decoupled:
        b = wd * p
        w, Sw = w + b, Sw + b.abs()
    return _D(p=p - lr * w, Sp=p.abs() + abs(lr) * Sw, m=m2, Sm=Sm, v=v2, Sv=Sv)


def rms64(p, g, ms, buf, hv, mutant=None):
    """One RMSprop step in float64.  hv = hp32([lr, rho, eps, wd, grad_scale, momentum]); ``buf``
    is not read when momentum is 0.  Returns p, Sp, ms, Sms, buf, Sbuf."""
    lr, rho, eps, wd, gs, mom = hv
    if mutant == "wd_applied":
        wd = WD_MUTANT
    elif mutant == "gs_dropped":
        gs = 1.0
    p, g, ms = p.double(), g.double(), ms.double()
    a, b = g * gs, wd * p
    g2, Sg = a + b, a.abs() + b.abs()
    a, b = rho * ms, (1.0 - rho) * g2 * g2
    s2, Ss = a + b, a.abs() + abs(1.0 - rho) * Sg * Sg
    den = (s2 + eps).sqrt() if mutant == "eps_in_sqrt" else s2.sqrt() + eps
    w = g2 / den
    Sw = Sg / den * _root_factor(g2, Sg, b, s2, s2.sqrt(), den)
    out = _D(ms=s2, Sms=Ss, buf=None, Sbuf=None)
    if mom != 0.0:
        a = mom * buf.double()
        b2, Sb = a + w, a.abs() + Sw
        out.buf, out.Sbuf = b2, Sb
        if mutant != "buf_ignored":
            w, Sw = b2, Sb
    out.p, out.Sp = p - lr * w, p.abs() + abs(lr) * Sw
    return out


def trunc_bf16(x):
    """The "model copy truncated" mutant: drop the low 16 bits instead of rounding to nearest even."""
    return (x.float().contiguous().view(torch.int32) >> 16).to(torch.int16).view(BF16)


# ------------------------------------------------------------------------------- criterion


def ratio(got, ref, S):
    """max over elements of |got - ref| / (PART_BOUND * S); <= 1 passes.  Elements whose S is 0
    must be exact; every element must be finite (the windows are pre-filled with NaN)."""
    g = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), "unwritten or non-finite elements"
    if g.numel() == 0:
        return 0.0
    err, lim = (g - ref).abs(), PART_BOUND * S
    assert (err[lim == 0] == 0).all(), "elements whose terms are all zero must be exact"
    return (err / lim.clamp_min(1e-300)).max().item()


def violating(got, ref, S, factor=2.0):
    """Fraction of elements with |got - ref| > factor * PART_BOUND * S."""
    return ((got.double() - ref).abs() > factor * PART_BOUND * S).double().mean().item()


def check_outputs(tag, got, ref, names):
    """Criterion for every named output of ``ref`` (a reference result); returns {name: ratio}."""
    worst = {k: ratio(got[k], ref[k], ref["S" + k]) for k in names}
    _say(tag, " ".join(f"{k} {v:.3f}" for k, v in worst.items()), "(bound 1)")
    for k, v in worst.items():
        assert v <= 1.0, (tag, k, v)
    return worst


# ------------------------------------------------------------------------------- inputs

ZERO_BLOCK = slice(512, 576)  # elements with g = m = v = 0 where ``zero_block`` is asked for


def make_inputs(n, seed, gdtype, zero_block=False):
    """The tensors one kernel reads, from a host generator: weights of order 0.5, gradients of
    either sign with magnitudes log-uniform in [1e-4, 30], first moments from 1e-3 to 1, second
    moments log-uniform in [1e-10, 1e-1] (small ones included: the eps placement shows there),
    a momentum buffer of order 0.3.  All non-zero but for the optional zero block."""
    gen = torch.Generator().manual_seed(seed)

    def rnd():
        return torch.rand(n, generator=gen, dtype=torch.float64)

    def sign():
        return torch.where(rnd() < 0.5, -1.0, 1.0)

    d = _D(n=n, gdtype=gdtype)
    d.p = (torch.randn(n, generator=gen, dtype=torch.float64) * 0.5).float()
    d.p = torch.where(d.p == 0, torch.full_like(d.p, 0.25), d.p)
    d.g = (sign() * 10.0 ** (rnd() * (math.log10(30.0) + 4.0) - 4.0)).float().to(gdtype)
    d.m = (sign() * 10.0 ** (rnd() * 3.0 - 3.0)).float()
    d.v = (10.0 ** (rnd() * 9.0 - 10.0)).float()
    d.buf = (sign() * (0.05 + 0.5 * rnd())).float()
    if zero_block and n >= ZERO_BLOCK.stop:
        for k in ("g", "m", "v"):
            d[k][ZERO_BLOCK] = 0
    return d


# ------------------------------------------------------------------------------- grids
# One entry per line of SgdOp / AdamOp / RmsOp; the GPU edge file runs the same grids.

LR = {"sgd": 0.1, "adam": 1e-2, "rms": 1e-2}
B1, B2, RHO = 0.9, 0.999, 0.9


def _sgd_case(mom, first, m, damp, nesterov, wd, gs):
    name = f"mom{mom}-first{first}-m_{m}-damp{damp}-nest{int(nesterov)}-wd{wd}-gs{gs}"
    return _D(name=name, mom=mom, first=first, m=m, damp=damp, nesterov=nesterov, wd=wd, gs=gs,
              hv=hp32([LR["sgd"], mom, damp, wd, gs, first]))


# m: "null" (pointer 0), "nan" (window left at the NaN sentinel: ``first`` must not read it), "rand"
SGD_CASES = [
    _sgd_case(0.0, 0, "null", 0.0, False, 0.0, 1.0),
    _sgd_case(0.0, 0, "null", 0.0, False, 1e-2, 0.5),
    _sgd_case(0.9, 1, "nan", 0.0, False, 1e-2, 0.5),
    _sgd_case(0.9, 1, "nan", 0.25, True, 0.0, 1.0),
    _sgd_case(0.9, 0, "rand", 0.0, False, 0.0, 1.0),
    _sgd_case(0.9, 0, "rand", 0.25, False, 1e-2, 0.5),
    _sgd_case(0.9, 0, "rand", 0.0, True, 1e-2, 1.0),
    _sgd_case(0.9, 0, "rand", 0.25, True, 0.0, 0.5),
    _sgd_case(0.9, 0, "rand", 0.25, True, 1e-2, 0.5),
]


def adam_hv(eps, wd, gs, t):
    return hp32([LR["adam"], B1, B2, eps, wd, gs, 1.0 - B1 ** t, 1.0 - B2 ** t])


ADAM_CASES = [
    _D(name=f"{'decoupled' if dec else 'coupled'}-wd{wd}-eps{eps}-t{t}-gs{gs}", decoupled=dec, wd=wd, eps=eps, t=t,
       gs=gs, hv=adam_hv(eps, wd, gs, t))
    for dec, wd, (eps, gs), t in itertools.product([False, True], [0.0, 1e-2], [(1e-7, 1.0), (1e-3, 0.5)], [1, 1000])
]

RMS_CASES = [
    _D(name=f"mom{mom}-wd{wd}-gs{gs}", mom=mom, wd=wd, gs=gs, eps=eps, hv=hp32([LR["rms"], RHO, eps, wd, gs, mom]))
    for mom, wd, (gs, eps) in itertools.product([0.0, 0.5], [0.0, 1e-3], [(1.0, 1e-7), (0.5, 1e-3)])
]

_ids = lambda c: c.name  # noqa: E731


def sgd_ref(d, c, mutant=None):
    return sgd64(d.p, d.g, d.m, c.hv, c.nesterov, mutant=mutant)


def adam_ref(d, c, mutant=None):
    return adam64(d.p, d.g, d.m, d.v, c.hv, c.decoupled, mutant=mutant)


def rms_ref(d, c, mutant=None):
    return rms64(d.p, d.g, d.v, d.buf, c.hv, mutant=mutant)


# ------------------------------------------------------------------------------- soundness
# The project's fp32 CPU path (FusedOptimizer._update on "cpu") performs the same operations in
# the same order as the kernels, each rounded once: it must meet the criterion.

N_CPU = 4096


def _cpu_step(kind, d, c):
    """One ``_update`` of the CPU path over the inputs ``d``; returns the outputs by name."""
    from cloud_amd import optim

    prm = torch.nn.Parameter(torch.zeros(d.n, dtype=d.gdtype))
    if kind == "sgd":
        o = optim.SGD([prm], momentum=c.mom, nesterov=c.nesterov, dampening=c.damp)
        state = {"momentum": "m"}
    elif kind == "adam":
        o = (optim.AdamW if c.decoupled else optim.Adam)([prm])
        state = {"m": "m", "v": "v"}
    else:
        o = optim.RMSprop([prm], momentum=c.mom)
        state = {"ms": "v", "mom": "buf"}
    a, st = o.arenas[0], o.state[0]
    assert a.n == d.n
    a.master.copy_(d.p)
    a.grad.copy_(d.g)
    for k, src in state.items():
        if k in st:
            st[k].copy_(d[src])
    if kind == "sgd" and c.m == "nan":
        st["momentum"].fill_(float("nan"))
    o._update(0, a, 0, d.n, torch.tensor(c.hv, dtype=torch.float32), None)
    got = _D(p=a.master, model=a.model)
    for k, name in (("momentum", "m"), ("m", "m"), ("v", "v"), ("ms", "ms"), ("mom", "buf")):
        if k in st:
            got[name] = st[k]
    return got


def _names(ref):
    return [k for k in ("p", "m", "v", "ms", "buf") if ref.get(k) is not None]


@pytest.mark.parametrize("gdtype", GDTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind,cases,ref_fn", [("sgd", SGD_CASES, sgd_ref), ("adam", ADAM_CASES, adam_ref),
                                               ("rms", RMS_CASES, rms_ref)], ids=["sgd", "adam+adamw", "rmsprop"])
def test_cpu_path_meets_the_bound(kind, cases, ref_fn, gdtype):
    worst = {}
    for i, c in enumerate(cases):
        d = make_inputs(N_CPU, 100 + i, gdtype, zero_block=kind == "adam")
        ref = ref_fn(d, c)
        got = _cpu_step(kind, d, c)
        for k, v in check_outputs(f"cpu {kind} {c.name}", got, ref, _names(ref)).items():
            worst[k] = max(worst.get(k, 0.0), v)
        if got.model is not None:
            assert torch.equal(got.model.view(torch.int16), got.p.to(BF16).view(torch.int16))
    _say(f"cpu path {kind}: worst err / bound", {k: round(v, 3) for k, v in worst.items()})


N_LARGE = 2048 * 256 * 8 + 64 * 97  # past one grid-stride trip of the vector kernels, a multiple of the arena's 64


@pytest.mark.parametrize("gdtype", GDTYPES, ids=["bf16", "fp32"])
def test_cpu_path_meets_the_bound_at_the_large_size(gdtype):
    """Adam with coupled decay and eps 1e-7 at 4.2 M elements: the case with the closest
    cancellations of g gs + wd p under the smallest denominators.  Also prints the figure that
    the plain reading of the denominators (K = 1) would give; that one is not asserted."""
    c = _case(ADAM_CASES, decoupled=False, wd=1e-2, eps=1e-7, t=1000)
    d = make_inputs(N_LARGE, 900, gdtype, zero_block=True)
    ref = adam_ref(d, c)
    got = _cpu_step("adam", d, c)
    check_outputs(f"cpu adam {c.name} n={N_LARGE}", got, ref, _names(ref))
    lr, _, _, eps, _, _, bc1, bc2 = c.hv
    plain = d.p.double().abs() + lr * (ref.Sm / bc1) / ((ref.v / bc2).sqrt() + eps)
    _say(f"  with K = 1 instead: p {((got.p.double() - ref.p).abs() / (PART_BOUND * plain)).max().item():.3f}")


def test_adam_zero_block_is_a_fixed_point_or_pure_decay():
    """g = m = v = 0: coupled with wd 0 leaves p as it is; decoupled gives p - lr wd p."""
    d = make_inputs(N_CPU, 7, F32, zero_block=True)
    c = next(c for c in ADAM_CASES if not c.decoupled and c.wd == 0.0)
    ref = adam_ref(d, c)
    assert torch.equal(ref.p[ZERO_BLOCK], d.p.double()[ZERO_BLOCK])
    c = next(c for c in ADAM_CASES if c.decoupled and c.wd != 0.0)
    ref = adam_ref(d, c)
    lr, wd = c.hv[0], c.hv[4]
    pz = d.p.double()[ZERO_BLOCK]
    assert torch.equal(ref.p[ZERO_BLOCK], pz - lr * (wd * pz))


# ------------------------------------------------------------------------------- discrimination
# Each mutant is one plausible one-line defect of a kernel.  It is judged on p, the output every
# defect must reach to matter, at the grid case where the line it breaks is live.

FLOOR = 0.10  # a floor against a mutant passing on a handful of lucky elements, not a measurement


def _case(cases, **want):
    return next(c for c in cases if all(c[k] == v for k, v in want.items()))


MUTANTS = [
    ("sgd", "damp_ignored", dict(m="rand", damp=0.25, nesterov=False)),
    ("sgd", "nesterov_ignored", dict(m="rand", nesterov=True, damp=0.0)),
    ("sgd", "first_ignored", dict(first=1, nesterov=False)),
    ("sgd", "wd_applied", dict(m="rand", wd=0.0, nesterov=False)),
    ("sgd", "gs_dropped", dict(m="rand", gs=0.5, nesterov=False)),
    ("adam", "decay_swapped", dict(decoupled=False, wd=1e-2, eps=1e-7, t=1000)),
    ("adam", "decay_swapped", dict(decoupled=True, wd=1e-2, eps=1e-7, t=1000)),
    ("adam", "wd_applied", dict(decoupled=False, wd=0.0, eps=1e-7, t=1000)),
    ("adam", "wd_applied", dict(decoupled=True, wd=0.0, eps=1e-7, t=1000)),
    ("adam", "gs_dropped", dict(decoupled=False, wd=0.0, eps=1e-3, t=1000)),
    ("adam", "bc_swapped", dict(decoupled=False, wd=0.0, eps=1e-7, t=1)),
    ("adam", "bc_swapped", dict(decoupled=False, wd=0.0, eps=1e-7, t=1000)),
    ("adam", "eps_in_sqrt", dict(decoupled=False, wd=0.0, eps=1e-3, t=1000)),
    ("rms", "wd_applied", dict(mom=0.5, wd=0.0, gs=1.0)),
    ("rms", "gs_dropped", dict(mom=0.0, wd=0.0, gs=0.5)),
    ("rms", "eps_in_sqrt", dict(mom=0.0, wd=0.0, eps=1e-3)),
    ("rms", "buf_ignored", dict(mom=0.5, wd=0.0, gs=1.0)),
]
_KIND = {"sgd": (SGD_CASES, sgd_ref), "adam": (ADAM_CASES, adam_ref), "rms": (RMS_CASES, rms_ref)}


@pytest.mark.parametrize("gdtype", GDTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind,mutant,want", MUTANTS, ids=[f"{k}-{m}-{i}" for i, (k, m, _) in enumerate(MUTANTS)])
def test_mutant_is_rejected(kind, mutant, want, gdtype):
    cases, ref_fn = _KIND[kind]
    c = _case(cases, **want)
    d = make_inputs(N_CPU, 300, gdtype)
    if kind == "sgd" and c.m == "nan":  # the mutant reads the old momentum: give it one to read
        c = _D(c, m="rand")
    ref, mut = ref_fn(d, c), ref_fn(d, c, mutant=mutant)
    frac = violating(mut.p, ref.p, ref.Sp)
    _say(f"mutant {kind} {mutant} [{c.name}]: {100 * frac:.1f} % of p beyond 2x the bound (floor 10 %)")
    assert frac >= FLOOR, (kind, mutant, frac)
    # and the float32 rounding of the mutant's result is as far off (what a wrong kernel would store)
    assert violating(mut.p.float(), ref.p, ref.Sp) >= FLOOR


def test_truncated_model_copy_is_rejected():
    """The model copy is compared bit for bit: truncation differs wherever the dropped half is
    above its midpoint (or at it with an even result), about half of all elements."""
    d = make_inputs(N_CPU, 301, F32)
    ref = sgd_ref(d, SGD_CASES[0])
    p_after = ref.p.float()
    rne, cut = p_after.to(BF16), trunc_bf16(p_after)
    frac = (rne.view(torch.int16) != cut.view(torch.int16)).double().mean().item()
    _say(f"mutant model copy truncated: {100 * frac:.1f} % of elements differ in bits (floor 10 %)")
    assert frac >= FLOOR


def test_reference_formulas_by_hand():
    """The rules on one element, written out with plain Python floats."""
    p, g, m, v = 0.5, -2.0, 0.25, 0.04
    t = lambda x: torch.tensor([x], dtype=torch.float64)  # noqa: E731
    lr, mom, damp, wd, gs, first = hv = [0.1, 0.5, 0.25, 0.125, 0.5, 0.0]
    r = sgd64(t(p), t(g), t(m), hv, nesterov=True)
    g2 = g * gs + wd * p
    m2 = mom * m + (1 - damp) * g2
    assert r.m.item() == m2 and r.p.item() == p - lr * (g2 + mom * m2)
    assert r.Sp.item() == abs(p) + lr * (abs(g * gs) + abs(wd * p) + mom * (abs(mom * m) + (1 - damp) * (abs(g * gs) + abs(wd * p))))
    r = sgd64(t(p), t(g), t(float("nan")), [lr, mom, damp, wd, gs, 1.0], nesterov=False)
    assert r.m.item() == g2 and r.p.item() == p - lr * g2
    lr, b1, b2, eps, wd, gs, bc1, bc2 = hv = [0.01, 0.5, 0.75, 0.001, 0.125, 0.5, 0.5, 0.25]
    r = adam64(t(p), t(g), t(m), t(v), hv, decoupled=True)
    g2 = g * gs
    m2, v2 = b1 * m + (1 - b1) * g2, b2 * v + (1 - b2) * g2 * g2
    assert r.m.item() == m2 and r.v.item() == v2
    assert r.p.item() == p - lr * ((m2 / bc1) / (math.sqrt(v2 / bc2) + eps) + wd * p)
    r = adam64(t(p), t(g), t(m), t(v), hv, decoupled=False)
    g2 = g * gs + wd * p
    m2, v2 = b1 * m + (1 - b1) * g2, b2 * v + (1 - b2) * g2 * g2
    assert r.p.item() == p - lr * ((m2 / bc1) / (math.sqrt(v2 / bc2) + eps))
    lr, rho, eps, wd, gs, mom = hv = [0.01, 0.75, 0.001, 0.125, 0.5, 0.5]
    r = rms64(t(p), t(g), t(v), t(m), hv)
    s2 = rho * v + (1 - rho) * g2 * g2
    b2_ = mom * m + g2 / (math.sqrt(s2) + eps)
    assert r.ms.item() == s2 and r.buf.item() == b2_ and r.p.item() == p - lr * b2_
