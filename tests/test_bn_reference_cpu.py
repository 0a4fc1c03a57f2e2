"""Float64 references, criteria, tiling model, inputs and case lists for the training BatchNorm
kernels (csrc/kernels/bn.hip) and the global pools (csrc/kernels/pool.hip: gap_fwd / gap_bwd /
gmp_fwd / gmp_bwd), proved on the CPU: every criterion is sound (an fp32 emulation of the kernels'
summation order and the project's torch path ``_torch_bn_act`` meet it on every case) and it
discriminates (every named mutant misses it on the case built for it).
test_bn_kernel_edges_gpu.py imports the references, the criteria, the inputs and the cases from here.

References.  Each takes exactly the bf16 / fp32 tensors the kernel reads, converted to float64, and
returns every output with its absolute-value companion S (the same expression with every addend
replaced by its absolute value):
    stats64     two-pass mean, biased var, rstd = 1 / sqrt(var + float32(eps)), scale = gamma rstd,
                shift = beta - mean scale
    running64   run' = (1 - mom) run + mom new, new = mean / the UNBIASED var (at M = 1 the
                kernel's documented choice: unb = var)
    apply64     x scale + shift [+ res];  resbn64: x scale + shift + bf16(r rscale + rshift)
    bwd64       dz = gate dy, dbeta = sum dz, dgamma = sum dz xhat, A = gamma rstd,
                B = -A (dgamma / M) rstd, D = -A dbeta / M - B mean;  dx64: A dz + B x + D;  dres = dz
    gap64 / gap_bwd64, gmp64 / gmp_bwd64: ties share evenly, +0.0 and -0.0 are one value.
They are cross-checked once against torch float64 autograd (F.batch_norm, mean, amax) at M >= 2.

Tiling model.  ``make_tiling`` ports bn.hip's make_tiling, ``trip_counts`` the per-thread loop
trips.  Every case carries the predicate of the branch it is named for (``CASES``); a retuned
tiling that stops reaching the branch fails ``test_case_reaches_its_branch``.

Criteria (derived, none tuned to a run; u = 2^-24).

  elementwise (y, dx, shortcut form): against the float64 expression evaluated with the kernel's
  OWN fp32 coefficients (stats[2C:4C], coef[3C]): |got - ref| <= 2^-8 |ref| + 2^-21 S, the derived
  bound of test_bn_fold_edges_gpu.py (two FMAs and an add on terms of total magnitude S, then one
  bf16 rounding).  An element with |pre| <= 2^-21 S may gate either way: there the mask and the
  backward follow the kernel's bit; every other bit, and bit == (y > 0) everywhere, is exact.  The
  share of such elements is capped at 0.1 % per case.
  Shortcut form: the reference rounds idn = r rscale + rshift to bf16 as the kernel does, and the
  bound adds 2^-8 |idn|.  Where idn lies within 2^-21 S_idn of a bf16 rounding midpoint, fp32 and
  float64 may round to different neighbours; such an element is judged against the nearer of the
  two.  That bound CANNOT see a kernel that skips the rounding (the skipped rounding is at most
  half an ulp of idn = the allowance), so the form is also held bit for bit to the op-by-op path
  (the shortcut BN's stored bf16 output fed as a plain residual) -- the property bn.hip states
  for it; the "not rounded" mutant is judged by that.

  statistics, random values: the criterion of test_bn_statistics_with_large_mean, per channel
  max(4 x the error of a plain fp32 one-pass on the same input, 1e-5), against the float64
  two-pass values: bm for |mean - ref| / max(|ref|, sd), br for |rstd / ref - 1|.  scale = gamma
  rstd inherits br.  shift = beta - mean scale: |err| <= (bm + br) (|beta| + max(|mean|, sd)
  |scale|) (product rule; the three fp32 roundings are 3 u, far below the 1e-5 floor).  Running
  mean: mom bm max(|mean|, sd) + 4 u S.  Running var: rstd = (var + eps)^-1/2 gives
  d var = 2 (var + eps) d rstd / rstd, so mom 2 br (var + eps) M / (M - 1) + 4 u S.

  dgamma / dbeta, random values: gamma_k S with gamma_k = k u / (1 - k u) and k the COUNTED longest
  chain of fp32 additions a term passes through for the case's tiling (K = rows_per_chunk / RP
  trips per thread, T2 = K // 2 two-row trips, K % 2 tail trips):
      dbeta   k = [T2 > 0] (the pair add) + T2 + K % 2 (adds into the thread's sum)
                  + RP (block_col_reduce, sequential) + 1 (the fp32 store)
      dgamma  k = the same + 3 (x - mean, * dz, * rstd round once each, relative to the term)
      accumulate: + 1, and S grows by |old|.  The chunk combine is in double and adds nothing.
  k per case: 1x8 258 / 261, 1x64 34 / 37, 255x8 and 257x8 258 / 261, 200x24 87 / 90, 131x40 53 / 56,
  90x72 30 / 33, 300x512 6 / 9, 16641x8 258 / 261, 77x520 and 77x1032 6 / 9, 234x64 34 / 37, 6272x256
  10 / 13 (dbeta / dgamma).  At C = 8, RP is 256 and the bound is loose: the geometry coverage rests on
  the exact-integer cases, not on it.  ``partials=`` (raw moments [sum dz | sum dz x] per 128-row
  tile, each rounded once to fp32): k = 2, or 2 + rows-per-lane + 16 through group_finalize_kernel,
  on S' = rstd (sum |dz x| + |mean| sum |dz|) for dgamma, which carries the cancellation of
  rstd (sum dz x - mean sum dz).
  B and D propagate it: eB = |A rstd / M| gamma_k S_dgamma + 2 u |B|,
  eD = |A / M| gamma_k S_dbeta + |mean| eB + 2 u (|A dbeta / M| + |B mean|), eA = 2 u |A|.

  exact-integer cases (the geometry pins): x, dy, res in {-2 .. 2}, mean an integer, rstd a power of
  two, planted mask bits.  Every fp32 partial sum is an integer or a multiple of 0.5 below 2^24
  (asserted), so any summation order is exact: the forward sums, dbeta and dgamma must EQUAL the
  float64 sums; mean, rstd and the coefficients hold to 2^-22 of their S (one fp32 rounding of a
  double result plus libm differences).

  global pools: gap_fwd  HW u S + 2 u |ref| (HW sequential adds of terms of total S = sum |x| / HW,
  one multiply by the rounded 1.f / HW) + 2^-8 |ref| for a bf16 output; integer inputs: bit-exact
  float32(sum) * float32(1 / HW).  gap_bwd 2 u |ref| + 2^-8 |ref|.  gmp_fwd: values and counts
  exact.  gmp_bwd: 2^-8 |ref| per element, non-maximum positions exactly 0.  Sum of dx over HW
  against dy: the cnt shares are EQUAL bf16 roundings of dy / cnt, each off by up to 2^-8 |dy| /
  cnt, so the sum is within 2^-8 |dy|.  (HW 2^-9 |dy| / cnt is not a bound where cnt > HW / 2: a
  whole-channel tie, or HW = 1 with an fp32 dy, rounds by up to 2^-8 relative --
  ``test_gmp_share_sum_bound_on_paper`` shows a correctly rounded share beyond it.  Where
  cnt <= HW / 2 it is the looser of the two, so 2^-8 |dy| asks more there.)

Figures observed (each test prints its own with ``[edges]``; reported, never used to set a bound):

    fp32 emulation, elementwise err / bound          y 0.996, shortcut form 0.960, dx 0.996
    torch path y err / bound                         0.996
    emulation statistics err / bound (random cases)  mean 0.006, rstd 0.17, scale 0.13, shift 0.06
    emulation running mean / var                     0.18 / 0.31 (exact cases, 2^-22: 0.50 / 0.43)
    emulation dgamma / dbeta; A / B / D              0.16 / 0.09; 0.49 / 0.10 / 0.08 of their bounds
    raw-moment partials dgamma / dbeta               0.12 / 0.08
    near-zero share, worst random case               1.9e-4 (131x40: 1 of 5240; cap 1e-3)
    pools: gap 0.996, gap_bwd 0.995, gmp_bwd per element and share sums 0.995
    mutants, err / bound: a dropped row 1.9e3 - 1.8e4, the ragged rows 4.3e4, gate ignored / from
    y >= 0 1.6e5 (B), D sign / B mean left out 3.2e5 / 1.6e5, unbiased rstd 214, biased running
    var 202, momentum swapped 2.6e6, ties not shared 1.1e4, bit compare 256 per element / 85 on
    the share sum, HW + 1 beyond 1; on the exact cases every sum mutant breaks equality; the
    unrounded shortcut value differs from the op-by-op path in 13.8 % of the elements (and sits
    at 0.88 of the derived bound, which is why that bound is not its judge)
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_resnet_kernel_edges_gpu as R  # noqa: E402  (_relu_bits and _say of the conv edge tests)

_relu_bits, _say = R._relu_bits, R._say
BF16, F32 = torch.bfloat16, torch.float32
U = 2.0 ** -24
EPS, MOM = 1e-5, 0.1
EXACT_REL = 2.0 ** -22
NEAR_ZERO_CAP = 1e-3


class _D(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def f32(v):
    """A Python float rounded to float32 (the value a kernel receives for a float argument)."""
    return torch.tensor(float(v), dtype=F32).item()


# ------------------------------------------------------------------------------- tiling model

BLK = 256


def make_tiling(M, C, total=2048, cap=1024):
    """bn.hip make_tiling: a block is TW column vectors x RP rows; [nchunks] row chunks of
    rows_per_chunk (a multiple of RP) x [ncol] column blocks."""
    CT = C // 8
    TW = min(CT, 64)
    RP = BLK // TW
    ncol = -(-CT // TW)
    want = min(max(total // ncol, 1), -(-M // RP), cap)
    rpc = -(-(-(-M // want)) // RP) * RP
    return _D(CT=CT, TW=TW, RP=RP, ncol=ncol, nchunks=-(-M // rpc), rpc=rpc)


def thread_rows(t, M, chunk):
    """Rows walked by the threads ty = 0 .. RP of a reduction block of ``chunk`` (index RP is the
    stray row group that exists when 256 % TW != 0; block_col_reduce drops its sums)."""
    n = min(t.rpc, M - chunk * t.rpc)
    ty = torch.arange(t.RP + 1)
    return ((n - ty + t.RP - 1) // t.RP).clamp_min(0)


def trip_counts(t, M):
    """Per-thread loop trips: thread ty = 0 of chunk 0 (the longest), of the last chunk, and the
    stray thread's rows; trips of the interleaved apply loop."""
    first, last = thread_rows(t, M, 0), thread_rows(t, M, t.nchunks - 1)
    n0, nl = int(first[0]), int(last[0])
    return _D(stats4=n0 // 4, stats_tail=n0 % 4, bwd2=n0 // 2, bwd_tail=n0 % 2,
              last_rows=M - (t.nchunks - 1) * t.rpc, last_stats4=nl // 4, last_bwd2=nl // 2,
              stray=(BLK % t.TW != 0), stray_threads=BLK - t.TW * t.RP, stray_rows=int(first[t.RP]),
              apply_trips=-(-M // (t.nchunks * t.RP)))


def chain_k(M, C, what, accumulate=False):
    """The counted longest chain of fp32 additions of the backward reduction (module docstring)."""
    t = make_tiling(M, C)
    K = t.rpc // t.RP
    k = (1 if K // 2 else 0) + K // 2 + K % 2 + t.RP + 1
    return k + (3 if what == "dgamma" else 0) + (1 if accumulate else 0)


def partials_k(nparts, rpg=512):
    """Chain of the ``partials=`` path: one fp32 rounding per partial, the fp32 group sums of
    group_finalize_kernel when there are more than 64 rows (16 lanes x rows-per-lane, then 16),
    the fp32 store."""
    return 2 + ((-(-min(nparts, rpg) // 16) + 16) if nparts > 64 else 0)


def gamma_k(k):
    return k * U / (1.0 - k * U)


def _case(M, C, data, why, reaches):
    return _D(name=f"{M}x{C}", M=M, C=C, data=data, why=why, reaches=reaches)


# data: "random" (numerics + geometry), "integer" (exact sums only)
CASES = [
    _case(1, 8, "random", "M = 1 at RP = 256: var 0, no unbiased correction, one row below RP",
          lambda t, n: t.RP == 256 and t.nchunks == 1 and n.last_rows == 1),
    _case(1, 64, "random", "M = 1 at RP = 32", lambda t, n: t.RP == 32 and t.nchunks == 1 and n.last_rows == 1),
    _case(255, 8, "random", "RP = 256: one short chunk",
          lambda t, n: t.RP == 256 and t.nchunks == 1 and n.last_rows == 255),
    _case(257, 8, "random", "RP = 256: two chunks, the second with one row",
          lambda t, n: t.RP == 256 and t.nchunks == 2 and n.last_rows == 1),
    _case(200, 24, "random", "256 % TW != 0 (RP = 85), ragged last chunk; the stray thread walks the next block's row",
          lambda t, n: n.stray and t.RP == 85 and 0 < n.last_rows < t.RP and t.nchunks > 1),
    _case(131, 40, "random", "256 % TW != 0 (RP = 51), ragged last chunk",
          lambda t, n: n.stray and t.RP == 51 and 0 < n.last_rows < t.RP and t.nchunks > 1),
    _case(90, 72, "random", "256 % TW != 0 (RP = 28, four stray threads), ragged last chunk",
          lambda t, n: n.stray and t.RP == 28 and n.stray_threads == 4 and 0 < n.last_rows < t.RP),
    _case(87041, 24, "integer", "256 % TW != 0 and rows_per_chunk = 2 RP: the stray thread has rows to walk; 513 "
          "chunks; the apply passes take a second interleaved trip",
          lambda t, n: n.stray and t.rpc == 2 * t.RP and n.stray_rows >= 1 and t.nchunks == 513 and n.bwd2 == 1
          and n.apply_trips >= 2 and n.last_rows == 1),
    _case(300, 512, "random", "TW = 64, RP = 4, 75 chunks > 64: group_finalize_kernel from the tail of ws; second "
          "wave_chunk_sum trip", lambda t, n: t.TW == 64 and t.RP == 4 and t.nchunks == 75),
    _case(16641, 8, "random", "66 chunks at RP = 256, one row in the last",
          lambda t, n: t.RP == 256 and t.nchunks == 66 and n.last_rows == 1),
    _case(77, 520, "random", "ncol = 2 with one live column in block 1",
          lambda t, n: t.ncol == 2 and t.CT - t.TW == 1 and n.last_rows < t.RP),
    _case(77, 1032, "random", "ncol = 3 with one live column in block 2",
          lambda t, n: t.ncol == 3 and t.CT - 2 * t.TW == 1 and n.last_rows < t.RP),
    _case(16389, 512, "integer", "rows_per_chunk = 5 RP: the 4-row and 2-row unrolled loops and their tails; 9 rows "
          "in the last of 820 chunks; five interleaved apply trips",
          lambda t, n: t.rpc == 5 * t.RP == 20 and n.stats4 == 1 and n.stats_tail == 1 and n.bwd2 == 2
          and n.bwd_tail == 1 and t.nchunks == 820 and n.last_rows == 9 and n.last_stats4 == 0 and n.last_bwd2 == 1
          and n.apply_trips >= 2),
    _case(234, 64, "random", "numerics: the large-mean channel groups", lambda t, n: t.RP == 32 and t.nchunks == 8),
    _case(6272, 256, "random", "numerics at a production shape: 784 chunks",
          lambda t, n: t.nchunks == 784 and t.rpc == t.RP == 8),
]
CASE = {c.name: c for c in CASES}
_ids = lambda c: c.name  # noqa: E731
RANDOM_CASES = [c for c in CASES if c.data == "random"]
SHORTCUT_CASES = [CASE["200x24"], CASE["300x512"], CASE["77x520"]]  # shortcut-BN form and statistics-only
INFER_CASES = [CASE["131x40"], CASE["77x1032"]]
CHILD_CASES = ["200x24", "300x512", "87041x24"]


def reduced(c):
    """The exact-integer cases are the large ones: they run a reduced combination matrix."""
    return c.data == "integer"


@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_case_reaches_its_branch(c):
    t = make_tiling(c.M, c.C)
    n = trip_counts(t, c.M)
    _say(f"tiling {c.name}: {dict(t)} {dict(n)}")
    assert c.reaches(t, n), (c.name, c.why, dict(t), dict(n))
    assert t.rpc % t.RP == 0 and (t.nchunks - 1) * t.rpc < c.M <= t.nchunks * t.rpc
    assert 2 * t.nchunks * c.C + 2 * 64 * c.C >= 2 * t.nchunks * c.C + 2 * 16 * c.C  # group rows fit the ws tail


# ------------------------------------------------------------------------------- inputs

BN_MEANS, BN_SPREADS = R.BN_MEANS, R.BN_SPREADS
CH_GAMMA0, CH_CONST, CH_MEAN128 = 0, 1, 2  # planted channels


@functools.lru_cache(maxsize=4)
def bn_data(M, C, kind):
    """Host operands of a case (never modified).  random: x = mean_c + spread_c N(0, 1) with
    channel means of order 1; channel 0 has gamma = beta = 0, channel 1 is constant, channel 2 has
    mean 128 and spread 0.25; the numerics cases 234x64 and 6272x256 lay the (mean, spread) groups
    of test_bn_statistics_with_large_mean over channels 8 and up.  integer: x, res, r, dy in
    {-2 .. 2}, a planted gate, an integer mean and a power-of-two rstd for the backward."""
    g = torch.Generator().manual_seed(611953 + 7919 * M + 31 * C + (kind == "integer"))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    d = _D(M=M, C=C, kind=kind)
    if kind == "integer":
        ri = lambda *s: torch.randint(-2, 3, s, generator=g).float()  # noqa: E731
        d.x, d.res, d.r, d.dy = ri(M, C).to(BF16), ri(M, C).to(BF16), ri(M, C).to(BF16), ri(M, C).to(BF16)
        d.x[:, CH_CONST] = 1.0
    else:
        mvec, svec = rn(C), 0.5 + torch.rand(C, generator=g)
        if (M, C) in ((234, 64), (6272, 256)):
            groups = [(m, s) for m in BN_MEANS for s in BN_SPREADS]
            idx = torch.arange(C - 8) % len(groups)
            mvec[8:] = torch.tensor([m for m, _ in groups])[idx]
            svec[8:] = torch.tensor([s for _, s in groups])[idx]
        mvec[CH_MEAN128], svec[CH_MEAN128] = 128.0, 0.25
        d.x = (mvec + svec * rn(M, C)).to(BF16)
        d.x[:, CH_CONST] = 0.75
        d.res, d.r, d.dy = rn(M, C).to(BF16), rn(M, C).to(BF16), rn(M, C).to(BF16)
    d.gamma = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)
    d.beta = 0.5 * rn(C)
    d.gamma[CH_GAMMA0], d.beta[CH_GAMMA0] = 0.0, 0.0
    d.rm, d.rv = rn(C), 0.5 + torch.rand(C, generator=g)
    d.rss = torch.cat([0.5 + torch.rand(C, generator=g), 0.5 * rn(C)])  # the shortcut BN's [scale | shift]
    d.old_dgamma, d.old_dbeta = rn(C), rn(C)
    # the backward of the exact cases: planted gate, integer mean, power-of-two rstd
    d.keep = torch.rand(M, C, generator=g) > 0.4
    d.y_planted = d.keep.to(BF16)
    d.mean_i = torch.randint(-1, 2, (C,), generator=g).float()
    d.rstd_p = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    return d


def planted_stats(d):
    """stats[4C] of an exact backward: integer mean, power-of-two rstd (scale / shift unused)."""
    return torch.cat([d.mean_i, d.rstd_p, torch.zeros(2 * d.C)])


# ------------------------------------------------------------------------------- references


def stats64(x, gamma, beta, eps=EPS, mutant=None):
    xd = x.double()
    M, C = xd.shape
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    unb = var * M / (M - 1) if M > 1 else var
    rstd = 1.0 / torch.sqrt((unb if mutant == "unbiased_rstd" else var) + f32(eps))
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    b = beta.double() if beta is not None else torch.zeros(C, dtype=torch.float64)
    scale = g * rstd
    return _D(M=M, mean=mean, var=var, unb=unb, sd=var.sqrt(), rstd=rstd, scale=scale, shift=b - mean * scale,
              beta=b, sum=xd.sum(0), sumsq=(xd * xd).sum(0), Ssum=xd.abs().sum(0))


def running64(rm, rv, st, mom=MOM, mutant=None):
    """(run_mean', S, run_var', S) of one update."""
    m = f32(mom)
    new_v = st.var if mutant == "biased_running" else st.unb
    a, b = (m, 1.0 - m) if mutant == "momentum_swapped" else (1.0 - m, m)
    return (a * rm.double() + b * st.mean, (a * rm.double()).abs() + (b * st.mean).abs(),
            a * rv.double() + b * new_v, (a * rv.double()).abs() + (b * new_v).abs())


def apply64(x, scale, shift, res=None):
    """Pre-activation x scale + shift [+ res] and S."""
    a = x.double() * scale.double()
    pre, S = a + shift.double(), a.abs() + shift.double().abs()
    if res is not None:
        pre, S = pre + res.double(), S + res.double().abs()
    return pre, S


def _bf(t):
    return t.float().to(BF16).double()


def resbn64(x, scale, shift, r, rscale, rshift, mutant=None):
    """Shortcut form: pre = x scale + shift + bf16(idn), idn = r rscale + rshift.  Returns pre, S,
    the allowance 2^-8 |idn| and the alternative pre where idn is within 2^-21 S_idn of a bf16
    rounding midpoint (equal to pre elsewhere)."""
    a = r.double() * rscale.double()
    idn, Si = a + rshift.double(), a.abs() + rshift.double().abs()
    pre0, S0 = apply64(x, scale, shift)
    if mutant == "idn_not_rounded":
        return pre0 + idn, S0 + Si, 2.0 ** -8 * idn.abs(), pre0 + idn
    lo, hi, mid = _bf(idn - 2.0 ** -21 * Si), _bf(idn + 2.0 ** -21 * Si), _bf(idn)
    alt = torch.where(lo != mid, lo, hi)
    return pre0 + mid, S0 + Si, 2.0 ** -8 * idn.abs(), pre0 + alt


def bwd64(dy, x, keep, mean, rstd, gamma, mutant=None):
    """Backward from the rule.  ``keep``: the gate [M, C] bool, or None without a ReLU."""
    M, C = x.shape
    if mutant == "gate_ignored":
        keep = None
    dz = dy.double() * (keep.double() if keep is not None else 1.0)
    mu, rs = mean.double(), rstd.double()
    t = dz * ((x.double() - mu) * rs)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    o = _D(dz=dz, dbeta=dz.sum(0), Sdbeta=dz.abs().sum(0), dgamma=t.sum(0), Sdgamma=t.abs().sum(0))
    o.A = g * rs
    o.B = -o.A * (o.dgamma / M) * rs
    p, q = -o.A * o.dbeta / M, -o.B * mu
    o.D = p + q
    if mutant == "D_sign":
        o.D = -o.D
    if mutant == "D_no_Bmean":
        o.D = p
    o.SA, o.SB, o.SD = o.A.abs(), o.B.abs(), p.abs() + q.abs()
    # raw moments of the ``partials=`` path and their companion
    zx = dz * x.double()
    o.Sraw = rs * (zx.abs().sum(0) + mu.abs() * o.Sdbeta)
    return o


def dx64(dz, x, A, B, D):
    a, b = A.double() * dz, B.double() * x.double()
    return a + b + D.double(), a.abs() + b.abs() + D.double().abs()


def gap64(x):
    """x [N, HW, C] -> mean over HW and S = sum |x| / HW."""
    xd = x.double()
    return xd.mean(1), xd.abs().mean(1)


def gap_bwd64(dy, HW, mutant=None):
    return (dy.double() / (HW + 1 if mutant == "gap_hw_plus_1" else HW))[:, None, :].expand(-1, HW, -1)


def gmp64(x):
    """Maximum over HW and the number of positions that attain it (value compare: signed zeros tie)."""
    xd = x.double()
    m = xd.amax(1)
    return m, (xd == m[:, None]).sum(1).double()


def gmp_bwd64(dy, x, mutant=None):
    xd = x.double()
    m, cnt = gmp64(x)
    hit = xd == m[:, None]
    if mutant == "gmp_bit_compare":  # bit patterns against the first maximum seen
        xb = x.contiguous().view(torch.int16)
        first = torch.gather(xb, 1, hit.int().argmax(1, keepdim=True))
        hit = xb == first
    share = dy.double() / (1.0 if mutant == "gmp_ties_not_shared" else cnt)
    return torch.where(hit, share[:, None], torch.zeros((), dtype=torch.float64)), hit, cnt


# ------------------------------------------------------------------------------- criteria


def elem_ratio(got, ref, S, extra=None, alt=None):
    """max |got - ref| / (2^-8 |ref| + 2^-21 S [+ extra]) (<= 1 passes); with ``alt`` each element is
    judged against the nearer of ref and alt."""
    g = got.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all(), "unwritten or non-finite elements"
    add = 2.0 ** -21 * S + (extra if extra is not None else 0.0)
    q = (g - ref).abs() / (2.0 ** -8 * ref.abs() + add).clamp_min(1e-300)
    if alt is not None:
        q = torch.minimum(q, (g - alt).abs() / (2.0 ** -8 * alt.abs() + add).clamp_min(1e-300))
    return q.max().item()


def fwd_check(y, mask, pre, S, relu, extra=None, alt=None):
    """y [M, C] bf16 (and the bitmask [M, C/8] or None) against the pre-activation.  Returns
    ratio, the gate the kernel took, the number of near-zero elements; asserts the exact parts."""
    M, C = pre.shape
    yd = y.detach().double().cpu().reshape(M, C)
    if not relu:
        assert mask is None
        return _D(ratio=elem_ratio(yd, pre, S, extra, alt), keep=None, unsure=0)
    kb = yd > 0
    if mask is not None:
        assert torch.equal(mask.cpu().reshape(M, C // 8), _relu_bits(kb)), "mask bit != (y > 0)"
    unsure = (pre.abs() <= 2.0 ** -21 * S) & (S > 0)
    if alt is not None:
        unsure |= (alt.abs() <= 2.0 ** -21 * S) | ((alt > 0) != (pre > 0))
    assert torch.equal(kb[~unsure], (pre > 0)[~unsure]), "a gate bit disagrees with the float64 pre-activation"
    assert unsure.double().mean().item() <= NEAR_ZERO_CAP, "too many elements too close to zero to call"
    zero = torch.zeros((), dtype=torch.float64)
    gated_alt = None if alt is None else torch.where(kb, alt, zero)
    return _D(ratio=elem_ratio(yd, torch.where(kb, pre, zero), S, extra, gated_alt),
              keep=kb, unsure=int(unsure.sum()))


def stats_bounds(x, eps=EPS):
    """Per channel (bm, br): max(4 x the fp32 one-pass error, 1e-5) for mean and rstd."""
    st = stats64(x, None, None, eps)
    xf = x.float()
    m1 = xf.sum(0).double() / st.M
    r1 = 1.0 / torch.sqrt(((xf * xf).sum(0).double() / st.M - m1 * m1).clamp_min(0) + f32(eps))
    em = (m1 - st.mean).abs() / torch.maximum(st.mean.abs(), st.sd).clamp_min(1e-300)
    er = (r1 / st.rstd - 1).abs()
    return (4 * em).clamp_min(1e-5), (4 * er).clamp_min(1e-5)


def _q(err, lim):
    """max err / lim; a value whose terms are all zero (lim 0) must be exact, else inf."""
    if (err[lim == 0] != 0).any():
        return float("inf")
    return (err / lim.clamp_min(1e-300)).max().item()


def stats_ratio(stats, x, gamma, beta, eps=EPS, exact=False):
    """stats[4C] = mean | rstd | scale | shift against stats64: err / bound per quantity."""
    st = stats64(x, gamma, beta, eps)
    C = x.shape[1]
    s = stats.detach().double().cpu()
    assert torch.isfinite(s).all()
    mean, rstd, scale, shift = (s[i * C:(i + 1) * C] for i in range(4))
    ms = torch.maximum(st.mean.abs(), st.sd)
    Sshift = st.beta.abs() + ms * st.scale.abs()
    if exact:
        bm = br = torch.full((C,), EXACT_REL, dtype=torch.float64)
        ms, Sshift = st.mean.abs(), st.beta.abs() + (st.mean * st.scale).abs()
    else:
        bm, br = stats_bounds(x, eps)
    return _D(mean=_q((mean - st.mean).abs(), bm * ms), rstd=_q((rstd - st.rstd).abs(), br * st.rstd),
              scale=_q((scale - st.scale).abs(), br * st.scale.abs()),
              shift=_q((shift - st.shift).abs(), (bm + br) * Sshift))


def running_ratio(rm_new, rv_new, rm, rv, x, eps=EPS, mom=MOM, exact=False):
    st = stats64(x, None, None, eps)
    em, Sm, ev, Sv = running64(rm, rv, st, mom)
    m = f32(mom)
    if exact:
        lm, lv = EXACT_REL * Sm, EXACT_REL * Sv
    else:
        bm, br = stats_bounds(x, eps)
        lm = m * bm * torch.maximum(st.mean.abs(), st.sd) + 4 * U * Sm
        lv = m * 2 * br * (st.var + f32(eps)) * (st.M / max(st.M - 1, 1)) + 4 * U * Sv
    return _D(run_mean=_q((rm_new.double().cpu() - em).abs(), lm), run_var=_q((rv_new.double().cpu() - ev).abs(), lv))


def sums_ratio(dgamma, dbeta, coef, ref, M, C, mean, kg, kb, old=None, exact=False):
    """dgamma, dbeta [C] and coef [3C] = A | B | D against bwd64 (``ref``): err / bound.  ``old``:
    (dgamma, dbeta) accumulated into.  exact: equality of the sums, 2^-22 S for the coefficients."""
    dg, db, cf = dgamma.detach().double().cpu(), dbeta.detach().double().cpu(), coef.detach().double().cpu()
    assert torch.isfinite(dg).all() and torch.isfinite(db).all() and torch.isfinite(cf).all()
    A, B, D = cf[:C], cf[C:2 * C], cf[2 * C:]
    mu = mean.double().abs()
    rg, Sg, rb, Sb = ref.dgamma, ref.Sdgamma, ref.dbeta, ref.Sdbeta
    if old is not None:
        og, ob = old[0].double(), old[1].double()
        rg, Sg, rb, Sb = rg + og, Sg + og.abs(), rb + ob, Sb + ob.abs()
    if exact:
        assert old is None
        assert ref.Sdbeta.max() < 2 ** 24 and 2 * ref.Sdgamma.max() < 2 ** 24, "sums must stay below 2^24"
        assert torch.equal(dg, rg) and torch.equal(db, rb), "exact-integer sums must EQUAL the float64 sums"
        eA, eB, eD = EXACT_REL * ref.SA, EXACT_REL * ref.SB, EXACT_REL * ref.SD
        o = _D(dgamma=0.0, dbeta=0.0)
    else:
        o = _D(dgamma=_q((dg - rg).abs(), gamma_k(kg) * Sg), dbeta=_q((db - rb).abs(), gamma_k(kb) * Sb))
        eA = 2 * U * ref.SA
        eB = (ref.A * ref.rstd_ / M).abs() * gamma_k(kg) * ref.Sdgamma + 2 * U * ref.SB
        eD = (ref.A / M).abs() * gamma_k(kb) * ref.Sdbeta + mu * eB + 2 * U * ref.SD
    o.A, o.B, o.D = _q((A - ref.A).abs(), eA), _q((B - ref.B).abs(), eB), _q((D - ref.D).abs(), eD)
    return o


def bwd_ref(d, keep, mean, rstd, gamma, mutant=None):
    o = bwd64(d.dy, d.x, keep, mean, rstd, gamma, mutant)
    o.rstd_ = rstd.double()
    return o


def gap_ratio(y, x, bf_out):
    ref, S = gap64(x)
    HW = x.shape[1]
    lim = HW * U * S + 2 * U * ref.abs() + (2.0 ** -8 * ref.abs() if bf_out else 0.0)
    return _q((y.detach().double().cpu() - ref).abs(), lim)


def gap_exact(x, bf_out):
    """Integer-valued x: float32(sum) * float32(1 / HW), bit for bit (rounded to bf16 for a bf16 output)."""
    HW = x.shape[1]
    v = x.double().sum(1).float() * torch.tensor(1.0, dtype=F32).div(torch.tensor(float(HW), dtype=F32))
    return v.to(BF16) if bf_out else v


def gap_bwd_ratio(dx, dy, HW):
    ref = gap_bwd64(dy, HW)
    return _q((dx.detach().double().cpu().reshape(ref.shape) - ref).abs(), (2 * U + 2.0 ** -8) * ref.abs())


def gmp_bwd_ratio(dx, dy, x):
    """Per element err / 2^-8 |ref| (non-maximum positions exactly 0) and the share sums: the
    float64 sum of dx over HW against dy, err / 2^-8 |dy|."""
    ref, hit, cnt = gmp_bwd64(dy, x)
    g = dx.detach().double().cpu().reshape(ref.shape)
    assert torch.isfinite(g).all()
    assert (g[~hit] == 0).all(), "positions below the maximum must get exactly 0"
    return _q((g - ref).abs(), 2.0 ** -8 * ref.abs()), _q((g.sum(1) - dy.double()).abs(), 2.0 ** -8 * dy.double().abs())


# ------------------------------------------------------------------------------- pool inputs

# (N, H, W, C)
POOL_CASES = [(1, 1, 1, 8), (3, 1, 1, 24), (2, 5, 9, 24), (5, 7, 7, 256), (300, 1, 2, 64), (3, 57, 57, 440)]
CH_TIE0, CH_TIE2, CH_NEG, CH_SZERO = 0, 5, 6, 7  # planted tie channels of images 0 and N - 1


@functools.lru_cache(maxsize=2)
def pool_data(N, H, W, C, integer=False):
    """x [N, HW, C] bf16 and dy [N, C] (fp32; the bf16 runs round it).  Images 0 and N - 1 carry a
    whole-channel tie at 0 (channels 0 - 4), a two-way tie at the maximum (5), an all-negative
    channel with a two-way tie (6) and a channel whose maximum is zero holding both -0.0 and +0.0,
    the negative one first (7); with HW = 1 the plants are single values."""
    g = torch.Generator().manual_seed(2750159 + 1000 * N + 100 * H + 10 * W + C + integer)
    HW = H * W
    d = _D(N=N, HW=HW, C=C)
    if integer:
        d.x = torch.randint(-2, 3, (N, HW, C), generator=g).float().to(BF16)
        d.dy = torch.randint(-2, 3, (N, C), generator=g).float()
        return d
    x = torch.randn(N, HW, C, generator=g)
    last = HW - 1
    for n in {0, N - 1}:
        x[n, :, 0:5] = 0.0
        x[n, 0, CH_TIE2] = x[n, last, CH_TIE2] = 9.0
        x[n, :, CH_NEG] = -1.0 - x[n, :, CH_NEG].abs()
        x[n, 0, CH_NEG] = x[n, last, CH_NEG] = -0.5
        x[n, :, CH_SZERO] = -0.25 - x[n, :, CH_SZERO].abs()
        x[n, 0, CH_SZERO] = -0.0
        x[n, last, CH_SZERO] = 0.0
        if HW >= 3:
            x[n, 1, CH_SZERO] = -0.0
    d.x = x.to(BF16)
    d.dy = torch.randn(N, C, generator=g)
    return d


def planted_tie_counts(d):
    """cnt the plants must produce in image 0: channels 0, 5, 6, 7."""
    HW = d.HW
    return {CH_TIE0: HW, CH_TIE2: min(HW, 2), CH_NEG: min(HW, 2), CH_SZERO: min(HW, 3)}


# ------------------------------------------------------------------------------- fp32 emulation
# The kernels' operations in the kernels' order, each rounded once to fp32 (FMAs through float64:
# the product of a bf16 and an fp32 value is exact there).


def emu_reduce(a, b, M, C, group, mutant=None):
    """bn_stats_kernel (group 4) / bn_bwd_reduce_kernel (group 2) over the fp32 addends a, b [M, C]:
    per thread the unrolled trips ((v0 + v1) + (v2 + v3) or v0 + v1 added to the running sum) and
    the one-row tail, block_col_reduce sequential over the RP row groups, the chunks in double.
    Returns (sum a, sum b) as float64 [C]."""
    t = make_tiling(M, C)
    RP, rpc, n = t.RP, t.rpc, t.nchunks
    K = rpc // RP
    a, b = a.clone(), b.clone()
    if mutant == "row_dropped":
        a[M // 2], b[M // 2] = 0, 0
    if mutant == "ragged_dropped":
        r0 = (n - 1) * rpc
        r0 += ((M - r0) // RP) * RP
        a[r0:], b[r0:] = 0, 0
    full = torch.empty(n, RP, dtype=torch.long)  # unrolled trips of thread ty of each chunk
    full[:] = thread_rows(t, M, 0)[:RP] // group
    full[n - 1] = thread_rows(t, M, n - 1)[:RP] // group
    out = []
    for v in (a, b):
        A = torch.cat([v, v.new_zeros(n * rpc - M, C)]).view(n, K, RP, C)
        s = torch.zeros(n, RP, C)
        for g in range(K // group):
            vs = [A[:, g * group + i] for i in range(group)]
            tree = (vs[0] + vs[1]) if group == 2 else (vs[0] + vs[1]) + (vs[2] + vs[3])
            seq = s
            for w in vs:
                seq = seq + w
            s = torch.where((full > g)[..., None], s + tree, seq)
        for k in range(K // group * group, K):
            s = s + A[:, k]
        r = torch.zeros(n, C)
        for ty in range(RP):
            r = r + s[:, ty]
        if mutant == "stray_twice" and BLK % t.TW and K > 1:
            # the stray threads (ty == RP, tx < 256 - TW RP) walk rows RP, 2 RP, .. of the chunk
            tx = BLK - t.TW * RP
            cols = torch.cat([torch.arange(8) + 8 * (blk * t.TW + x) for blk in range(t.ncol) for x in range(tx)])
            cols = cols[cols < C]
            r[:, cols] += A[:, 1:, 0][:, :, cols].sum(1)
        out.append(r.double().sum(0))
    return out


def emu_fwd_finalize(s, q, M, gamma, beta, eps=EPS, mom=MOM, rm=None, rv=None):
    """FwdFin: double until the stores.  Returns stats[4C] fp32 and the updated running stats."""
    mean = s / M
    var = (q / M - mean * mean).clamp_min(0)
    rstd = (1.0 / torch.sqrt(var + f32(eps))).float()
    C = s.numel()
    g = gamma.float() if gamma is not None else torch.ones(C)
    b = beta.float() if beta is not None else torch.zeros(C)
    m32 = mean.float()
    stats = torch.cat([m32, rstd, g * rstd, b - m32 * g * rstd])
    if rm is None:
        return stats, None, None
    unb = var * M / (M - 1) if M > 1 else var
    m = torch.tensor(mom, dtype=F32)
    return stats, (1 - m) * rm + m * m32, (1 - m) * rv + m * unb.float()


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emu_apply(x, scale, shift, res=None, relu=True, rss=None, mutant=None):
    """bn_apply_kernel / bn_apply_resbn_kernel (``rss`` = the shortcut BN's [scale | shift], res its input)."""
    C = x.shape[1]
    z = _fma(x.float(), scale, shift)
    if rss is not None:
        idn = _fma(res.float(), rss[:C], rss[C:])
        z = z + (idn if mutant == "idn_not_rounded" else idn.to(BF16).float())
    elif res is not None:
        z = z + res.float()
    if relu:
        z = z.clamp_min(0.0)
    return z.to(BF16), (_relu_bits(z > 0) if relu else None)


def emu_bwd(dy, x, keep, mean, rstd, gamma, M, C, accumulate=None, mutant=None):
    """bn_bwd_reduce_kernel + BwdFin + bn_bwd_apply_kernel.  Returns dgamma, dbeta, coef, dx, dres."""
    d = dy.float() if keep is None else torch.where(keep, dy.float(), torch.zeros(()))  # gated off: +0, as relu_gate
    sd, sdx = emu_reduce(d, d * (x.float() - mean.float()) * rstd.float(), M, C, 2, mutant)
    g = gamma.double() if gamma is not None else torch.ones(C, dtype=torch.float64)
    rs, mu = rstd.double(), mean.double()
    k1 = g * rs
    a, b = sd / M, sdx / M
    coef = torch.cat([k1, -k1 * b * rs, -k1 * a + k1 * b * rs * mu]).float()
    dgamma, dbeta = sdx.float(), sd.float()
    if accumulate is not None:
        dgamma, dbeta = dgamma + accumulate[0], dbeta + accumulate[1]
    dx = _fma(coef[:C], d, _fma(coef[C:2 * C], x.float(), coef[2 * C:])).to(BF16)
    return dgamma, dbeta, coef, dx, d.to(BF16)


def emu_gap(x, bf_out):
    acc = torch.zeros(x.shape[0], x.shape[2])
    for i in range(x.shape[1]):
        acc = acc + x[:, i].float()
    y = acc * (torch.tensor(1.0) / torch.tensor(float(x.shape[1])))
    return y.to(BF16) if bf_out else y


def emu_gmp_bwd(dy, x):
    m, cnt = gmp64(x)
    share = (dy.float() / cnt.float()).to(BF16)
    return torch.where(x.double() == m[:, None], share[:, None], torch.zeros((), dtype=BF16))


# ------------------------------------------------------------------------------- cross-checks


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True)])
def test_references_match_torch_float64_autograd(relu, res):
    d = bn_data(131, 40, "random")
    x = d.x.double().requires_grad_()
    gm, bt = d.gamma.double().requires_grad_(), d.beta.double().requires_grad_()
    r = d.res.double().requires_grad_() if res else None
    rm, rv = d.rm.double().clone(), d.rv.double().clone()
    z = F.batch_norm(x, rm, rv, gm, bt, True, f32(MOM), f32(EPS))
    z = z + r if res else z
    y = torch.relu(z) if relu else z
    y.backward(d.dy.double())
    st = stats64(d.x, d.gamma, d.beta)
    pre, _ = apply64(d.x, st.scale, st.shift, d.res if res else None)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-11)  # noqa: E731
    close(pre.clamp_min(0) if relu else pre, y.detach())
    em, _, ev, _ = running64(d.rm, d.rv, st)
    close(em, rm), close(ev, rv)
    o = bwd64(d.dy, d.x, (pre > 0) if relu else None, st.mean, st.rstd, d.gamma)
    close(o.dbeta, bt.grad), close(o.dgamma, gm.grad)
    close(dx64(o.dz, d.x, o.A, o.B, o.D)[0], x.grad)
    if res:
        close(o.dz, r.grad)


def test_pool_references_match_torch_float64_autograd():
    d = pool_data(2, 5, 9, 24)
    x = d.x.double().requires_grad_()
    x.mean(1).backward(d.dy.double())
    assert torch.equal(gap64(d.x)[0], d.x.double().mean(1))
    torch.testing.assert_close(gap_bwd64(d.dy, d.HW).contiguous(), x.grad, rtol=1e-12, atol=0)
    x.grad = None
    y = x.amax(1)
    y.backward(d.dy.double())
    ref, hit, cnt = gmp_bwd64(d.dy, d.x)
    assert torch.equal(gmp64(d.x)[0], y.detach())
    torch.testing.assert_close(ref, x.grad, rtol=1e-12, atol=0)  # amax shares over ties, signed zeros included
    for ch, k in planted_tie_counts(d).items():
        assert cnt[0, ch] == k, (ch, cnt[0, ch], k)
    assert (ref[0, :, CH_SZERO] != 0).sum() == 3


def test_m_equal_1_formula():
    """torch refuses M = 1 in training mode; the explicit formula is the reference: var 0,
    rstd = 1 / sqrt(eps), y = beta, unb = var."""
    d = bn_data(1, 8, "random")
    st = stats64(d.x, d.gamma, d.beta)
    assert torch.equal(st.var, torch.zeros(8, dtype=torch.float64)) and torch.equal(st.unb, st.var)
    assert torch.equal(st.mean, d.x.double()[0])
    torch.testing.assert_close(apply64(d.x, st.scale, st.shift)[0][0], d.beta.double(), rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------- soundness


def _combos(c):
    return [(True, True)] if reduced(c) else [(r, s) for r in (False, True) for s in (False, True)]


@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_emulation_and_torch_path_meet_the_forward_criteria(c):
    from cloud_amd.ops.batchnorm import _torch_bn_act

    M, C = c.M, c.C
    d = bn_data(M, C, c.data)
    exact = c.data == "integer"
    xf = d.x.float()
    s, q = emu_reduce(xf, xf * xf, M, C, 4)
    st = stats64(d.x, d.gamma, d.beta)
    if exact:
        assert st.Ssum.max() < 2 ** 24 and st.sumsq.max() < 2 ** 24
        assert torch.equal(s, st.sum) and torch.equal(q, st.sumsq), "exact-integer sums must EQUAL the float64 sums"
    stats, rm, rv = emu_fwd_finalize(s, q, M, d.gamma, d.beta, rm=d.rm, rv=d.rv)
    w = dict(stats_ratio(stats, d.x, d.gamma, d.beta, exact=exact))
    w.update(running_ratio(rm, rv, d.rm, d.rv, d.x, exact=exact))
    unsure = 0
    for relu, res in _combos(c):
        r = d.res if res else None
        y, mask = emu_apply(d.x, stats[2 * C:3 * C], stats[3 * C:], r, relu)
        f = fwd_check(y, mask, *apply64(d.x, stats[2 * C:3 * C], stats[3 * C:], r), relu)
        w["y"], unsure = max(w.get("y", 0.0), f.ratio), max(unsure, f.unsure)
        if relu and not res:
            assert (y[:, CH_GAMMA0] == 0).all() and (mask[:, 0] & 1 == 0).all()
        # the project's torch path, judged with ITS fp32 statistics
        yt = _torch_bn_act(d.x, r, d.gamma, d.beta, None, None, EPS, MOM, relu, True)
        m32, v32 = xf.mean(0), xf.var(0, unbiased=False)
        sc = d.gamma.double() / torch.sqrt(v32.double() + EPS)
        ft = fwd_check(yt, None, *apply64(d.x, sc, d.beta.double() - m32.double() * sc, r), relu)
        w["y_torch"] = max(w.get("y_torch", 0.0), ft.ratio)
    if c in SHORTCUT_CASES:
        y, mask = emu_apply(d.x, stats[2 * C:3 * C], stats[3 * C:], d.r, True, rss=d.rss)
        pre, S, extra, alt = resbn64(d.x, stats[2 * C:3 * C], stats[3 * C:], d.r, d.rss[:C], d.rss[C:])
        w["shortcut"] = fwd_check(y, mask, pre, S, True, extra, alt).ratio
        idn, _ = emu_apply(d.r, d.rss[:C], d.rss[C:], None, False)
        assert torch.equal(y, emu_apply(d.x, stats[2 * C:3 * C], stats[3 * C:], idn, True)[0]), "op-by-op path"
    _say(f"cpu fwd {c.name}: err / bound", {k: round(v, 3) for k, v in w.items()}, f"near-zero {unsure} of {M * C}")
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("c", CASES, ids=_ids)
def test_emulation_meets_the_backward_criteria(c):
    M, C = c.M, c.C
    d = bn_data(M, C, c.data)
    exact = c.data == "integer"
    if exact:
        stats, keep = planted_stats(d), d.keep
    else:
        xf = d.x.float()
        stats = emu_fwd_finalize(*emu_reduce(xf, xf * xf, M, C, 4), M, d.gamma, d.beta)[0]
        y, _ = emu_apply(d.x, stats[2 * C:3 * C], stats[3 * C:], d.res, True)
        keep = y.double() > 0
    mean, rstd = stats[:C], stats[C:2 * C]
    w = {}
    for relu, acc in ((True, False), (False, False)) + (() if exact else ((True, True),)):
        old = (d.old_dgamma, d.old_dbeta) if acc else None
        kp = keep if relu else None
        dg, db, coef, dx, dres = emu_bwd(d.dy, d.x, kp, mean, rstd, d.gamma, M, C, old)
        ref = bwd_ref(d, kp, mean, rstd, d.gamma)
        r = sums_ratio(dg, db, coef, ref, M, C, mean, chain_k(M, C, "dgamma", acc), chain_k(M, C, "dbeta", acc), old,
                       exact)
        r.dx = elem_ratio(dx, *dx64(ref.dz, d.x, coef[:C], coef[C:2 * C], coef[2 * C:]))
        want = d.dy.view(torch.int16) * (kp.to(torch.int16) if kp is not None else 1)
        assert torch.equal(dres.view(torch.int16), want), "dres: the bits of dy where gated on, +0 elsewhere"
        assert (dx[:, CH_GAMMA0] == 0).all(), "gamma = 0: dx must be exactly 0"
        for k, v in r.items():
            w[k] = max(w.get(k, 0.0), v)
    _say(f"cpu bwd {c.name}: err / bound", {k: round(v, 3) for k, v in w.items()},
         f"k = {chain_k(M, C, 'dbeta')} / {chain_k(M, C, 'dgamma')}")
    assert max(w.values()) <= 1.0, w


def partials_of(a, b, rows=128):
    """[tiles][2][C] fp32 partials of the float64 addends a, b [M, C] (float64-exact, rounded once)."""
    M, C = a.shape
    tiles = -(-M // rows)
    pad = lambda v: torch.cat([v, v.new_zeros(tiles * rows - M, C)]).view(tiles, rows, C).sum(1)  # noqa: E731
    return torch.stack([pad(a), pad(b)], 1).float()


def raw_ratio(dgamma, dbeta, ref, nparts, rpg=512, old=None):
    """dgamma / dbeta of the ``partials=`` path against bwd64, on S' (module docstring)."""
    k = gamma_k(partials_k(nparts, rpg) + (1 if old is not None else 0))
    og, ob = (old[0].double(), old[1].double()) if old is not None else (0.0, 0.0)
    return _D(dgamma=_q((dgamma.double().cpu() - ref.dgamma - og).abs(), k * (ref.Sraw + abs(og))),
              dbeta=_q((dbeta.double().cpu() - ref.dbeta - ob).abs(), k * (ref.Sdbeta + abs(ob))))


@pytest.mark.parametrize("c", [CASE["234x64"], CASE["16641x8"]], ids=_ids)
def test_raw_moment_partials_meet_their_bound(c):
    d = bn_data(c.M, c.C, "random")
    st = stats64(d.x, d.gamma, d.beta)
    mean, rstd = st.mean.float(), st.rstd.float()
    ref = bwd_ref(d, d.keep, mean, rstd, d.gamma)
    p = partials_of(ref.dz, ref.dz * d.x.double())
    sd, sdx = p[:, 0].sum(0).double(), p[:, 1].sum(0).double()  # fp32 sums: within the group-sum chain
    r = raw_ratio((rstd.double() * (sdx - mean.double() * sd)).float(), sd.float(), ref, p.shape[0])
    _say(f"cpu raw-moment partials {c.name}: err / bound {dict(r)}")
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("case", POOL_CASES[:5], ids=lambda c: "x".join(map(str, c)))
def test_pool_emulation_meets_the_criteria(case):
    d = pool_data(*case)
    w = {}
    for bf in (True, False):
        w[f"gap{'_bf' if bf else ''}"] = gap_ratio(emu_gap(d.x, bf), d.x, bf)
        dy = d.dy.to(BF16) if bf else d.dy
        k = "_bf" if bf else ""
        spread = (dy.float() * (torch.tensor(1.0) / d.HW))[:, None].expand(-1, d.HW, -1).to(BF16)
        w["gap_bwd" + k] = gap_bwd_ratio(spread, dy, d.HW)
        w["gmp_bwd" + k], w["gmp_sum" + k] = gmp_bwd_ratio(emu_gmp_bwd(dy, d.x), dy, d.x)
    di = pool_data(*case, integer=True)
    for bf in (True, False):
        assert torch.equal(emu_gap(di.x, bf), gap_exact(di.x, bf))
    _say(f"cpu pools {case}: err / bound", {k: round(v, 3) for k, v in w.items()})
    assert max(w.values()) <= 1.0, w


def test_gmp_share_sum_bound_on_paper():
    """A correctly rounded share exceeds HW 2^-9 |dy| / cnt where cnt = HW: dy = 1 + 2^-8 rounds (to
    even) to 1.0, off by 2^-8 = 0.996 of 2^-8 |dy| and 1.99 of 2^-9 |dy|."""
    dy = torch.tensor([[1.0 + 2.0 ** -8]])
    x = torch.zeros(1, 1, 1, dtype=BF16)
    dx = emu_gmp_bwd(dy, x)
    err = (dx.double().sum(1) - dy.double()).abs().item()
    assert 2.0 ** -9 * dy.item() < err <= 2.0 ** -8 * dy.item()
    assert max(gmp_bwd_ratio(dx, dy, x)) <= 1.0


# ------------------------------------------------------------------------------- discrimination
# Each mutant is one plausible defect of a kernel, judged on the case built for it.


@pytest.mark.parametrize("mutant,name", [("row_dropped", "16389x512"), ("row_dropped", "87041x24"),
                                         ("ragged_dropped", "16389x512"), ("ragged_dropped", "200x24"),
                                         ("stray_twice", "87041x24")])
def test_sum_mutant_is_rejected_by_the_exact_cases(mutant, name):
    c = CASE[name]
    d = bn_data(c.M, c.C, "integer")
    xf = d.x.float()
    st = stats64(d.x, None, None)
    s, q = emu_reduce(xf, xf * xf, c.M, c.C, 4, mutant)
    assert not torch.equal(q, st.sumsq), "forward sum of squares"
    stats = planted_stats(d)
    dg, db, coef, _, _ = emu_bwd(d.dy, d.x, d.keep, stats[:c.C], stats[c.C:2 * c.C], d.gamma, c.M, c.C, mutant=mutant)
    ref = bwd_ref(d, d.keep, stats[:c.C], stats[c.C:2 * c.C], d.gamma)
    assert not torch.equal(db.double(), ref.dbeta) or not torch.equal(dg.double(), ref.dgamma)
    with pytest.raises(AssertionError):
        sums_ratio(dg, db, coef, ref, c.M, c.C, stats[:c.C], 0, 0, exact=True)


@pytest.mark.parametrize("mutant,name", [("row_dropped", "6272x256"), ("row_dropped", "234x64"),
                                         ("ragged_dropped", "131x40")])
def test_sum_mutant_is_rejected_by_the_counted_bound(mutant, name):
    c = CASE[name]
    M, C = c.M, c.C
    d = bn_data(M, C, "random")
    st = stats64(d.x, d.gamma, d.beta)
    mean, rstd = st.mean.float(), st.rstd.float()
    dg, db, coef, _, _ = emu_bwd(d.dy, d.x, d.keep, mean, rstd, d.gamma, M, C, mutant=mutant)
    r = sums_ratio(dg, db, coef, bwd_ref(d, d.keep, mean, rstd, d.gamma), M, C, mean, chain_k(M, C, "dgamma"),
                   chain_k(M, C, "dbeta"))
    _say(f"mutant {mutant} {name}: dbeta {r.dbeta:.1f} dgamma {r.dgamma:.1f} of the bound")
    assert r.dbeta > 1.0 and r.dgamma > 1.0, r


@pytest.mark.parametrize("mutant", ["gate_ignored", "gate_y_ge0", "D_sign", "D_no_Bmean"])
def test_backward_mutant_is_rejected(mutant):
    c = CASE["234x64"]
    M, C = c.M, c.C
    d = bn_data(M, C, "random")
    st = stats64(d.x, d.gamma, d.beta)
    mean, rstd = st.mean.float(), st.rstd.float()
    y, _ = emu_apply(d.x, st.scale.float(), st.shift.float(), None, True)
    keep = y.double() > 0
    ref = bwd_ref(d, keep, mean, rstd, d.gamma)
    mut = bwd_ref(d, (y.double() >= 0) if mutant == "gate_y_ge0" else keep, mean, rstd, d.gamma, mutant)
    r = sums_ratio(mut.dgamma.float(), mut.dbeta.float(), torch.cat([mut.A, mut.B, mut.D]).float(), ref, M, C, mean,
                   chain_k(M, C, "dgamma"), chain_k(M, C, "dbeta"))
    rdx = elem_ratio(dx64(mut.dz, d.x, mut.A, mut.B, mut.D)[0].to(BF16), *dx64(ref.dz, d.x, ref.A, ref.B, ref.D))
    _say(f"mutant {mutant}: {dict(r)} dx {rdx:.1f} of the bound")
    if mutant.startswith("gate"):
        assert r.dbeta > 1.0 and r.dgamma > 1.0 and not torch.equal(mut.dz, ref.dz), r
    else:
        assert r.D > 1.0 and rdx > 1.0, (r, rdx)


@pytest.mark.parametrize("mutant", ["unbiased_rstd", "biased_running", "momentum_swapped"])
def test_statistics_mutant_is_rejected(mutant):
    c = CASE["234x64"]
    d = bn_data(c.M, c.C, "random")
    st = stats64(d.x, d.gamma, d.beta, mutant=mutant)
    if mutant == "unbiased_rstd":
        r = stats_ratio(torch.cat([st.mean, st.rstd, st.scale, st.shift]).float(), d.x, d.gamma, d.beta)
        _say(f"mutant {mutant}: rstd {r.rstd:.0f} scale {r.scale:.0f} of the bound")
        assert r.rstd > 1.0 and r.scale > 1.0, r
    else:
        em, _, ev, _ = running64(d.rm, d.rv, st, mutant=mutant)
        r = running_ratio(em.float(), ev.float(), d.rm, d.rv, d.x)
        _say(f"mutant {mutant}: {dict(r)} of the bound")
        assert r.run_var > 1.0 and (mutant == "biased_running" or r.run_mean > 1.0), r


def test_shortcut_value_not_rounded_is_rejected():
    """The derived bound allows the skipped rounding by construction; the op-by-op identity does not."""
    c = CASE["200x24"]
    C = c.C
    d = bn_data(c.M, C, "random")
    st = stats64(d.x, d.gamma, d.beta)
    sc, sh = st.scale.float(), st.shift.float()
    idn, _ = emu_apply(d.r, d.rss[:C], d.rss[C:], None, False)
    two_step, _ = emu_apply(d.x, sc, sh, idn, True)
    assert torch.equal(emu_apply(d.x, sc, sh, d.r, True, rss=d.rss)[0], two_step)
    mut, mask = emu_apply(d.x, sc, sh, d.r, True, rss=d.rss, mutant="idn_not_rounded")
    frac = (mut.view(torch.int16) != two_step.view(torch.int16)).double().mean().item()
    pre, S, extra, alt = resbn64(d.x, sc, sh, d.r, d.rss[:C], d.rss[C:])
    _say(f"mutant idn_not_rounded: {100 * frac:.1f} % of the bits differ from the op-by-op path; "
         f"err / derived bound {fwd_check(mut, mask, pre, S, True, extra, alt).ratio:.3f}")
    assert frac > 0.05


@pytest.mark.parametrize("mutant", ["gmp_ties_not_shared", "gmp_bit_compare", "gap_hw_plus_1"])
def test_pool_mutant_is_rejected(mutant):
    d = pool_data(2, 5, 9, 24)
    if mutant == "gap_hw_plus_1":
        assert gap_bwd_ratio(gap_bwd64(d.dy, d.HW, mutant).to(BF16), d.dy, d.HW) > 1.0
        assert gap_ratio((gap64(d.x)[0] * d.HW / (d.HW + 1)).to(BF16), d.x, True) > 1.0
        return
    bad = gmp_bwd64(d.dy, d.x, mutant)[0].to(BF16)
    ref, hit, _ = gmp_bwd64(d.dy, d.x)
    per = _q((bad.double() - ref).abs(), 2.0 ** -8 * ref.abs())
    tot = _q((bad.double().sum(1) - d.dy.double()).abs(), 2.0 ** -8 * d.dy.double().abs())
    _say(f"mutant {mutant}: per element {per:.1f}, share sum {tot:.1f} of the bound")
    assert per > 1.0 and tot > 1.0
    if mutant == "gmp_bit_compare":  # only the signed-zero channel is hit: -0.0 first, so +0.0 gets nothing
        wrong = ((bad.double() - ref).abs() > 2.0 ** -8 * ref.abs()).any(1)
        assert wrong[0, CH_SZERO] and int(wrong.sum()) == 2
