"""Planted pre-activations for the conv epilogues and what each must become (numpy only, no GPU, no torch).

A conv with all-zero weights has an accumulator of +0, so the pre-activation of channel c is its folded bias bit for bit,
whatever the kernel's K order, tile or MFMA: the epilogue's result is a function of known float32 inputs.  This module holds

  * ``rne_bf16`` / ``rne_f16``: the two storage roundings on integer bit patterns (a second implementation: the host test
    compares ``oracle.darknet_oracle.bf16_round`` / ``f16_round`` against them);
  * one list of at most 128 tagged float32 pre-activations per activation (``cases(act)``);
  * the expected value of every entry: exact for linear / leaky, an interval of storage values for mish / logistic
    (``expect``), with or without a shortcut operand r;
  * the shortcut pre-activations of the two residual convs of the family network, found by search against the known
    operands (``shortcut_cases``);
  * the channel layout of the GPU test (``offset``, ``layer_values``, ``finite_only``).

Two things the family network cannot hold, because a zero weight times a non-finite input is NaN (the accumulator of every
conv that READS a non-finite activation is NaN): a non-finite shortcut operand r (inf + -inf, finite a + NaN r), and a
non-finite value in any layer whose reader is checked in the same forward.  The GPU test therefore runs one forward per
checked layer, with the complete list in that layer and ``finite_only`` lists in the layers before it; inf + finite r and
NaN + finite r are planted on the a side.  The fused kernels take their shortcut operand from the input of their first conv,
so it must be finite there too; inf + -inf and finite + NaN are planted on a single conv that reads its operand from a tensor
of its own (test_shortcut_operand_non_finite).

A bias of -0.0 gives t = +0 * scale + -0 = +0 under a positive BN scale.  ``NEG_SCALE_TAG`` marks the one entry whose
channel gets a negative scale (gamma < 0, mean = -0.0): +0 * scale = -0, and -0 + -0 = -0.
"""
import collections

import numpy as np

F32 = np.float32
Case = collections.namedtuple("Case", "tag t kind")      # kind: tie / nbr / threshold / sat / range / nonfinite
DTYPES = ("float32", "bf16", "fp16")
ACTS = ("linear", "leaky", "mish", "logistic")
SLOPE = F32(0.1)
FILLER = F32(0.5)
NEG_SCALE_TAG = "-0"
LIST_LEN = 128


def f32(x):
    return np.asarray(x, dtype=np.float32)


def bits(x):
    return f32(x).view(np.uint32)


def from_bits(u):
    return np.asarray(u, dtype=np.uint32).view(np.float32)


def step(x, n):
    """the float32 n steps above (n > 0) / below (n < 0) x on the real line (x finite, non-zero, no sign change)"""
    b = bits(x).astype(np.int64)
    return from_bits((b + np.where(b & 0x80000000, -n, n)).astype(np.uint32))


# ---- storage roundings on bit patterns -----------------------------------------------------------------------------------
def rne_bf16(x):
    u = bits(x).astype(np.uint64)
    nan = (u & 0x7fffffff) > 0x7f800000
    r = (u + 0x7fff + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xffff0000)    # a carry out of the mantissa is the overflow to inf
    r = np.where(nan, (u | np.uint64(0x00400000)) & np.uint64(0xffff0000), r)
    return from_bits(r.astype(np.uint32))


def rne_f16(x):
    u = bits(x).astype(np.uint64)
    sign = (u & np.uint64(0x80000000)).astype(np.uint32)
    a = u & np.uint64(0x7fffffff)
    nan = a > 0x7f800000
    # normal halves: drop 13 mantissa bits
    rn = (a + np.uint64(0xfff) + ((a >> np.uint64(13)) & np.uint64(1))) & np.uint64(0xffffe000)
    rn = np.where(rn > 0x477fe000, np.uint64(0x7f800000), rn)                  # above 65504: inf
    # below 2^-14: a multiple q of 2^-24, q = m * 2^(e - 126) rounded
    e = (a >> np.uint64(23)).astype(np.int64)
    m = np.where(e > 0, (a & np.uint64(0x7fffff)) | np.uint64(0x800000), a & np.uint64(0x7fffff))
    sh = np.clip(126 - np.maximum(e, 1), 1, 40).astype(np.uint64)
    q = m >> sh
    rem = m & ((np.uint64(1) << sh) - np.uint64(1))
    half = np.uint64(1) << (sh - np.uint64(1))
    q = q + ((rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))).astype(np.uint64)
    rs = bits(q.astype(np.float32) * F32(2.0 ** -24)).astype(np.uint64)
    r = np.where(a < 0x38800000, rs, rn)
    r = np.where(nan, a | np.uint64(0x00400000), r)
    return from_bits(r.astype(np.uint32) | sign)


def rne_f32(x):
    return f32(x)


RND = {"float32": rne_f32, "bf16": rne_bf16, "fp16": rne_f16}
STORE_MAX = {"float32": from_bits(0x7f7fffff), "bf16": from_bits(0x7f7f0000), "fp16": F32(65504.0)}
# mantissa bits dropped by the narrowing (a tie has exactly the top dropped bit set); fp16: in its normal range
DROPPED = {"bf16": 16, "fp16": 13}


def is_tie(dtype, x):
    """x sits exactly halfway between two neighbouring storage values (integer arithmetic on its bit pattern)"""
    a = int(bits(x)) & 0x7fffffff
    if a >= 0x7f800000:
        return False
    if dtype == "bf16":
        return (a & 0xffff) == 0x8000
    if a >= 0x38800000:
        return (a & 0x1fff) == 0x1000
    e = a >> 23
    m = (a & 0x7fffff) | 0x800000 if e > 0 else a & 0x7fffff
    sh = 126 - max(e, 1)
    return sh < 40 and (m & ((1 << sh) - 1)) == 1 << (sh - 1)


def round_odd_f32(x64):
    """float64 -> float32, round to odd: a later nearest-even narrowing to a 16-bit type is then the direct rounding"""
    x64 = np.asarray(x64, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = x64.astype(np.float32)
        exact = (f.astype(np.float64) == x64) | np.isnan(x64)
        other = np.nextafter(f, np.where(x64 > f.astype(np.float64), F32(np.inf), F32(-np.inf)).astype(np.float32))
    odd = (bits(f) & 1) == 1
    return np.where(exact | odd, f, other).astype(np.float32)


def rnd64(dtype, x64):
    """a float64 value rounded once to the storage type; float32: to nearest"""
    if dtype == "float32":
        with np.errstate(over="ignore"):
            return np.asarray(x64, dtype=np.float64).astype(np.float32)
    return RND[dtype](round_odd_f32(x64))


# ---- the lists -------------------------------------------------------------------------------------------------------------
def _with_neighbours(tag, v, kind="tie"):
    return [Case(tag, F32(v), kind), Case(tag + " -1 step", F32(step(v, -1)), "nbr"), Case(tag + " +1 step", F32(step(v, 1)), "nbr")]


def _common():
    c = []
    for tag, v in (("0", 0.0), ("smallest subnormal", from_bits(1)), ("1e-40", 1e-40), ("FLT_MIN", from_bits(0x00800000)),
                   ("0.5", 0.5), ("1", 1.0), ("FLT_MAX", from_bits(0x7f7fffff)), ("inf", np.inf)):
        kind = "nonfinite" if tag == "inf" else "range"
        c += [Case("+" + tag, F32(v), kind), Case("-" + tag, F32(-F32(v)), kind)]
    c.append(Case("NaN", F32(np.nan), "nonfinite"))
    # bf16: 8 mantissa bits kept
    c += _with_neighbours("bf16 tie 1+2^-8 (even below)", 1 + 2.0 ** -8)
    c += _with_neighbours("bf16 tie 1+3*2^-8 (odd below)", 1 + 3 * 2.0 ** -8)
    c.append(Case("bf16 tie -(1+3*2^-8)", F32(-(1 + 3 * 2.0 ** -8)), "tie"))
    c.append(Case("bf16 max 3.3895314e38", from_bits(0x7f7f0000), "range"))
    c.append(Case("bf16 overflow: below the tie above max", from_bits(0x7f7f7fff), "nbr"))
    c.append(Case("bf16 overflow: tie above max", from_bits(0x7f7f8000), "tie"))
    # fp16: 11 bits kept
    c += _with_neighbours("fp16 tie 1+2^-11 (even below)", 1 + 2.0 ** -11)
    c += _with_neighbours("fp16 tie 1+3*2^-11 (odd below)", 1 + 3 * 2.0 ** -11)
    c.append(Case("fp16 max 65504", F32(65504.0), "range"))
    c.append(Case("fp16 overflow: largest float32 below 65520", F32(step(F32(65520.0), -1)), "nbr"))
    c.append(Case("fp16 overflow: 65520 (tie, to inf)", F32(65520.0), "tie"))
    c.append(Case("fp16 subnormal 2^-24", F32(2.0 ** -24), "range"))
    c.append(Case("fp16 subnormal tie 2^-25 (to 0)", F32(2.0 ** -25), "tie"))
    c.append(Case("fp16 subnormal: just above 2^-25", F32(step(F32(2.0 ** -25), 1)), "nbr"))
    c.append(Case("fp16 subnormal tie 3*2^-25 (odd below)", F32(3 * 2.0 ** -25), "tie"))
    c.append(Case("fp16 largest subnormal 1023*2^-24", F32(1023 * 2.0 ** -24), "range"))
    c.append(Case("fp16 subnormal tie 1023.5*2^-24 (to 2^-14)", F32(1023.5 * 2.0 ** -24), "tie"))
    c.append(Case("fp16 -3e-5 (subnormal, negative)", F32(-3e-5), "range"))
    return c


def leaky_f32(t):
    """the scalar epilogue: t > 0 ? t : 0.1f * t, every operation float32"""
    t = f32(t)
    with np.errstate(all="ignore"):
        return np.where(t > 0, t, SLOPE * t).astype(np.float32)


def leaky_max(t):
    """the 16-bit epilogues: max(t, 0.1f * t)"""
    t = f32(t)
    with np.errstate(all="ignore"):
        return np.maximum(t, SLOPE * t).astype(np.float32)


def leaky_double_slope(t):
    """NOT the product's: the slope as a double 0.1, narrowed afterwards"""
    t = f32(t)
    with np.errstate(all="ignore"):
        return np.where(t > 0, t, (0.1 * t.astype(np.float64)).astype(np.float32)).astype(np.float32)


def leaky_preimage(a):
    """a negative t with float32(0.1f * t) == a (a < 0), or None"""
    a = F32(a)
    with np.errstate(all="ignore"):
        t0 = F32(a / SLOPE)
        if not np.isfinite(t0) or t0 == 0:
            return None
        cand = step(np.full(33, t0, dtype=np.float32), np.arange(-16, 17))
        hit = cand[(SLOPE * cand).astype(np.float32) == a]
    return F32(hit[0]) if hit.size else None


def _leaky_extra():
    c = []
    for dtype, lo_bits in (("bf16", 8), ("fp16", 11)):
        for odd in (0, 1):
            for k in range(0, 12):          # the tie -(1 + (2 odd + 1) 2^-lo_bits) * 2^k, first k with a preimage
                tie = F32(-(1 + (2 * odd + 1) * 2.0 ** -lo_bits) * 2.0 ** k)
                t = leaky_preimage(tie)
                if t is not None:
                    break
            c += _with_neighbours("leaky: 0.1f*t on a %s tie (%s below)" % (dtype, "odd" if odd else "even"), t)
    for dtype in DTYPES:
        w = slope_witnesses(dtype)
        if w.size:
            c.append(Case("leaky: float slope 0.1f against a double 0.1, differs after %s rounding" % dtype, F32(w[0]), "range"))
    return c


def negative_ties(dtype):
    """every negative float32 that is a tie of the storage type"""
    if dtype == "bf16":
        return from_bits((np.arange(0x8000, 0xff7f, dtype=np.uint32) << 16) | 0x8000)
    normal = from_bits(((np.arange(113, 143, dtype=np.uint32)[:, None] << 23) | (np.arange(1024, dtype=np.uint32)[None, :] << 13)
                        | 0x80001000).ravel())
    return np.concatenate([(-(np.arange(1024) + 0.5) * 2.0 ** -24).astype(np.float32), normal])


def slope_witnesses(dtype):
    """negative t for which 0.1f * t and float32(0.1 * t) (a double slope, narrowed afterwards) are stored differently.

    float32: a fifth of all t.  16-bit: the two float32 products are equal or neighbours, so they round apart only when one of
    them IS a storage tie T; then t lies within a few float32 steps of T / 0.1 (a step of t moves the product by 0.8 or 1.6 of
    its ulps), so the search below over every tie and 12 steps either way is exhaustive.  In float32's normal range it finds
    nothing: 10 T has few enough bits to be a float32, both slopes take it to T itself, and its neighbours land 0.8 ulp and
    more away.  Only where the product is a float32 subnormal, which bf16 keeps and fp16 does not have, do the two slopes
    round apart at a tie: bf16 has witnesses (near 1e-39), fp16 has none at all."""
    if dtype == "float32":
        cand = step(np.full(4096, F32(-10.0)), -np.arange(4096))
    else:
        with np.errstate(all="ignore"):
            t0 = (negative_ties(dtype) / SLOPE).astype(np.float32)
        t0 = t0[np.isfinite(t0) & (np.abs(t0) > 1e-43)]
        cand = np.concatenate([step(t0, n) for n in range(-12, 13)])
        cand = cand[np.isfinite(cand) & (cand < 0)]
    return cand[RND[dtype](leaky_f32(cand)) != RND[dtype](leaky_double_slope(cand))]


MISH_MIN = F32(-1.1924)
_MISH = (30.0, 43.0, 44.0, 44.5, 88.0, 89.0, 1e30)
_MISH_NEG = (-0.3, -5.0, -10.0, -17.0, -20.0, -50.0, -87.0, -88.0, -90.0, -103.0, -104.0, -200.0, -1e30)
_LOGISTIC = (16.6, 17.0, 20.0, 87.0, 88.7, 89.0, 104.0)


def _mish_extra():
    c = [Case("mish switch: 20.0", F32(20.0), "threshold"), Case("mish switch: just above 20", F32(step(F32(20.0), 1)), "sat"),
         Case("mish switch: just below 20", F32(step(F32(20.0), -1)), "threshold")]
    c += [Case("mish %g (past the switch)" % v, F32(v), "sat") for v in _MISH]
    c.append(Case("mish minimum near -1.1924", MISH_MIN, "range"))
    c += [Case("mish %g" % v, F32(v), "range") for v in _MISH_NEG]
    # between the planted edges, every half from -4.5 to 19.5: each a different exponential argument, and where the 16-bit
    # either-side rule allows one storage value only
    have = set(float(e.t) for e in c) | set(float(e.t) for e in _common())
    for v in np.arange(-4.5, 20.0, 0.5):
        if float(v) in have:
            continue
        for k in range(8):      # moved by a few float32 steps where the rule would allow two values of either 16-bit type
            t = F32(step(F32(v), k))
            if all(bits(lo) == bits(hi) for lo, hi, _ in (expect("mish", d, t) for d in ("bf16", "fp16"))):
                c.append(Case("mish sweep %g%s" % (v, " +%d steps" % k if k else ""), t, "range"))
                break
    return c


def _logistic_extra():
    c = []
    for v in _LOGISTIC:
        c.append(Case("logistic +%g" % v, F32(v), "sat" if v >= 17 else "range"))
        c.append(Case("logistic -%g" % v, F32(-v), "sat" if v >= 104 else "range"))
    return c


_CASES = {}


def cases(act):
    if act not in _CASES:
        extra = {"linear": list, "leaky": _leaky_extra, "mish": _mish_extra, "logistic": _logistic_extra}[act]()
        common = _common()
        if act in ("mish", "logistic"):     # a tie of the linear result is an ordinary argument to these two
            common = [e if e.kind == "nonfinite" else e._replace(kind="range") for e in common]
        _CASES[act] = tuple(common + extra)
        assert len(_CASES[act]) <= LIST_LEN
    return _CASES[act]


# ---- expected values -------------------------------------------------------------------------------------------------------
def act_exact(act, t):
    """linear / leaky in float32, one correctly rounded operation"""
    return f32(t) if act == "linear" else leaky_f32(t)


def want64(act, t):
    """mish / logistic in float64 of the exact float32 t, in a form that neither overflows nor cancels"""
    x = f32(t).astype(np.float64)
    with np.errstate(all="ignore"):
        if act == "mish":
            sp = np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))
            return x * np.tanh(sp)
        e = np.exp(-np.abs(x))
        return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def ulp32(x64):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.spacing(np.abs(np.asarray(x64, dtype=np.float64).astype(np.float32))).astype(np.float64)


def bound(w64):
    """the project's float32 bound on mish / logistic: 4 float32 ulp or 1e-6"""
    return np.maximum(4.0 * ulp32(w64), 1e-6)


def saturated(act, t):
    """(mask, value): entries the documented formula gives exactly.  mish(t) == t above 20 (the select); logistic == 1 from
    17 up (e^-t is below half an ulp of 1) and == 0 from -104 down (e^-t is inf in float32, its reciprocal 0)"""
    t = f32(t)
    with np.errstate(invalid="ignore"):
        if act == "mish":
            return t > 20, t
        return (t >= 17) | (t <= -104), np.where(t >= 17, F32(1), F32(0)).astype(np.float32)


def _inward_f32(lo64, hi64):
    """the float32 interval inside [lo64, hi64]"""
    with np.errstate(over="ignore", invalid="ignore"):
        lo = lo64.astype(np.float32)
        lo = np.where(lo.astype(np.float64) < lo64, np.nextafter(lo, F32(np.inf)), lo)
        hi = hi64.astype(np.float32)
        hi = np.where(hi.astype(np.float64) > hi64, np.nextafter(hi, F32(-np.inf)), hi)
    return lo.astype(np.float32), hi.astype(np.float32)


def expect(act, dtype, t, r=None, fused=True):
    """(lo, hi, nan) float32 arrays: the stored result of pre-activation t (and shortcut operand r) must be NaN where ``nan``,
    the bits of lo where lo and hi have the same bits, in [lo, hi] otherwise.

    linear / leaky: out = rnd(a), rnd(float32(a + r)) fused, rnd(float32(rnd(a) + r)) when the add is its own kernel.
    mish / logistic: every storage value a float32 result within b = max(4 ulp, 1e-6) of the float64 function can round to,
    rnd(want64 - b) .. rnd(want64 + b); with a fused shortcut want64 + r and b + one float32 ulp of the sum."""
    t = f32(t)
    rnd = RND[dtype]
    r = None if r is None else f32(r)
    with np.errstate(all="ignore"):
        if act in ("linear", "leaky"):
            lo = hi = _exact_tail(rnd, act_exact(act, t), r, fused)
        else:
            w = want64(act, t)
            b = bound(w)
            sat, val = saturated(act, t)
            if r is None or not fused:
                if dtype == "float32":
                    lo, hi = _inward_f32(w - b, w + b)
                else:
                    lo, hi = rnd64(dtype, w - b), rnd64(dtype, w + b)
                lo = np.where(sat, rnd(val), lo)
                hi = np.where(sat, rnd(val), hi)
                if r is not None:
                    lo, hi = rnd((lo + r).astype(np.float32)), rnd((hi + r).astype(np.float32))
            else:
                s = w + r.astype(np.float64)
                bs = b + ulp32(s)
                if dtype == "float32":
                    lo, hi = _inward_f32(s - bs, s + bs)
                else:
                    lo, hi = rnd64(dtype, s - bs), rnd64(dtype, s + bs)
                ex = rnd((val + r).astype(np.float32))
                lo = np.where(sat, ex, lo)
                hi = np.where(sat, ex, hi)
        lo, hi = lo.astype(np.float32), hi.astype(np.float32)
        nan = np.isnan(lo) | np.isnan(hi)
    return lo, hi, nan


def _exact_tail(rnd, a, r, fused):
    if r is None:
        return rnd(a)
    if fused:
        return rnd((a + r).astype(np.float32))
    return rnd((rnd(a) + r).astype(np.float32))


def check(lo, hi, nan, got):
    """mask of the values of ``got`` (float32) that miss their expectation"""
    got = f32(got)
    exact = bits(lo) == bits(hi)
    with np.errstate(invalid="ignore"):
        ok = np.where(nan, np.isnan(got), np.where(exact, bits(got) == bits(lo), (got >= lo) & (got <= hi)))
    return ~ok


# ---- shortcut operands -----------------------------------------------------------------------------------------------------
SHORTCUT_KINDS = ("witness", "tie", "inexact", "cancel", "inf", "nan", "overflow", "witness negative a")


def _is_tie_normal(dtype, x):
    """is_tie for arrays of finite values in the storage type's normal range"""
    a = bits(x) & 0x7fffffff
    return (a & 0xffff) == 0x8000 if dtype == "bf16" else ((a & 0x1fff) == 0x1000) & (a >= 0x38800000)


def shortcut_cases(act, dtype, r, seed):
    """pre-activations t (one per channel) of a linear / leaky conv whose fused shortcut operand is the known storage value r:
    by channel, the kinds of SHORTCUT_KINDS, each found among 64 random candidates and verified here; a kind that this r
    cannot give (no tie in float32, an r too small to overflow, ...) is planted as a random value and tagged "plain"."""
    assert act in ("linear", "leaky")
    rnd = RND[dtype]
    rng = np.random.RandomState(seed)
    r = f32(r)
    n, tries = r.size, 64
    kind_of = np.arange(n) % len(SHORTCUT_KINDS)
    mag = np.where((np.abs(r) >= 1e-3) & (np.abs(r) <= 1e4), np.abs(r), F32(1)).astype(np.float32)
    u = rng.uniform(0.25, 4.0, (n, tries))
    t_pos = (mag[:, None] * u).astype(np.float32)
    t_neg = (-t_pos / SLOPE).astype(np.float32) if act == "leaky" else -t_pos
    rc = r[:, None]
    t = t_pos[:, 0].copy()
    tags = ["shortcut: plain"] * n

    def pre(a):          # t with act(t) == a
        a = F32(a)
        return a if (act == "linear" or a > 0) else leaky_preimage(a)

    def first(k, ok, cand):
        rows = np.nonzero(kind_of == k)[0]
        hit = ok[rows]
        for c, h, col in zip(rows, hit.any(axis=1), hit.argmax(axis=1)):
            if h:
                t[c], tags[c] = cand[c, col], "shortcut: " + SHORTCUT_KINDS[k]

    with np.errstate(all="ignore"):
        for k, cand in ((0, t_pos), (7, t_neg)):                       # witness, witness negative a
            a = act_exact(act, cand)
            one, two = rnd((a + rc).astype(np.float32)), rnd((rnd(a) + rc).astype(np.float32))
            first(k, np.isfinite(one) & np.isfinite(two) & (one != two), cand)
        if dtype != "float32":                                         # tie: a + r exact and halfway between v and the next value
            v = rnd((np.maximum(np.abs(rc), 1) * rng.uniform(2.0, 4.0, (n, tries))).astype(np.float32))
            v = np.where(np.isfinite(v) & (v < 3e38), v, F32(2))
            tie = ((v.astype(np.float64) + step(v, 1 << DROPPED[dtype]).astype(np.float64)) / 2).astype(np.float32)
            a = (tie - rc).astype(np.float32)
            ok = (a > 0) & (a.astype(np.float64) + rc.astype(np.float64) == tie.astype(np.float64)) & _is_tie_normal(dtype, tie)
            first(1, ok & np.isfinite(rnd(a)), a)
        a = act_exact(act, t_pos)                                      # inexact
        first(2, a.astype(np.float64) + rc.astype(np.float64) != (a + rc).astype(np.float32).astype(np.float64), t_pos)
        for c in range(n):
            kind, got = SHORTCUT_KINDS[kind_of[c]], None
            if kind == "cancel" and r[c] != 0:
                got = pre(-r[c])
            elif kind == "inf":
                got = F32(np.inf)
            elif kind == "nan":
                got = F32(np.nan)
            elif kind == "overflow" and r[c] != 0:
                m = STORE_MAX[dtype]
                for a in (m, m if dtype == "float32" else step(m, (1 << (DROPPED[dtype] - 1)) - 1)):
                    a = F32(a if r[c] > 0 else -a)
                    if np.isfinite(rnd(a)) and np.isinf(rnd(F32(a + r[c]))):
                        got = pre(a)
                        break
            if got is not None:
                t[c], tags[c] = got, "shortcut: " + kind
    return t, tags


def shortcut_tag_holds(tag, act, dtype, t, r):
    """whether the property a shortcut tag names is true of (t, r)"""
    rnd = RND[dtype]
    kind = tag[len("shortcut: "):]
    with np.errstate(all="ignore"):
        a = act_exact(act, F32(t))
        s = F32(a + F32(r))
        if kind.startswith("witness"):
            return bool(rnd(s) != rnd(F32(rnd(a) + F32(r)))) and (kind == "witness" or bool(a < 0))
        if kind == "tie":
            return float(a) + float(r) == float(s) and is_tie(dtype, s)
        if kind == "inexact":
            return float(a) + float(r) != float(s)
        if kind == "cancel":
            return bool(a == -F32(r)) and bool(s == 0)
        if kind == "inf":
            return bool(np.isinf(a) and np.isinf(rnd(s)))
        if kind == "nan":
            return bool(np.isnan(rnd(s)))
        if kind == "overflow":
            return bool(np.isfinite(rnd(a)) and np.isfinite(r) and np.isinf(rnd(s)))
    return kind == "plain"


# ---- channel layout of the GPU test ----------------------------------------------------------------------------------------
def padded(act):
    """the list repeated to LIST_LEN entries: (t, index into cases(act))"""
    cs = cases(act)
    idx = np.arange(LIST_LEN) % len(cs)
    return np.asarray([cs[i].t for i in idx], dtype=np.float32), idx


def offset(run, layer):
    """first list entry of channel 0.  Layers of 128 channels and more hold the whole list whatever the offset; the offset steps
    by 32 entries from run to run, so the 32-channel stem has met the whole list after four runs and the 64-channel block
    after three (runs 0 and 2), and every layer is shifted by 5 entries against the one before, so an entry meets different
    lanes of the eight-channel epilogue groups."""
    return (32 * run + 5 * layer) % LIST_LEN


def layer_values(act, run, layer, channels):
    """(t, case index) per channel of conv block ``layer`` in run number ``run``"""
    t, idx = padded(act)
    sel = (np.arange(channels) + offset(run, layer)) % LIST_LEN
    return t[sel], idx[sel]


def finite_only(act, dtype, t):
    """t with every entry whose stored result may be non-finite replaced by FILLER: what the layers BEFORE the checked one
    carry, so that the checked conv reads finite activations (0 * inf is NaN)"""
    lo, hi, nan = expect(act, dtype, t)
    bad = nan | ~np.isfinite(lo) | ~np.isfinite(hi)
    return np.where(bad, FILLER, f32(t)).astype(np.float32)


# conv blocks of the family network with a shortcut after them -> the block whose output is the operand
RESIDUAL_FROM = {4: 2, 8: 7}


def shortcut_operand(act, dtype, run, src_layer, channels):
    """linear / leaky: the stored output of block ``src_layer`` under its finite_only list, the operand r of the shortcut"""
    t = finite_only(act, dtype, layer_values(act, run, src_layer, channels)[0])
    lo, hi, nan = expect(act, dtype, t)
    assert not nan.any() and (bits(lo) == bits(hi)).all()
    return lo


def residual_layer(act, dtype, run, layer, channels):
    """(t, tags, r) of residual conv block ``layer``, linear / leaky: the searched shortcut cases against the known operand"""
    r = shortcut_operand(act, dtype, run, RESIDUAL_FROM[layer], channels)
    t, tags = shortcut_cases(act, dtype, r, 1000 * run + layer)
    return t, tags, r
