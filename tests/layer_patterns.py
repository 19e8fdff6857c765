"""Storage patterns, references and the case table for the memory-bound layer kernels (csrc/layers.hip): max-pool in every form,
nearest upsample, add and channel-slice copy.  numpy and torch-CPU only; tensors are NHWC arrays of unsigned storage patterns
(uint16 for bf16 / fp16, uint32 for float32), never floats, so that -0, subnormals, infinities and NaN payloads stay what they are.

The rule the kernels are held to ("The layer kernels on every storage pattern"):

  max pools     IEEE 754-2019 ``maximum`` of the taps that count, on stored values: +0 beats -0, the winner's bits come back
                unchanged.  A NaN tap is left out (Darknet's ``val > max``).  A window whose counting taps are all NaN gives
                -inf; under the reference's padding rule a padded tap is a +0 tap, so such a window gives +0.
  upsample/copy the pattern comes back (16-bit types: a NaN comes back as some NaN, the kernels go through float).
  add           (a.float() + b.float()) rounded once to the storage type, to nearest even; a NaN result is some NaN.

``key`` maps an ordered (non-NaN) pattern to an integer whose order is the ``maximum`` order: sign-magnitude to two's complement
with -0 = -1 just below +0 = 0.  The pool reference is stated twice: ``pool_keys`` (integer max over keys with sliding windows,
NaN taps masked to the key of -inf, the border as a key) and ``pool_taps`` (an explicit tap loop on float values with the rule
spelled out).  ``pool_taps`` takes the update rule as an argument; the WRONG_* rules are what tests/test_layer_patterns_host.py
uses to show that the cases tell the rule from its neighbours.
"""
import functools

import numpy as np
import torch

DTYPES = ("float32", "bf16", "fp16")
#            bits, mantissa bits, +inf pattern, torch type, kernel name tag
_INFO = {"float32": (32, 23, 0x7F800000, torch.float32, "f32"),
         "bf16": (16, 7, 0x7F80, torch.bfloat16, "bf16"),
         "fp16": (16, 10, 0x7C00, torch.float16, "f16")}
SEED = 20251


def bits(dtype):
    return _INFO[dtype][0]


def man_bits(dtype):
    return _INFO[dtype][1]


def inf_bits(dtype):
    return _INFO[dtype][2]


def torch_dtype(dtype):
    return _INFO[dtype][3]


def tag(dtype):
    return _INFO[dtype][4]


def utype(dtype):
    return np.uint32 if bits(dtype) == 32 else np.uint16


def itype(dtype):
    return np.int32 if bits(dtype) == 32 else np.int16


def sign_bit(dtype):
    return 1 << (bits(dtype) - 1)


def neg_inf(dtype):
    return inf_bits(dtype) | sign_bit(dtype)


def is_nan(p, dtype):
    return (np.asarray(p).astype(np.int64) & (sign_bit(dtype) - 1)) > inf_bits(dtype)


def boundary(dtype):
    """{name: pattern}: the values every form must be able to return (test_layer_patterns_host.py: coverage)"""
    s, m, inf = sign_bit(dtype), man_bits(dtype), inf_bits(dtype)
    pos = {"zero": 0, "sub_min": 1, "sub_max": (1 << m) - 1, "norm_min": 1 << m, "max": inf - 1, "inf": inf}
    out = {}
    for name, p in pos.items():
        out["+" + name], out["-" + name] = p, p | s
    return out


# ---- pattern sets ----------------------------------------------------------------------------------------------------------

def to_torch(p, dtype):
    """patterns -> a torch-CPU tensor of the storage type holding them"""
    p = np.array(p, dtype=utype(dtype), order="C")                  # a copy: the shared maps are read-only
    return torch.from_numpy(p.view(itype(dtype))).view(torch_dtype(dtype))


def from_torch(t):
    """a torch tensor of a storage type -> its patterns"""
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def _widened(dtype):
    vals = np.array(sorted(set(boundary(dtype).values())), dtype=utype(dtype))
    return from_torch(to_torch(vals, dtype).float())


@functools.lru_cache(None)
def planted_f32():
    """the planted float32 list: zeros, subnormal edges, FLT_MIN, neighbours of 1 / 65504 / FLT_MAX, FLT_MAX, inf, of each sign,
    and every bf16 and fp16 boundary value widened"""
    pos = [0x00000000, 0x00000001, 0x00000002, 0x007FFFFE, 0x007FFFFF, 0x00800000, 0x00800001,
           0x3F7FFFFF, 0x3F800000, 0x3F800001, 0x477FDFFF, 0x477FE000, 0x477FE001, 0x7F7FFFFE, 0x7F7FFFFF, 0x7F800000]
    pats = set(pos) | set(p | 0x80000000 for p in pos)
    pats |= set(int(v) for v in _widened("bf16")) | set(int(v) for v in _widened("fp16"))
    return np.array(sorted(pats), dtype=np.uint32)


@functools.lru_cache(None)
def ordered(dtype):
    """every non-NaN pattern of a 16-bit type; for float32 the planted list and 4096 seeded random non-NaN patterns"""
    if bits(dtype) == 16:
        p = np.arange(1 << 16, dtype=np.uint32)
        return p[~is_nan(p, dtype)].astype(np.uint16)
    rnd = np.random.default_rng(SEED).integers(0, 1 << 32, size=6000, dtype=np.uint64).astype(np.uint32)
    rnd = rnd[~is_nan(rnd, dtype)][:4096]
    assert rnd.size == 4096
    return np.unique(np.concatenate([planted_f32(), rnd]))


@functools.lru_cache(None)
def nans(dtype):
    """NaN patterns: all of a 16-bit type; for float32 both signs, quiet and signalling payloads"""
    if bits(dtype) == 16:
        p = np.arange(1 << 16, dtype=np.uint32)
        return p[is_nan(p, dtype)].astype(np.uint16)
    return np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FBFFFFF, 0xFFBFFFFF, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA5A5A5,
                     0xFFD5A5A5], dtype=np.uint32)


def key(p, dtype):
    """ordered pattern -> int64 whose order is the ``maximum`` order (-0 = -1 just below +0 = 0)"""
    p = np.asarray(p).astype(np.int64)
    mag = p & (sign_bit(dtype) - 1)
    return np.where(p & sign_bit(dtype), -mag - 1, mag)


def unkey(k, dtype):
    k = np.asarray(k, dtype=np.int64)
    return np.where(k < 0, (-k - 1) | sign_bit(dtype), k).astype(utype(dtype))


def to_float(p, dtype):
    """patterns -> numpy float32 values (exact)"""
    p = np.ascontiguousarray(p, dtype=utype(dtype))
    if dtype == "float32":
        return p.view(np.float32)
    if dtype == "bf16":
        return (p.astype(np.uint32) << 16).view(np.float32)
    return p.view(np.float16).astype(np.float32)


def rne(f, dtype):
    """float32 values -> patterns of the storage type, one rounding to nearest even, in integer arithmetic for bf16 and by numpy
    for fp16 (``add_torch`` rounds with torch: two libraries, one rule)"""
    f = np.ascontiguousarray(f, dtype=np.float32)
    u = f.view(np.uint32)
    if dtype == "float32":
        return u.copy()
    if dtype == "bf16":
        r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
        return np.where(np.isnan(f), np.uint16(0x7FC0), r).astype(np.uint16)
    with np.errstate(over="ignore"):
        return f.astype(np.float16).view(np.uint16).copy()


def canon_nan(p, dtype):
    """every NaN pattern replaced by one quiet NaN: what is compared where the rule says "some NaN" """
    p = np.asarray(p, dtype=utype(dtype))
    return np.where(is_nan(p, dtype), utype(dtype)(inf_bits(dtype) | (1 << (man_bits(dtype) - 1))), p).astype(utype(dtype))


# ---- input maps ------------------------------------------------------------------------------------------------------------

def _rng(*what):
    return np.random.default_rng([SEED] + [sum(ord(ch) * (i + 1) for i, ch in enumerate(str(w))) for w in what])


def lay(flat, shape):
    """a flat list laid over (B, H, W, C), repeated from its start when the map is larger"""
    return np.resize(np.asarray(flat), shape)


def map_perm(dtype, shape):
    """every ordered pattern in a seeded permutation.  -0 has a fixed place, (1, 1) of frame 0 in channel 0, and is not repeated
    where the list is: no window that holds it there reaches the reference's padding, so the map has no window whose joint
    maximum is both zeros by padding (torch's pool, which the ordered maps are held to, resolves that tie by scan order), and
    one by two neighbouring zeros would take a -0 beside a +0 with nothing positive around (the host test asserts there is none)."""
    o = ordered(dtype)
    m = lay(_rng("perm", dtype).permutation(o[o != sign_bit(dtype)]), shape)
    m[0, 1, 1, 0] = sign_bit(dtype)
    return m


def map_neighbours(dtype, shape):
    """sorted by key; channel c takes the run of B*H*W patterns that starts at c*B*H*W, ascending over the pixels in even
    channels and descending in odd ones: taps next to each other hold adjacent patterns, and the winning tap of a window is
    its last in even channels and its first in odd ones.  -0 is left out of this arrangement (the permutation holds it, and the
    zeros maps are about it): next to +0 it makes windows whose joint maximum is both zeros, and the ordered maps are held to
    torch's pool without exception, which resolves that tie by scan order."""
    srt = ordered(dtype)[ordered(dtype) != sign_bit(dtype)]
    srt = srt[np.argsort(key(srt, dtype), kind="stable")]
    b, h, w, c = shape
    px = b * h * w
    i = np.arange(px, dtype=np.int64)[:, None]
    ch = np.arange(c, dtype=np.int64)[None, :]
    idx = ch * px + np.where(ch % 2 == 0, i, px - 1 - i)
    return srt[idx % srt.size].reshape(shape)


def map_zeros(dtype, shape):
    """negative ordered patterns, about 30 % of them -0, and a few +0"""
    r = _rng("zeros", dtype)
    neg = ordered(dtype)[(ordered(dtype) & utype(dtype)(sign_bit(dtype))) != 0]
    m = r.choice(neg, size=shape)
    u = r.random(shape)
    m = np.where(u < 0.30, utype(dtype)(sign_bit(dtype)), m)
    return np.where(u > 0.995, utype(dtype)(0), m).astype(utype(dtype))


LONE_AT = 8        # the lone taps sit at rows / columns 8 and 9: inside a window of every size on every map here
NAN_BLOCK = (2, 3, 13)


def map_nan(dtype, shape):
    """three frames.  0: ordered patterns with about 2 % NaN and one 13 x 13 block (the largest window) of NaN only at (2, 3);
    1: NaN only but for one tap per channel, channel j holding boundary value j % 12 at (8 + (j & 1), 8 + (j >> 1 & 1)), so
    that every boundary value wins a window as its only non-NaN tap and every tap position of a 2 x 2 window does; 2: NaN only"""
    b, h, w, c = shape
    assert b == 3 and h >= 16 and w >= 16
    r = _rng("nan", dtype)
    m = np.empty(shape, dtype=utype(dtype))
    m[0] = r.choice(ordered(dtype), size=shape[1:])
    some = r.choice(nans(dtype), size=shape[1:])
    m[0] = np.where(r.random(shape[1:]) < 0.02, some, m[0])
    y, x, n = NAN_BLOCK
    m[0, y:y + n, x:x + n] = some[y:y + n, x:x + n]
    m[1:] = r.choice(nans(dtype), size=(2,) + tuple(shape[1:]))
    lone = list(boundary(dtype).values())
    for j in range(c):
        m[1, LONE_AT + (j & 1), LONE_AT + ((j >> 1) & 1), j] = lone[j % len(lone)]
    return m


def map_all(dtype, shape):
    """every pattern of the set, NaN included, in a seeded permutation (upsample, copy)"""
    return lay(_rng("all", dtype).permutation(np.concatenate([ordered(dtype), nans(dtype)])), shape)


# ---- max-pool references ---------------------------------------------------------------------------------------------------

def pool_geometry(h, w, k, s, darknet):
    """(out_h, out_w, pad_lo, pad_hi): the reference pads k - 1 right / bottom at stride 1, Darknet's rule (padding k - 1) pads
    (k - 1) / 2 left / top and the rest right / bottom"""
    if darknet:
        p = k - 1
        return (h + p - k) // s + 1, (w + p - k) // s + 1, p // 2, p - p // 2
    if s == 1 and k > 1:
        return h, w, 0, k - 1
    return (h - k) // s + 1, (w - k) // s + 1, 0, 0


def _windows_max(a, k, s, oh, ow):
    """max over k x k windows at stride s of the (B, H', W', C) integer array a, rows then columns"""
    v = np.lib.stride_tricks.sliding_window_view(a, k, axis=2).max(axis=-1)
    v = np.lib.stride_tricks.sliding_window_view(v, k, axis=1).max(axis=-1)
    return v[:, ::s, ::s][:, :oh, :ow]


def pool_keys(p, dtype, k, s, darknet):
    """statement one: integer max over keys.  A NaN tap is masked to the key of -inf (left out, and -inf when nothing is left);
    the border is the key of -inf under Darknet's rule and of +0 under the reference's."""
    b, h, w, c = p.shape
    oh, ow, lo, hi = pool_geometry(h, w, k, s, darknet)
    least = int(key(neg_inf(dtype), dtype))
    kk = np.where(is_nan(p, dtype), least, key(p, dtype))
    kk = np.pad(kk, ((0, 0), (lo, hi), (lo, hi), (0, 0)), constant_values=least if darknet else 0)
    return unkey(_windows_max(kk, k, s, oh, ow), dtype)


def rule_maximum(best, best_set, v, counts):
    """the rule: a NaN tap is left out; a larger value wins, and +0 wins over -0"""
    ok = counts & ~np.isnan(v)
    better = (v > best) | ((v == best) & np.signbit(best) & ~np.signbit(v))
    take = ok & (better | ~best_set)
    return np.where(take, v, best), best_set | ok


def wrong_ge_cascade(best, best_set, v, counts):
    """``x >= y ? x : y`` with x the running value: -0 beats a later +0, a NaN in x is dropped, a NaN in y is kept"""
    with np.errstate(invalid="ignore"):
        keep = best_set & (best >= v)
    take = counts & ~keep
    return np.where(take, v, best), best_set | counts


def wrong_gt(best, best_set, v, counts):
    """``a > b ? a : b`` with a the running value: a later -0 replaces +0, a NaN tap replaces everything before it"""
    with np.errstate(invalid="ignore"):
        keep = best_set & (best > v)
    take = counts & ~keep
    return np.where(take, v, best), best_set | counts


def wrong_nan_propagates(best, best_set, v, counts):
    """torch's pool: a NaN tap makes the window NaN"""
    nb, ns = rule_maximum(best, best_set, v, counts)
    bad = counts & np.isnan(v)
    nb = np.where(bad | (best_set & np.isnan(best)), np.float32(np.nan), nb)
    return nb, ns | bad


def wrong_bf16_compare(best, best_set, v, counts):
    """float32 values compared after truncation to bf16: the first of two values that share 16 leading bits wins"""
    def cut(f):
        return (np.ascontiguousarray(f, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    ok = counts & ~np.isnan(v)
    take = ok & ((cut(v) > cut(best)) | ~best_set)
    return np.where(take, v, best), best_set | ok


def pool_taps(p, dtype, k, s, darknet, rule=rule_maximum, fixed_tap=None, flush=False):
    """statement two: the tap loop on float values.  Taps are visited row by row; under the reference's rule a tap outside the
    map is a +0 tap, under Darknet's it is left out.  A window in which nothing counted gives -inf.  ``fixed_tap`` (ky, kx)
    returns that tap whatever the others hold, ``flush`` reads subnormal inputs as zeros of their sign: wrong on purpose."""
    b, h, w, c = p.shape
    oh, ow, lo, hi = pool_geometry(h, w, k, s, darknet)
    f = to_float(p, dtype)
    if flush:
        sub = (np.abs(f) < np.float32(2.0 ** (-126 if dtype != "fp16" else -14))) & (f != 0)
        f = np.where(sub, np.copysign(np.float32(0), f), f).astype(np.float32)
    fp = np.pad(f, ((0, 0), (lo, hi), (lo, hi), (0, 0)), constant_values=0.0)
    inside = np.pad(np.ones((1, h, w, 1), dtype=bool), ((0, 0), (lo, hi), (lo, hi), (0, 0)), constant_values=False)
    best = np.full((b, oh, ow, c), -np.inf, dtype=np.float32)
    best_set = np.zeros((b, oh, ow, c), dtype=bool)
    for ky in range(k):
        for kx in range(k):
            ys, xs = slice(ky, ky + (oh - 1) * s + 1, s), slice(kx, kx + (ow - 1) * s + 1, s)
            v = fp[:, ys, xs]
            counts = np.broadcast_to(inside[:, ys, xs] | (not darknet), v.shape)
            if fixed_tap is not None:
                if (ky, kx) == fixed_tap:
                    best, best_set = v.copy(), np.ones_like(best_set)
                continue
            with np.errstate(invalid="ignore"):
                best, best_set = rule(best, best_set, v, counts)
    return rne(best, dtype)


def pool_stats(p, dtype, k, s, darknet, taps=None):
    """per window (B, Ho, Wo, C): ``nan`` a NaN among its taps inside the map, ``tie`` both zeros among the taps that share the
    maximum (a padded tap of the reference's rule is a +0 tap), ``empty`` no non-NaN tap inside the map, ``winner`` the
    winner's key.  With ``taps`` (the windows are laid out tap by tap, so for small k only) also ``adjacent``: the key distance
    of winner and runner-up where both are non-NaN taps inside the map (else -1), and ``lone``: the tap position ky * k + kx
    of the windows whose only non-NaN tap inside the map won (else -1)."""
    b, h, w, c = p.shape
    oh, ow, lo, hi = pool_geometry(h, w, k, s, darknet)
    least = int(key(neg_inf(dtype), dtype))
    nan = is_nan(p, dtype)
    kk = np.where(nan, least, key(p, dtype))
    pad = ((0, 0), (lo, hi), (lo, hi), (0, 0))
    kp = np.pad(kk, pad, constant_values=least if darknet else 0)
    top = _windows_max(kp, k, s, oh, ow)
    has_nan = _windows_max(np.pad(nan, pad, constant_values=False), k, s, oh, ow)
    neg_zero = _windows_max(np.pad(~nan & (kk == -1), pad, constant_values=False), k, s, oh, ow)
    realp = np.pad(~nan, pad, constant_values=False)             # a non-NaN tap inside the map
    out = dict(nan=has_nan, tie=(top == 0) & neg_zero, empty=~_windows_max(realp, k, s, oh, ow), winner=top)
    if not taps:
        return out

    def win(a):
        v = np.lib.stride_tricks.sliding_window_view(a, (k, k), axis=(1, 2))[:, ::s, ::s][:, :oh, :ow]
        return v.reshape(v.shape[:4] + (k * k,))
    wk, wreal = win(kp), win(realp)
    srt = np.sort(np.where(wreal, wk, np.iinfo(np.int64).min), axis=-1)
    both = wreal.sum(axis=-1) >= 2
    out["adjacent"] = np.where(both & (srt[..., -1] == top), srt[..., -1] - srt[..., -2], -1)
    lone = np.where(wreal.sum(axis=-1) == 1, wreal.argmax(axis=-1), -1)
    out["lone"] = np.where((lone >= 0) & (np.take_along_axis(wk, np.maximum(lone, 0)[..., None], -1)[..., 0] == top), lone, -1)
    return out


# ---- upsample, copy, add ---------------------------------------------------------------------------------------------------

def upsample_gather(p, s):
    """out[b, y, x] = in[b, y / s, x / s] on the patterns"""
    b, h, w, c = p.shape
    return p[:, np.arange(h * s) // s][:, :, np.arange(w * s) // s]


def upsample_repeat(p, s):
    return np.repeat(np.repeat(p, s, axis=1), s, axis=2)


def add_torch(a, b, dtype):
    """the torch float32 sum narrowed once"""
    return from_torch((to_torch(a, dtype).float() + to_torch(b, dtype).float()).to(torch_dtype(dtype)))


def add_numpy(a, b, dtype):
    with np.errstate(all="ignore"):
        return rne(to_float(a, dtype) + to_float(b, dtype), dtype)


def wrong_add_through_fp16(a, b, dtype):
    """the sum rounded to fp16 first, then to the storage type"""
    with np.errstate(all="ignore"):
        once = (to_float(a, dtype) + to_float(b, dtype)).astype(np.float16).astype(np.float32)
    return rne(once, dtype)


def wrong_add_operands_through_fp16(a, b, dtype):
    """each operand narrowed to fp16 before the sum"""
    with np.errstate(all="ignore"):
        fa, fb = (to_float(v, dtype).astype(np.float16).astype(np.float32) for v in (a, b))
        return rne(fa + fb, dtype)


def wrong_add_rereads_output(a, b, dtype):
    """an in-place add that reads a after having written it"""
    return add_numpy(add_numpy(a, b, dtype), b, dtype)


SECOND = ("+0", "-0", "+sub_min", "-sub_min", "negation", "+half_ulp", "-half_ulp", "+3half_ulp", "-3half_ulp",
          "+65504", "-65504", "+bf16_max", "-bf16_max", "+inf", "-inf", "nan")


def add_second(a, which, dtype):
    """the second operand ``which`` of SECOND for every element of a (16-bit types).  half_ulp: half the distance from a to its
    neighbour away from zero, which makes a + b a tie between a and that neighbour (3half_ulp: between the next two), to be
    broken towards the even one: both parities occur, since a runs over every pattern.  Where half an ulp is below the smallest
    subnormal it narrows to what the type holds; 65504 and the largest bf16 narrow to the type too (inf in the other type)."""
    a = np.asarray(a, dtype=utype(dtype))
    s = sign_bit(dtype)
    const = {"+0": 0, "-0": s, "+sub_min": 1, "-sub_min": s | 1, "+inf": inf_bits(dtype), "-inf": neg_inf(dtype),
             "nan": inf_bits(dtype) | (1 << (man_bits(dtype) - 1)) | 1}
    if which in const:
        return np.full(a.shape, const[which], dtype=utype(dtype))
    if which == "negation":
        return a ^ utype(dtype)(s)
    if which[1:] in ("65504", "bf16_max"):
        v = 65504.0 if which[1:] == "65504" else float(to_float(np.array([0x7F7F], dtype=np.uint16), "bf16")[0])
        t = torch.tensor([v if which[0] == "+" else -v], dtype=torch.float32).to(torch_dtype(dtype))
        return np.full(a.shape, from_torch(t)[0], dtype=utype(dtype))
    m = man_bits(dtype)
    fa = np.abs(to_float(a, dtype))
    with np.errstate(all="ignore"):
        e = np.floor(np.log2(np.where((fa > 0) & np.isfinite(fa), fa, 1.0).astype(np.float64)))
    e = np.maximum(e, -126 if dtype == "bf16" else -14)              # subnormals share the smallest normal's ulp
    half = np.ldexp(1.0, (e - m - 1).astype(np.int64)) * (3.0 if "3" in which else 1.0)
    half = np.where(which[0] == "+", half, -half).astype(np.float32)
    return from_torch(torch.from_numpy(half).to(torch_dtype(dtype)))


def add_cases(dtype, shape):
    """[(name, a, b)] patterns laid over ``shape``.  16-bit: every ordered pattern (the seeded permutation) against each second
    operand of SECOND; float32: the planted list against itself, every pair."""
    if bits(dtype) == 16:
        a = map_perm(dtype, shape)
        return [(w, a, add_second(a, w, dtype)) for w in SECOND]
    pl = planted_f32()
    n = pl.size
    assert n * n <= int(np.prod(shape))
    return [("planted x planted", lay(np.repeat(pl, n), shape), lay(np.tile(pl, n), shape))]


# ---- the case table --------------------------------------------------------------------------------------------------------

WIDE = (2, 64, 64, 16)          # 16-byte vectors in every dtype
ELEM = (2, 72, 71, 13)          # element-wise
WIDE_UP = (2, 32, 128, 16)
ELEM_UP = (2, 36, 142, 13)      # holds every 16-bit pattern as ELEM does; 72 x 71 would quadruple at stride 4 for nothing
SPP_FRAME = (19, 20, 32)        # (H + 12)(W + 12) * 64 bytes = 63488 < 64 KiB
POOL_KS = ((2, 2), (2, 1), (3, 2), (5, 1))
SPP_KS = (5, 9, 13)
UPSAMPLE_STRIDES = (1, 2, 3, 4)
MAP_KINDS = ("perm", "neighbours", "zeros", "nan")
_MAKERS = {"perm": map_perm, "neighbours": map_neighbours, "zeros": map_zeros, "nan": map_nan, "all": map_all}


def spp_frames(dtype):
    """frames the pyramid needs to hold every ordered pattern (6 for a 16-bit type), at least 2"""
    per = int(np.prod(SPP_FRAME))
    return max(2, -(-ordered(dtype).size // per))


@functools.lru_cache(None)
def input_map(kind, dtype, shape):
    if kind == "nan":
        shape = (3,) + tuple(shape[1:])
    m = _MAKERS[kind](dtype, shape)
    m.setflags(write=False)
    return m


def pool_inputs(form, dtype):
    """[(label, map)] for a pool form: "maxpool", "maxpool_dk" (single pools, wide and element-wise) or "spp", "spp_dk" """
    if form.startswith("spp"):
        shapes = [("spp", (spp_frames(dtype),) + SPP_FRAME)]
    else:
        shapes = [("wide", WIDE), ("elem", ELEM)]
    return [("%s/%s" % (sname, kind), input_map(kind, dtype, shape)) for sname, shape in shapes for kind in MAP_KINDS]


def pool_ks(form):
    return [(k, 1) for k in SPP_KS] if form.startswith("spp") else list(POOL_KS)


@functools.lru_cache(None)
def pool_expected(form, dtype, label, k, s):
    """the reference output (statement one) of one case, computed once and shared; read-only"""
    m = dict(pool_inputs(form, dtype))[label]
    out = pool_keys(m, dtype, k, s, form.endswith("_dk"))
    out.setflags(write=False)
    return out
