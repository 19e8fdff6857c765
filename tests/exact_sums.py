"""Planted operands on which a conv's float32 sum is ONE number whatever the order, and that number (numpy only: no torch, no GPU).

Every conv kernel accumulates in float32.  If activations, weights, bias and shortcut are integers and, for every output,

    (a)  sum_k |w_k * x_k| + |bias / scale| < 2^24                                                    (EXACT_F32)

then every partial sum of every K order, K-tiling, MFMA grouping and fma contraction is an integer below 2^24 and therefore a
float32: nothing is ever rounded, and the accumulator is the integer an int64 convolution gives.  2^24 is where float32 stops
holding every integer (24 significand bits).  The scales are +-1 and +-0.5, so t = acc * scale + bias is exact as well (a
multiple of 0.5 below 2^24), fused into one fma or not.  The output is the epilogue of t as tests/epilogue_cases.py states it
(tests/test_gpu_epilogue.py pins that rule on the GPU): leaky or linear, one float32 rounding of a fused shortcut sum, the
storage rounding.  So the expected output is known to the bit in all three storage types, without knowing the sum order.

Three plants per case and storage type (``plant``):

  unit    activations from {-1, 0, +1}, weights from {-1, +1}, small integer bias and shortcut: |t| stays inside the storage
          type's exact-integer range -- (b) below -- where a sum that is off by one unit (a tap read twice, or from the
          neighbouring pixel) is always a different bit pattern;
  wide_x  activations are odd integers that need the storage type's whole significand (up to 255 in bf16: 8 bits, 2047 in fp16:
          11 bits, 4095 in float32 or what (a) leaves: 12 bits, which no 16-bit type and no 10-bit input format holds), weights
          from {-1, 0, +1}: an operand that loses low bits on its way to the multiplier shows;
  wide_w  the mirror image: wide weights, unit activations.

Byte inputs (the stems, the conv_direct uint8 rows) hold only the bytes 0 and 255, which the kernels' IEEE division by 255 turns
into 0.0 and 1.0 exactly; they have no wide_x plant.

  (b)  on the unit plant at most 1 % (OUTSIDE_CAP) of a case's outputs may have |t| outside the exact-integer range of the
       OUTPUT type: 256 in bf16 (8 significand bits: every integer up to 2^8), 2048 in fp16 (11 bits: 2^11), 2^24 in float32;
       halved for the +-0.5 scales, whose t are multiples of 0.5.  The deepest row of the table has K = 4608
       (dw48_k3_c512_res): a sum of 4608 products of {-1, 0, 1} x {-1, +1} has sigma = sqrt(4608 * 2 / 3) = 55 (a trial of
       20000 such sums: sigma 56, max |sum| 221, none beyond 256), of +-1 x +-1 sigma = 68: 256 is 3.8 sigma, 0.02 %.
       (Below zero the leaky slope compresses t by ten, so there two neighbouring sums CAN round to one storage value; half
       the outputs are positive.)
  (c)  every (tap, input channel) has a non-zero weight in at least one output channel, and every input position is non-zero in
       at least one frame: no K index and no pixel is invisible.  One exception, stated in ``input_nonzero_required``: a byte
       input of ONE frame keeps its zeros, because the only all-non-zero byte plant is all 255, on which every misplaced tap
       reads the value it should have read.

Two-conv groups (stem_pair, resblock, block) store their intermediate after leaky.  The first conv gets sparse weights and a
positive bias so that every one of its pre-activations is a positive integer inside the storage type's exact range: leaky and the
store leave it as it is (``reference`` asserts it), and (a)-(c) apply to the second conv on that intermediate.  The fused block's
first conv reads ONE input channel per output channel (its 1152-deep second conv leaves (b) no room for more); the three plants
start at different channels, so together they read them all.

The sum itself: the products are summed by a float64 matrix product, exact in any order because (a) keeps every partial sum
below 2^24, far below 2^53, and the result is converted to int64 after a check that it holds integers only
(tests/test_exact_sums_host.py holds it to a literal int64 accumulation and to the oracle's float64 conv_block)."""
import zlib

import numpy as np

import epilogue_cases as EC

EXACT_F32 = 1 << 24                                       # (a): float32 holds every integer below 2^24
EXACT_INT = {"bf16": 1 << 8, "fp16": 1 << 11, "float32": 1 << 24}     # (b): |integer| <= this is exact in the storage type
OUTSIDE_CAP = 0.01                                        # (b): share of a unit case's outputs allowed outside that range
WIDE = {"bf16": 255, "fp16": 2047, "float32": 4095}       # largest odd integer of the wide plants: 8, 11 and 12 bits
SCALES = (1.0, -1.0, 0.5, -0.5)
BIAS_MAX = 4                                              # |bias| and |shortcut| of a single conv
PLANTS = ("unit", "wide_x", "wide_w")
GROUPS = ("conv", "stem_pair", "resblock", "block")
HEAD_TAPS = 8                                             # non-zero weights per head channel: |logit| <= 8 + 4 <= HEAD_LOGIT_MAX
HEAD_LOGIT_MAX = 16
FAULTS = ("tap_shift", "drop_k", "bf16_per_64", "x_bf16")


# ------------------------------------------------------------------------------------------------ the cases' convs

def conv_specs(case):
    """[dict(cin, cout, k, s, pad, leaky)] of the case's convs (tests/test_gpu_footprint.py _conv_specs, with the padding)"""
    g = case["group"]
    mk = lambda cin, cout, k, s, pad, leaky=True: dict(cin=cin, cout=cout, k=k, s=s, pad=pad, leaky=leaky)
    if g == "conv":
        return [mk(case["cin"], case["cout"], case["k"], case["s"], case["pad"], case.get("leaky", True))]
    if g == "stem_pair":
        return [mk(3, 32, 3, 1, 1), mk(32, 64, 3, 2, 1)]
    if g == "resblock":
        return [mk(64, 32, 1, 1, 0), mk(32, 64, 3, 1, 1)]
    if g == "block":
        return [mk(case["cin"], 128, 1, 1, 0), mk(128, case["cout"], 3, 1, 1)]
    if g == "head":
        return [mk(case["cin"], 255, 1, 1, 0, False)]
    raise AssertionError(g)


def input_kind(case):
    """"act" (activations of the storage type), "nchw" (float32 network input) or "u8" (byte frames, BGR)"""
    if case["group"] == "stem_pair":
        return "u8"
    return case["inp"] if case["group"] == "conv" else "act"


def shortcut_kind(case):
    """None, "own" (an operand of its own, the output's shape) or "input" (the fused groups: the group's input)"""
    g = case["group"]
    if g == "conv":
        return "own" if case["res"] else None
    if g == "resblock" or (g == "block" and case["res"]):
        return "input"
    return None


def out_dtype(case, dtype):
    return "float32" if case["group"] == "head" or case.get("out_f32") else dtype


def plants_of(case):
    """the plants a case gets: byte inputs have no wide activations; the heads run the unit plant (finite decode)"""
    if case["group"] == "head":
        return ("unit",)
    if case["group"] == "conv" and input_kind(case) == "u8":
        return ("unit", "wide_w")
    return PLANTS


def input_nonzero_required(case):
    """(c) for the input: every position non-zero in some frame -- but for one frame of bytes (see the module text)"""
    return not (input_kind(case) == "u8" and case["B"] == 1)


def out_hw(h, w, sp):
    return (h + 2 * sp["pad"] - sp["k"]) // sp["s"] + 1, (w + 2 * sp["pad"] - sp["k"]) // sp["s"] + 1


# ------------------------------------------------------------------------------------------------ generators

def _rng(case, dtype, kind):
    return np.random.RandomState(zlib.crc32(("%s/%s/%s" % (case["id"], dtype, kind)).encode()) & 0x7fffffff)


def _signs(rng, shape):
    return rng.randint(0, 2, shape) * 2 - 1


def _odd(rng, shape, amp):
    """odd integers of either sign up to ``amp`` (odd): every one needs its lowest bit, half of them the highest too"""
    return (2 * rng.randint(0, (amp + 1) // 2, shape) + 1) * _signs(rng, shape)


def _wide_amp(dtype, k_total, x_max=1):
    """the largest odd amplitude (a) leaves a K of ``k_total`` whose other operand reaches ``x_max``"""
    a = min(WIDE[dtype], (EXACT_F32 - 1 - 2 * BIAS_MAX - 1) // (k_total * x_max))
    a -= 1 - a % 2
    assert a >= 3, (dtype, k_total, x_max)
    return a


def _no_dead_frames(x, fill):
    """x (B, ...): positions that are zero in every frame get ``fill`` (an array of x's per-frame shape) in one frame"""
    dead = np.nonzero((x == 0).all(axis=0).ravel())[0]
    flat = x.reshape(x.shape[0], -1)
    flat[dead % x.shape[0], dead] = fill.ravel()[dead]
    return x


def _no_dead_taps(w, rng):
    """w (cout, cin, k, k): (tap, channel) positions that are zero in every output channel get +-1 in one"""
    dead = np.nonzero((w == 0).all(axis=0).ravel())[0]
    flat = w.reshape(w.shape[0], -1)
    flat[dead % w.shape[0], dead] = _signs(rng, dead.size)
    return w


def _sparse_weights(rng, sp, taps, start, values=(-1, 1)):
    """``taps`` non-zero weights per output channel, laid so that consecutive channels read consecutive K positions from
    ``start`` on: taps * cout >= K covers every position"""
    cout, kk = sp["cout"], sp["k"] * sp["k"] * sp["cin"]
    w = np.zeros((cout, kk), dtype=np.int64)
    pos = (start + np.arange(cout * taps)) % kk
    w[np.repeat(np.arange(cout), taps), pos] = rng.choice(values, cout * taps)
    # K order here is (ky, kx, ci); any order would do: the layout only has to cover
    return np.ascontiguousarray(w.reshape(cout, sp["k"], sp["k"], sp["cin"]).transpose(0, 3, 1, 2))


def _scales(rng, cout):
    s = np.asarray(SCALES)[np.arange(cout) % 4]           # every scale value in every group of four channels ...
    return s[rng.permutation(cout)] if cout >= 8 else s    # ... in an order that is no period of the tile


def _input(rng, case, kind, dtype, cin, amp=None):
    B, h, w = case["B"], case["h"], case["w"]
    shape = (B, h, w, cin)
    if input_kind(case) == "u8":
        x = rng.randint(0, 2, shape)
        return _no_dead_frames(x, np.ones(shape[1:], dtype=np.int64)) if input_nonzero_required(case) else x
    if kind == "wide_x":
        return _odd(rng, shape, amp)
    x = rng.randint(-1, 2, shape)
    return _no_dead_frames(x, _signs(rng, shape[1:]))


def plant(case, dtype, kind):
    """The planted operands of ``case`` in storage type ``dtype``: dict of
    x       (B, h, w, cin) int64, the input's values (bytes: 0 / 1 for the bytes 0 / 255, channels in the conv's RGB order)
    res     (B, ho, wo, cout) int64 or None: the shortcut operand where it is an operand of its own
    convs   [dict(w=(cout, cin, k, k) int64, scale=(cout,) float32, bias=(cout,) float32)]"""
    assert kind in plants_of(case), (case["id"], kind)
    rng = _rng(case, dtype, kind)
    specs = conv_specs(case)
    if len(specs) == 1:
        sp = specs[0]
        kk = sp["k"] * sp["k"] * sp["cin"]
        amp = _wide_amp(dtype, kk) if kind != "unit" else None
        x = _input(rng, case, kind, dtype, sp["cin"], amp)
        shape = (sp["cout"], sp["cin"], sp["k"], sp["k"])
        if case["group"] == "head":
            assert HEAD_TAPS * sp["cout"] >= kk and HEAD_TAPS + BIAS_MAX <= HEAD_LOGIT_MAX
            w = _sparse_weights(rng, sp, HEAD_TAPS, 0)
        elif kind == "unit":
            w = _signs(rng, shape)
        elif kind == "wide_x":
            w = _no_dead_taps(rng.randint(-1, 2, shape), rng)
        else:
            w = _odd(rng, shape, amp)
        ho, wo = out_hw(case["h"], case["w"], sp)
        res = rng.randint(-BIAS_MAX, BIAS_MAX + 1, (case["B"], ho, wo, sp["cout"])) if shortcut_kind(case) == "own" else None
        conv = dict(w=w, scale=_scales(rng, sp["cout"]).astype(np.float32),
                    bias=rng.randint(-BIAS_MAX, BIAS_MAX + 1, sp["cout"]).astype(np.float32))
        return dict(x=x, res=res, convs=[conv])
    return _plant_pair(rng, case, dtype, kind, specs)


def _plant_pair(rng, case, dtype, kind, specs):
    """first conv: ``taps`` weights of +-1 / |scale| per channel and a bias that keeps t1 = acc * scale + bias a positive integer,
    1 .. 2 * taps + 1 (unit, wide_w) or an ODD integer up to the storage type's widest (wide_x: even sums, odd bias)"""
    s1, s2 = specs
    k1, k2 = s1["k"] ** 2 * s1["cin"], s2["k"] ** 2 * s2["cin"]
    x = _input(rng, case, "unit", dtype, s1["cin"])
    x_abs = 1
    # (b) on the 1152-deep second conv of the fused block: t1 in 1 .. 3 gives sigma = sqrt(1152 * 4.7) = 73, 256 is 3.5 sigma;
    # two taps (t1 in 1 .. 5, sigma 109) would put 1.9 % of the outputs outside
    taps = 1 if case["group"] == "block" else max(1, -(-k1 // s1["cout"]))
    start = PLANTS.index(kind) * s1["cout"] * taps
    scale1 = _scales(rng, s1["cout"])
    unit_w = _sparse_weights(rng, s1, taps, start)
    step = 2 if kind == "wide_x" else 1                   # wide_x: every product even
    w1 = unit_w * (step / np.abs(scale1)).astype(np.int64)[:, None, None, None]
    reach = taps * x_abs * step                            # |acc * scale| <= reach
    if kind == "wide_x":
        amp = _wide_amp(dtype, k2)
        assert amp > 2 * reach + 2
        bias1 = 2 * rng.randint(0, (amp - 2 * reach + 1) // 2, s1["cout"]) + 1 + reach       # odd, reach + 1 .. amp - reach
        t1_max = amp
    else:
        bias1 = np.full(s1["cout"], reach + 1)
        t1_max = 2 * reach + 1
    shape2 = (s2["cout"], s2["cin"], s2["k"], s2["k"])
    if kind == "unit":
        w2 = _signs(rng, shape2)
    elif kind == "wide_x":
        w2 = _no_dead_taps(rng.randint(-1, 2, shape2), rng)
    else:
        w2 = _odd(rng, shape2, _wide_amp(dtype, k2, t1_max))
    convs = [dict(w=w1, scale=scale1.astype(np.float32), bias=bias1.astype(np.float32)),
             dict(w=w2, scale=_scales(rng, s2["cout"]).astype(np.float32),
                  bias=rng.randint(-BIAS_MAX, BIAS_MAX + 1, s2["cout"]).astype(np.float32))]
    return dict(x=x, res=None, convs=convs)


def frames_of(p):
    """the byte frames of a byte-input plant: 0 / 255, BGR in memory (the kernels flip to the conv's RGB)"""
    return np.ascontiguousarray((p["x"][..., ::-1] * 255).astype(np.uint8))


# ------------------------------------------------------------------------------------------------ the reference

def im2col(x, sp):
    """x (B, h, w, c) -> (B * ho * wo, k * k * c) float64, zero padding, K order (ky, kx, ci)"""
    k, s, pad = sp["k"], sp["s"], sp["pad"]
    B, h, w, c = x.shape
    ho, wo = out_hw(h, w, sp)
    xp = np.zeros((B, h + 2 * pad + k, w + 2 * pad + k, c), dtype=np.float64)       # (room for an even kernel's last tap)
    xp[:, pad:pad + h, pad:pad + w] = x
    cols = [xp[:, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s] for ky in range(k) for kx in range(k)]
    return np.concatenate(cols, axis=-1).reshape(B * ho * wo, k * k * c)


def weight_matrix(w):
    """(cout, cin, k, k) -> (k * k * cin, cout) float64 in im2col's K order"""
    return np.ascontiguousarray(w.transpose(2, 3, 1, 0).reshape(-1, w.shape[0])).astype(np.float64)


def to_int64(acc):
    r = np.rint(acc)
    assert np.array_equal(r, acc) and np.abs(acc).max(initial=0) < 2.0 ** 53
    return r.astype(np.int64)


def epilogue(acc, conv, leaky, r, odt):
    """the stored float32 values of integer sums ``acc`` (n, cout): tests/epilogue_cases.py ``expect``, which must be exact"""
    t = acc.astype(np.float64) * conv["scale"].astype(np.float64) + conv["bias"].astype(np.float64)
    t32 = t.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), t), "acc * scale + bias is no float32: condition (a) is broken"
    lo, hi, nan = EC.expect("leaky" if leaky else "linear", odt, t32, None if r is None else r.astype(np.float32), fused=True)
    assert not nan.any() and np.array_equal(EC.bits(lo), EC.bits(hi))
    return t, lo


class Last:
    """the last conv of a case on its planted input: what the reference, the conditions and the faults all start from"""

    def __init__(self, case, dtype, p):
        specs = conv_specs(case)
        x = p["x"].astype(np.float64)
        self.mid_t = None
        if len(specs) == 2:
            acc1 = to_int64(im2col(x, specs[0]) @ weight_matrix(p["convs"][0]["w"]))
            t1, mid = epilogue(acc1, p["convs"][0], True, None, dtype)
            # the intermediate as stored IS the positive integer t1: leaky and the storage rounding changed nothing
            assert (t1 >= 1).all() and np.array_equal(t1, np.rint(t1)) and np.array_equal(mid.astype(np.float64), t1), case["id"]
            ho, wo = out_hw(case["h"], case["w"], specs[0])
            self.mid_t = t1
            self.x = t1.reshape(case["B"], ho, wo, specs[0]["cout"])
        else:
            self.x = x
        self.sp, self.conv = specs[-1], p["convs"][-1]
        self.B = case["B"]
        self.ho, self.wo = out_hw(self.x.shape[1], self.x.shape[2], self.sp)
        kind = shortcut_kind(case)
        self.r = None if kind is None else (p["res"] if kind == "own" else p["x"]).reshape(-1, self.sp["cout"])
        self.odt = out_dtype(case, dtype)
        self.wm = weight_matrix(self.conv["w"])
        self.cols = im2col(self.x, self.sp)

    def stored(self, acc, rows=None):
        r = self.r if self.r is None or rows is None else self.r[rows]
        return epilogue(acc, self.conv, self.sp["leaky"], r, self.odt)


def reference(case, dtype, p):
    """(pre-activations t float64, expected stored output float32 bits as float32), both (B * ho * wo, cout)"""
    last = Last(case, dtype, p)
    return last.stored(to_int64(last.cols @ last.wm))


def first_difference(got, want, case, dtype, p):
    """None, or "N of M values differ, first at (frame, y, x, channel): got, want" for two (pixels, cout) float32 arrays
    compared as bit patterns"""
    differ = EC.bits(got) != EC.bits(want)
    if not differ.any():
        return None
    sp = conv_specs(case)[-1]
    h, w = (case["h"], case["w"]) if len(conv_specs(case)) == 1 else out_hw(case["h"], case["w"], conv_specs(case)[0])
    ho, wo = out_hw(h, w, sp)
    pix, ch = np.argwhere(differ)[0]
    b, rem = divmod(int(pix), ho * wo)
    return "%d of %d values differ, first at (frame %d, y %d, x %d, channel %d): got %r (0x%08x), want %r (0x%08x)" % (
        int(differ.sum()), differ.size, b, rem // wo, rem % wo, int(ch), float(got[pix, ch]), int(EC.bits(got)[pix, ch]),
        float(want[pix, ch]), int(EC.bits(want)[pix, ch]))


# ------------------------------------------------------------------------------------------------ the conditions

def conditions(case, dtype, kind, p, last=None):
    """Asserts (a), (b) and (c) for one planted case; returns the measured figures"""
    last = last or Last(case, dtype, p)
    conv, wm = last.conv, last.wm
    what = "%s %s %s" % (case["id"], dtype, kind)
    # (a) every order of the float32 sum is exact: sum |w x| + |bias / scale| < 2^24, and so is the scaled t
    absum = (np.abs(last.cols) @ np.abs(wm)).max(axis=0) + np.abs(conv["bias"].astype(np.float64) / conv["scale"])
    assert absum.max() < EXACT_F32, "(a) %s: sum |w x| + |bias / scale| reaches %d" % (what, absum.max())
    acc = to_int64(last.cols @ wm)
    t, _ = last.stored(acc)
    assert np.abs(t).max() < EXACT_F32, "(a) %s: |t| reaches %g" % (what, np.abs(t).max())
    assert set(np.abs(conv["scale"]).tolist()) <= {1.0, 0.5}
    # (b) the unit plant stays in the output type's exact-integer range, halved for the +-0.5 scales
    limit = EXACT_INT[last.odt] * np.abs(conv["scale"].astype(np.float64))
    outside = float((np.abs(t) > limit).mean()) if last.odt != "float32" else float((np.abs(t) >= limit).mean())
    if kind == "unit":
        assert outside <= OUTSIDE_CAP, "(b) %s: %.2f %% of the pre-activations lie outside the exact range" % (what, 100 * outside)
    if case["group"] == "head":
        assert np.abs(t).max() <= HEAD_LOGIT_MAX, "%s: |logit| reaches %g" % (what, np.abs(t).max())
    # (c) no K index and no input position is invisible
    assert (wm != 0).any(axis=1).all(), "(c) %s: a (tap, channel) has no non-zero weight" % what
    if input_nonzero_required(case) or last.mid_t is not None:
        assert (last.x != 0).any(axis=0).all(), "(c) %s: an input position is zero in every frame" % what
    else:
        assert (last.x != 0).mean() > 0.4                # one frame of bytes: zeros stay (module text)
    return dict(absum=float(absum.max()), t_max=float(np.abs(t).max()), outside=outside)


# ------------------------------------------------------------------------------------------------ faults, for the host test
# What the comparison is FOR, recomputed without a GPU: each fault below is applied to the last conv's sum on a sample of the
# output pixels, and must change at least one expected bit pattern.

def sample_rows(last, most=1024):
    """output pixels the faults are tried on: the whole last column and an even sample of the rest"""
    n = last.cols.shape[0]
    col = np.arange(n)[np.arange(n) % last.wo == last.wo - 1]
    rest = np.arange(0, n, max(1, n // most))
    return np.unique(np.concatenate([col[:: max(1, col.size // most)], rest]))


def fault_applies(fault, case, dtype):
    sp = conv_specs(case)[-1]
    if fault == "bf16_per_64":
        # there must be a K-tile boundary to narrow at, and a wide plant: the unit plant's sums are bf16 values by design, (b).
        # (The heads run the unit plant only: a fused head that narrowed its accumulator would differ from conv + decode on the
        # footprint suite's random data, and the unfused conv is an implicit-GEMM row with all three plants.)
        return sp["k"] ** 2 * sp["cin"] > 64 and len(plants_of(case)) > 1
    if fault == "x_bf16":                                 # float32 operands that hold more than bf16's 8 bits
        return dtype == "float32" and input_kind(case) != "u8"
    return True


def faulty_sum(last, fault, rows):
    """the sums (len(rows), cout) float64 a kernel with ``fault`` would hand its epilogue"""
    cols, wm, sp = last.cols[rows], last.wm, last.sp
    c = sp["cin"]
    if fault == "drop_k":                                 # one K index is never multiplied
        cols = cols.copy()
        cols[:, cols.shape[1] // 2] = 0
        return cols @ wm
    if fault == "tap_shift":                              # the centre tap of the LAST output column reads the pixel to its left
        shifted = np.zeros_like(last.x)
        shifted[:, :, 1:] = last.x[:, :, :-1]
        other = im2col(shifted, sp)[rows]
        tap = (sp["k"] // 2) * sp["k"] + sp["k"] // 2
        edge = rows % last.wo == last.wo - 1
        cols = cols.copy()
        cols[np.ix_(edge, np.arange(tap * c, (tap + 1) * c))] = other[np.ix_(edge, np.arange(tap * c, (tap + 1) * c))]
        return cols @ wm
    if fault == "bf16_per_64":                            # the running sum narrowed to bf16 between K-tiles of 64
        acc = np.zeros((cols.shape[0], wm.shape[1]))
        for k0 in range(0, cols.shape[1], 64):
            if k0:
                acc = EC.rne_bf16(acc.astype(np.float32)).astype(np.float64)
            acc = acc + cols[:, k0:k0 + 64] @ wm[k0:k0 + 64]
        return acc
    if fault == "x_bf16":                                 # float32 activations that reach the multiplier as bf16
        return EC.rne_bf16(cols.astype(np.float32)).astype(np.float64) @ wm
    raise AssertionError(fault)


def fault_changes(last, fault, rows):
    """how many expected bit patterns of the sampled rows the fault changes"""
    _, good = last.stored(to_int64(last.cols[rows] @ last.wm), rows)
    # (a faulty sum is still an integer: every fault drops, moves or rounds integers)
    _, bad = last.stored(to_int64(faulty_sum(last, fault, rows)), rows)
    return int((EC.bits(good) != EC.bits(bad)).sum())
