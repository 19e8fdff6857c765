"""Planted logits for the default (soft-max) YOLO decode and its float64 restatement.  Plain numpy, seeded, no GPU and no
package import: tests/test_yolo_decode_host.py proves on the references alone that every input is what it claims to be, and
tests/test_gpu_yolo_decode.py runs them through every compiled form of the decode.

The operation (YOLOLayer.forward plus the w, h / network-size division), for a head of ``A`` anchors on an ``h x w`` grid:

    box   = ((sxy(sigmoid(tx)) + x) / w, (sxy(sigmoid(ty)) + y) / h, exp(tw) * Aw / net_w, exp(th) * Ah / net_h)
    score = max_c softmax(class logits)_c * sigmoid(obj)          cls = the first index of that maximum
    sxy(v) = v * s - (s - 1) / 2 with the head's scale_x_y s;  row = row_offset + a * h * w + y * w + x

The four-lane forms split the class range by ``per = (classes + 3) >> 2``: lane k holds the classes ``k * per .. (k + 1) * per - 1``
that exist.  Lanes 0 / 1 and 2 / 3 are merged first (the xor1 step), then 0 / 2 and 1 / 3 (the xor2 step), so where a tie sits
relative to that split decides which comparison resolves it.

Every box is either a CLEAR MAXIMUM (the two largest float64 probabilities differ by more than ``MARGIN``, so no last bit of an
exponential decides the arg-max) or a PLANTED EXACT TIE (equal float32 logits at the maximum: equal exponentials in every form,
the lowest class must win).  ``classify`` tells which, ``tie_placements`` where a tie sits.

Not planted: NaN logits, a box whose class logits are all -inf, a class logit of +inf.  The reference's own answer there (NaN
propagation through the soft-max, torch's arg-max over NaN) is a property of torch, not of the operation.

float32 overflow is part of the operation: exp(tw) above float32's largest finite value is inf, and so is exp(tw) * Aw.  The
float64 restatement applies exactly that rule to those two intermediates (``f32_overflow``) and nothing else of float32; the
planted values stay clear of the boundary (exp(88) * 2 = 3.30e38 against 3.40e38; exp(90) = 1.2e39)."""
import numpy as np

F = np.float32
MARGIN = 1e-4                      # tests/darknet_scores_restate.py's
F32_MAX = float(np.finfo(F).max)
GRIDS = ((5, 7), (3, 9))           # 35 and 27 pixels a frame: no multiple of the decode's 32-pixel tile at batch 2 or 3

# sides of 1, 2 and 3: exp(88) * side stays finite in float32 for 1 and 2 only; every other side overflows there
ANCHOR_POOL = ((1, 2), (10, 14), (23, 27), (37, 58), (81, 82), (135, 169), (344, 319), (3, 1))

XY_EXTREMES = (20.0, -20.0, 90.0, -90.0, np.inf, -np.inf)          # tx, ty
OBJ_EXTREMES = (20.0, 90.0, np.inf, -20.0, -90.0, -np.inf)         # (the last three give a score of ~0 / exactly 0)
WH_EXTREMES = (20.0, -20.0, 88.0, 90.0, -90.0, -np.inf, np.inf)    # tw, th
WINNERS = (20.0, 90.0, 1000.0)
SHIFT = 500.0

RECIPES = ("clear", "same_lane", "boundary_0", "boundary_1", "boundary_2", "lanes_01", "lanes_02", "lanes_12", "lanes_03",
           "three_way", "three_way_123", "four_way", "all_equal", "ragged_last", "winner_20", "winner_90", "winner_1000",
           "shift_base", "shift_plus", "shift_minus", "neg_inf", "neg_inf_lane", "clear_b")
TIE_RECIPES = RECIPES[1:14]
# recipes whose SCORE is the point: their boxes get no objectness that sends the score to 0
SCORE_RECIPES = RECIPES[14:22]


# ---- the lane split -------------------------------------------------------------------------------------------------------------
def lane_per(ncls):
    return (ncls + 3) >> 2


def lane_of(c, ncls):
    return np.asarray(c) // lane_per(ncls)


def lane_range(lane, ncls):
    """classes of ``lane`` (empty for the lanes past the last class)"""
    per = lane_per(ncls)
    return range(min(lane * per, ncls), min((lane + 1) * per, ncls))


def tie_classes(recipe, ncls):
    """The classes that ``recipe`` makes equal at the maximum, ascending, or None where ``ncls`` has no such placement."""
    per = lane_per(ncls)
    lanes = [lane_range(k, ncls) for k in range(4)]

    def one_per_lane(which):
        if any(len(lanes[k]) == 0 for k in which):
            return None
        # the first class of the lowest lane, the last of the highest, the middle of those between: off the lane boundaries
        # wherever a lane holds more than one class
        out = []
        for i, k in enumerate(which):
            r = lanes[k]
            out.append(r[0] if i == 0 else (r[-1] if i == len(which) - 1 else r[len(r) // 2]))
        return tuple(out)

    if recipe == "same_lane":
        return (per, per + 1) if per >= 2 and per + 1 < ncls else None
    if recipe.startswith("boundary_"):
        b = (int(recipe[-1]) + 1) * per
        return (b - 1, b) if b < ncls else None
    if recipe.startswith("lanes_"):
        return one_per_lane((int(recipe[-2]), int(recipe[-1])))
    if recipe == "three_way":
        return one_per_lane((0, 1, 2))
    if recipe == "three_way_123":
        return one_per_lane((1, 2, 3))
    if recipe == "four_way":
        return one_per_lane((0, 1, 2, 3))
    if recipe == "all_equal":
        return tuple(range(ncls)) if ncls >= 2 else None
    if recipe == "ragged_last":
        # the last lane that holds a class holds fewer than ``per``; the earlier member sits in the lane before it
        if ncls % per == 0:
            return None
        last = (ncls - 1) // per
        return (lanes[last - 1][len(lanes[last - 1]) // 2], ncls - 1)
    raise KeyError(recipe)


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------
def f32_overflow(v):
    """a float64 intermediate as float32 holds it when it is out of range: inf.  (Nothing else of float32 is restated.)"""
    v = np.asarray(v, np.float64)
    return np.where(np.abs(v) > F32_MAX, np.copysign(np.inf, v), v)


def sigmoid64(v):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(v, np.float64)))


def softmax64(z):
    """soft-max over the last axis in float64, the maximum subtracted first.  (Needs a finite maximum: see the module docstring.)"""
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def softmax_decode64(t, anchors, grid, net, sxy=1.0):
    """t (B, h, w, A, 5 + classes); anchors: A (w, h) pixel pairs; grid (h, w); net (net_w, net_h); sxy: the head's scale_x_y, taken
    as the float32 the op stores.  -> (bbox (B, A * h * w, 4) float64, score (B, A * h * w) float64, cls (B, A * h * w) int64), rows
    in the order a * h * w + y * w + x: the head's own rows, which the decode writes from ``row_offset`` on."""
    t = np.asarray(t, np.float64)
    b, h, w, a, n = t.shape
    assert (h, w) == tuple(grid) and a == len(anchors) and n > 5
    s = float(F(sxy))
    gx = np.arange(w, dtype=np.float64).reshape(1, 1, w, 1)
    gy = np.arange(h, dtype=np.float64).reshape(1, h, 1, 1)
    aw = np.asarray([p[0] for p in anchors], np.float64).reshape(1, 1, 1, a)
    ah = np.asarray([p[1] for p in anchors], np.float64).reshape(1, 1, 1, a)
    with np.errstate(over="ignore"):
        bx = (sigmoid64(t[..., 0]) * s - (s - 1.0) / 2.0 + gx) / w
        by = (sigmoid64(t[..., 1]) * s - (s - 1.0) / 2.0 + gy) / h
        bw = f32_overflow(f32_overflow(np.exp(t[..., 2])) * aw) / float(net[0])
        bh = f32_overflow(f32_overflow(np.exp(t[..., 3])) * ah) / float(net[1])
    p = softmax64(t[..., 5:])
    cls = np.argmax(p, axis=-1)                                      # the first index of the maximum
    score = np.take_along_axis(p, cls[..., None], -1)[..., 0] * sigmoid64(t[..., 4])
    rows = lambda v: np.ascontiguousarray(np.moveaxis(v, 3, 1)).reshape((b, a * h * w) + v.shape[4:])
    return rows(np.stack([bx, by, bw, bh], -1)), rows(score), rows(cls).astype(np.int64)


# ---- what a box is --------------------------------------------------------------------------------------------------------------
def classify(t):
    """Per box of t (..., 5 + classes) float32: ``(clear, tie)``.  clear: the two largest float64 probabilities differ by more than
    MARGIN (a single class is clear).  tie: the maximum float32 logit occurs more than once."""
    z = np.asarray(t, F)[..., 5:]
    if z.shape[-1] == 1:
        return np.ones(z.shape[:-1], bool), np.zeros(z.shape[:-1], bool)
    top = np.sort(softmax64(z), axis=-1)[..., -2:]
    clear = (top[..., 1] - top[..., 0]) > MARGIN
    tie = (z == z.max(-1, keepdims=True)).sum(-1) > 1
    return clear, tie


def tie_placements(t):
    """The set of placements, relative to the lane split, that the exact ties of t (..., 5 + classes) occupy.  Computed from the
    logits alone:  "same lane": two tied classes in one lane;  "boundary k": the last class of lane k and the first of lane k + 1;
    "lanes a b": exactly two tied classes, in lanes a < b;  "three way" / "four way": that many tied classes, one per lane;
    "all equal": every class;  "ragged last": the last class is tied with an earlier one and its lane is not full."""
    z = np.asarray(t, F)[..., 5:].reshape(-1, t.shape[-1] - 5)
    ncls = z.shape[1]
    per = lane_per(ncls)
    found = set()
    for row in z[(z == z.max(-1, keepdims=True)).sum(-1) > 1]:
        tied = np.nonzero(row == row.max())[0]
        lanes = lane_of(tied, ncls)
        if len(tied) == ncls:
            found.add("all equal")
            if ncls > 2:                                             # (counted as that alone: it would be every placement at once)
                continue
        if len(set(lanes.tolist())) < len(lanes):
            found.add("same lane")
        for c0, c1 in zip(tied[:-1].tolist(), tied[1:].tolist()):
            if c1 == c0 + 1 and c1 % per == 0:
                found.add("boundary %d" % (c0 // per))
        if len(tied) == 2 and lanes[0] != lanes[1]:
            found.add("lanes %d %d" % (lanes[0], lanes[1]))
        if len(tied) in (3, 4) and len(set(lanes.tolist())) == len(tied):
            found.add("three way" if len(tied) == 3 else "four way")
        if tied[-1] == ncls - 1 and ncls % per != 0:
            found.add("ragged last")
    return found


ALL_PLACEMENTS = {"same lane", "boundary 0", "boundary 1", "boundary 2", "lanes 0 1", "lanes 2 3", "lanes 0 2", "lanes 1 2",
                  "lanes 0 3", "three way", "four way", "all equal", "ragged last"}


# ---- the generator --------------------------------------------------------------------------------------------------------------
def _clear(rng, z, lo=0.5, hi=2.0):
    """lift one class above the rest by more than 0.5 in the logit (tests/darknet_scores_restate.py's recipe)"""
    best = int(rng.integers(0, len(z)))
    rest = np.delete(z, best)
    z[best] = F((rest.max() if len(rest) else 0.0) + rng.uniform(lo, hi))
    return best


def planted_logits(seed, batch, h, w, anchors, ncls):
    """-> (t (B, h, w, A, 5 + ncls) float32, recipe (B * h * w * A,) of names, shift_triples [(base, plus, minus)] box indices).
    Box k (in the order of ``t.reshape(-1, 5 + ncls)``) takes class recipe ``RECIPES[k % 23]`` where ``ncls`` allows it (else a clear
    maximum), and extremes in tx / ty / tw / th / obj on cycles of 17 / 19 / 29 / 31 / 13 boxes, coprime to 23 and to each other (every
    case holds at least 81 boxes, so every value occurs)."""
    rng = np.random.default_rng(seed)
    n_attr = 5 + ncls
    t = np.empty((batch, h, w, anchors, n_attr), F)
    flat = t.reshape(-1, n_attr)
    n = flat.shape[0]
    flat[:, :4] = rng.uniform(-2.0, 2.0, size=(n, 4))
    flat[:, 4] = rng.uniform(-4.0, 4.0, size=n)
    flat[:, 5:] = rng.uniform(-6.0, 4.0, size=(n, ncls))
    recipe = np.empty(n, dtype=object)
    triples = []
    for k in range(n):
        name = RECIPES[k % len(RECIPES)]
        z = flat[k, 5:]
        if name in TIE_RECIPES:
            tied = tie_classes(name, ncls)
            if tied is None:
                name = "clear"
            else:
                v = F((2.5, 6.0, 30.0)[(k // len(RECIPES)) % 3])
                z[:] = np.minimum(z, v - F(1.5))
                z[list(tied)] = v
        elif name.startswith("winner_"):
            z[int(rng.integers(0, ncls))] = F(float(name[7:]))
        elif name == "shift_base" and k + 2 < n:
            # multiples of 2^-10 below 8 in size: adding +-500 is exact in float32, so the three boxes hold the same soft-max
            q = np.round(rng.uniform(-6.0, 4.0, size=ncls) * 1024.0) / 1024.0
            best = int(rng.integers(0, ncls))
            q[best] = np.delete(q, best).max(initial=0.0) + np.round(rng.uniform(0.5, 2.0) * 1024.0) / 1024.0
            z[:] = q
            flat[k + 1, 5:] = (q + SHIFT).astype(F)
            flat[k + 2, 5:] = (q - SHIFT).astype(F)
            assert np.array_equal(flat[k + 1, 5:].astype(np.float64) - SHIFT, q)
            assert np.array_equal(flat[k + 2, 5:].astype(np.float64) + SHIFT, q)
            triples.append((k, k + 1, k + 2))
        elif name in ("shift_plus", "shift_minus") and triples and triples[-1][-1] >= k:
            pass                                                     # written with its base
        elif name == "neg_inf" and ncls >= 2:
            best = _clear(rng, z)
            others = np.delete(np.arange(ncls), best)
            gone = others[rng.uniform(size=len(others)) < 0.5]
            z[gone if len(gone) else others[:1]] = -np.inf
        elif name == "neg_inf_lane" and ncls >= 2:
            # a whole lane at -inf: lane 0 with the winner in the last lane that holds a class, or the other way round
            last = (ncls - 1) // lane_per(ncls)
            dead, alive = (0, last) if (k // len(RECIPES)) % 2 == 0 else (last, 0)
            z[list(lane_range(dead, ncls))] = -np.inf
            win = lane_range(alive, ncls)
            win = win[int(rng.integers(0, len(win)))]
            finite = np.isfinite(z)
            finite[win] = False
            z[win] = F((z[finite].max() if finite.any() else 0.0) + rng.uniform(0.5, 2.0))
        else:
            name = "clear" if name not in ("clear", "clear_b") else name
        if name in ("clear", "clear_b"):
            _clear(rng, z)
        recipe[k] = name
    # extremes, whatever the class recipe; a box whose score is the point keeps an objectness that leaves the score alone
    for k in range(n):
        if k % 17 < len(XY_EXTREMES):
            flat[k, 0] = XY_EXTREMES[k % 17]
        if k % 19 < len(XY_EXTREMES):
            flat[k, 1] = XY_EXTREMES[k % 19]
        if k % 29 < len(WH_EXTREMES):
            flat[k, 2] = WH_EXTREMES[k % 29]
        if k % 31 < len(WH_EXTREMES):
            flat[k, 3] = WH_EXTREMES[k % 31]
        if k % 13 < (3 if recipe[k] in SCORE_RECIPES else len(OBJ_EXTREMES)):
            flat[k, 4] = OBJ_EXTREMES[k % 13]
    for base, plus, minus in triples:
        flat[plus, 4] = flat[minus, 4] = flat[base, 4]
    return t, recipe, triples


# name: (grid, batch, anchors, classes, scale_x_y, row_offset, rows after the head)
CASE_TABLE = {
    "c1_a3": ((5, 7), 2, 3, 1, 1.0, 0, 0),
    "c2_a1": ((3, 9), 3, 1, 2, 1.0, 0, 0),
    "c3_a2": ((5, 7), 2, 2, 3, 1.0, 0, 0),
    "c4_a3_s12": ((3, 9), 3, 3, 4, 1.2, 0, 0),
    "c5_a8": ((5, 7), 2, 8, 5, 1.0, 0, 0),
    "c7_a2_mid": ((3, 9), 3, 2, 7, 1.0, 50, 33),
    "c80_a3_mid": ((5, 7), 3, 3, 80, 1.0, 317, 41),
    "c80_a1_s20": ((3, 9), 3, 1, 80, 2.0, 0, 0),
    "c81_a2": ((5, 7), 2, 2, 81, 1.0, 0, 0),
    "c122_a3": ((3, 9), 3, 3, 122, 1.0, 0, 0),
    "c27_a8": ((3, 9), 2, 8, 27, 1.0, 0, 0),
}
CASE_NAMES = tuple(CASE_TABLE)
_CASES = {}


def case(name):
    """dict(t, anchors, grid, net, sxy, row_offset, rows_total, recipe, shift_triples); made once, to be left unchanged"""
    if name not in _CASES:
        grid, batch, na, ncls, sxy, row_offset, after = CASE_TABLE[name]
        seed = 7000 + 97 * CASE_NAMES.index(name)
        t, recipe, triples = planted_logits(seed, batch, grid[0], grid[1], na, ncls)
        t.setflags(write=False)
        _CASES[name] = dict(name=name, t=t, anchors=tuple((float(a), float(b)) for a, b in ANCHOR_POOL[:na]), grid=grid,
                            net=(32.0 * grid[1], 32.0 * grid[0]), sxy=sxy, row_offset=row_offset,
                            rows_total=row_offset + na * grid[0] * grid[1] + after, recipe=recipe, shift_triples=triples)
    return _CASES[name]


def want(c):
    """softmax_decode64 of a case"""
    return softmax_decode64(c["t"], c["anchors"], c["grid"], c["net"], c["sxy"])


# ---- planted detection heads: one box per anchor, drawn from a case -------------------------------------------------------------
def head_boxes(name, n_sets):
    """``n_sets`` tuples of A box indices of case ``name``, walking its recipes in order (every recipe first, then again with the
    next box that carries it, whose extremes differ): set j holds recipes j * A .. j * A + A - 1 (mod 23)."""
    c = case(name)
    na = len(c["anchors"])
    n = len(c["recipe"])
    picks = []
    for i in range(n_sets * na):
        r, lap = i % len(RECIPES), i // len(RECIPES)
        k = r + len(RECIPES) * lap
        if RECIPES[r] in ("shift_plus", "shift_minus") and not any(k in tr for tr in c["shift_triples"]):
            k = r                                                   # (a triple cut off by the end of the case)
        assert k < n
        picks.append(k)
    return [tuple(picks[j * na:(j + 1) * na]) for j in range(n_sets)]


def head_bias(name, boxes):
    """the bias of a head conv whose anchor a carries box ``boxes[a]`` of case ``name``: (A * (5 + classes),) float32"""
    flat = case(name)["t"].reshape(-1, case(name)["t"].shape[-1])
    return np.concatenate([flat[k] for k in boxes]).astype(F)
