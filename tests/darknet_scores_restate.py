"""Darknet's class scores and multi-label candidates restated in numpy float32, independent of the package.

The rule (Darknet src/yolo_layer.c: forward_yolo_layer's logistic activations, get_yolo_detections), every operation rounded
to float32 on its own:

    obj = 1 / (1 + exp(-t4))        p_c = 1 / (1 + exp(-t_c))                        (logistic_activate)
    single label:  prob = p_best * obj,  cls = the first c with p_c == max p_c        (Y3_F_SCORES_DARKNET)
    multi label:   if obj > thresh:  for every c:  s_c = obj * p_c;  if s_c > thresh: label (row, c, s_c)

A ``new_coords`` head stores probabilities already: obj = t4, p_c = t_c.  Rows are numbered as the decode numbers them,
row_offset + anchor * h * w + y * w + x; labels come in ascending (row, c) order.

numpy's float32 exp and the device's expf may differ in the last bit, so the inputs are PLANTED: evaluated in float64, no obj
and no s_c of a row whose objectness passes (the only rows whose s_c is ever looked at) lies within MARGIN of a threshold in
use, and where an arg-max is compared the two largest p_c differ by more than MARGIN or are exact float32 ties planted on
purpose (two equal logits; a pair of logits above 20, which both give 1.0f).  ``check_margins`` / ``check_argmax`` assert this;
tests/test_darknet_scores_host.py runs them on every input the GPU tests use.  The inputs are made by the seeded generators
below, so the committed seeds and shapes ARE the committed inputs.
"""
import numpy as np

F = np.float32
MARGIN = 1e-4
THRESHOLDS = (0.25, 0.001, 0.0)


def logistic(x):
    """1 / (1 + expf(-x)) with float32 roundings.  expf itself is float64's exp rounded to float32: a function of the VALUE alone
    (numpy's vectorised float32 exp may round the same value differently at different positions of an array, which would break
    the exact ties between equal logits that the suppression order depends on)."""
    x = np.asarray(x, F)
    with np.errstate(over="ignore"):
        e = np.exp(-x.astype(np.float64)).astype(F)
        return (F(1) / (F(1) + e)).astype(F)


def probabilities(t, new_coords=False):
    """t (..., n_attr) float32 -> (obj (...), p (..., classes)) float32"""
    t = np.asarray(t, F)
    if new_coords:
        return t[..., 4].copy(), t[..., 5:].copy()
    return logistic(t[..., 4]), logistic(t[..., 5:])


def decode_scores(t, new_coords=False):
    """single label: (prob float32, cls int64) of every box of t (..., n_attr)"""
    obj, p = probabilities(t, new_coords)
    cls = np.argmax(p, axis=-1)                                  # the first index of the maximum
    best = np.take_along_axis(p, cls[..., None], -1)[..., 0]
    return (best * obj).astype(F), cls.astype(np.int64)


def head_rows(t, row_offset):
    """t (B, h, w, A, n_attr) -> (t as (B, A * h * w, n_attr) in row order, rows)"""
    b, h, w, a, n = t.shape
    flat = np.ascontiguousarray(np.transpose(t, (0, 3, 1, 2, 4))).reshape(b, a * h * w, n)
    return flat, row_offset + np.arange(a * h * w)


def labels(heads, thresh):
    """heads: [dict(t=(B, h, w, A, n_attr) float32, row_offset=int, new_coords=bool)].  Per frame: (rows int64, cls int64,
    score float32) of every label, in ascending (row, c) order.  NaN compares false."""
    thresh = F(thresh)
    batch = heads[0]["t"].shape[0]
    out = []
    for f in range(batch):
        rows, cls, score = [], [], []
        for hd in sorted(heads, key=lambda d: d["row_offset"]):
            flat, rr = head_rows(hd["t"], hd["row_offset"])
            obj, p = probabilities(flat[f], hd.get("new_coords", False))
            with np.errstate(invalid="ignore"):
                s = (obj[:, None] * p).astype(F)
                hit = (obj > thresh)[:, None] & (s > thresh)
            r, c = np.nonzero(hit)                               # row-major: (row, c) ascending
            rows.append(rr[r])
            cls.append(c)
            score.append(s[r, c])
        out.append((np.concatenate(rows).astype(np.int64), np.concatenate(cls).astype(np.int64),
                    np.concatenate(score).astype(F)))
    return out


# ---- float64 evaluation and the margins -----------------------------------------------------------------------------------------

def probabilities64(t, new_coords=False):
    t = np.asarray(t, np.float64)
    if new_coords:
        return t[..., 4], t[..., 5:]
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-t[..., 4])), 1.0 / (1.0 + np.exp(-t[..., 5:]))


def check_margins(t, thresholds, new_coords=False, margin=MARGIN):
    """AssertionError unless, in float64, every finite obj of ``t`` and every s_c of a row with obj > threshold stays more
    than ``margin`` away from each threshold.  (NaN rows decide by the comparison's NaN rule, not by arithmetic.)"""
    obj, p = probabilities64(t, new_coords)
    s = obj[..., None] * p
    for th in thresholds:
        with np.errstate(invalid="ignore"):
            d_obj = np.abs(obj - th)
            assert not bool((d_obj <= margin).any()), "an objectness within %g of the threshold %g" % (margin, th)
            live = np.broadcast_to((obj > th)[..., None], s.shape)
            assert not bool((live & (np.abs(s - th) <= margin)).any()), "a score within %g of the threshold %g" % (margin, th)


def check_argmax(t, new_coords=False, margin=MARGIN):
    """AssertionError unless the two largest p_c of every box differ by more than ``margin`` in float64 or are an exact tie in
    float32 (planted).  Returns the number of boxes whose maximum is such a tie."""
    _, p64 = probabilities64(t, new_coords)
    if p64.shape[-1] < 2:
        return 0
    _, p32 = probabilities(t, new_coords)
    top = np.sort(p64, axis=-1)[..., -2:]
    close = (top[..., 1] - top[..., 0]) <= margin
    top32 = np.sort(p32, axis=-1)[..., -2:]
    tie = top32[..., 1] == top32[..., 0]
    assert not bool((close & ~tie).any()), "two largest class probabilities within %g and not an exact tie" % margin
    return int(tie.sum())


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def decode_logits(seed, batch, h, w, anchors, classes):
    """(B, h, w, A, 5 + classes) float32 for the decode tests: ordinary logits; +-20 and +-90 in the objectness of some boxes, -20
    and -90 in the two last class logits of others (tx, ty, tw, th stay within +-2: tests/yolo_decode_cases.py saturates those);
    planted ties (two equal maximal logits; a pair above 20), and an arg-max that no last bit decides (check_argmax)."""
    rng = np.random.default_rng(seed)
    t = rng.uniform(-6.0, 4.0, size=(batch, h, w, anchors, 5 + classes)).astype(F)
    t[..., :4] = rng.uniform(-2.0, 2.0, size=t[..., :4].shape)
    flat = t.reshape(-1, 5 + classes)
    n = flat.shape[0]
    # extremes: the objectness of some boxes, low class logits of others (a high one would be a tie: planted below)
    for k, v in enumerate((20.0, -20.0, 90.0, -90.0)):
        flat[k::17, 4] = v
    if classes >= 3:
        flat[3::11, 5 + classes - 1] = -90.0
        flat[5::13, 5 + classes - 2] = -20.0
    # make the maximum unique and clear: lift one class of every box above the rest by > 0.5 in the logit ...
    best = rng.integers(0, classes, size=n)
    rest_max = flat[:, 5:].max(axis=1)
    flat[np.arange(n), 5 + best] = np.minimum(rest_max + rng.uniform(0.5, 2.0, size=n), 12.0).astype(F)
    if classes >= 2:
        # ... except the planted ties: two equal logits (the first must win) and a pair above 20 (both give 1.0f)
        for k in range(0, n, 7):
            a, b = sorted(rng.choice(classes, size=2, replace=False))
            flat[k, 5:] = np.minimum(flat[k, 5:], 1.0)
            flat[k, 5 + a] = flat[k, 5 + b] = F(2.5)
        for k in range(3, n, 19):
            a, b = sorted(rng.choice(classes, size=2, replace=False))
            flat[k, 5:] = np.minimum(flat[k, 5:], 1.0)
            flat[k, 5 + a], flat[k, 5 + b] = (F(21.0), F(90.0)) if k % 2 else (F(25.0), F(20.5))
    return t


DECODE_GRIDS = ((5, 7), (13, 13))
DECODE_CLASSES = (1, 3, 80, 81)
DECODE_BATCH, DECODE_ANCHORS = 3, 3


def decode_case(grid, classes):
    h, w = grid
    return decode_logits(1000 * h + classes, DECODE_BATCH, h, w, DECODE_ANCHORS, classes)


def label_logits(seed, batch, h, w, anchors, classes, thresholds=THRESHOLDS):
    """(B, h, w, A, 5 + classes) float32 for the multi-label tests: about a third of the boxes pass 0.25, all pass 0.001, and
    every obj and s_c keeps the margin to all of ``thresholds`` (offenders are drawn again)."""
    rng = np.random.default_rng(seed)
    shape = (batch, h, w, anchors, 5 + classes)
    t = rng.uniform(-2.0, 2.0, size=shape).astype(F)
    high = rng.uniform(size=shape[:-1]) < 0.3
    t[..., 4] = np.where(high, rng.uniform(0.0, 4.0, size=shape[:-1]), rng.uniform(-6.0, -2.0, size=shape[:-1]))
    t[..., 5:] = rng.uniform(-2.5, 3.0, size=t[..., 5:].shape)
    for _ in range(200):
        obj, p = probabilities64(t)
        s = obj[..., None] * p
        bad_obj = np.zeros(obj.shape, bool)
        bad_s = np.zeros(s.shape, bool)
        for th in thresholds:
            bad_obj |= np.abs(obj - th) <= 2 * MARGIN
            bad_s |= (np.abs(s - th) <= 2 * MARGIN) & ~bad_obj[..., None]
        if not bad_obj.any() and not bad_s.any():
            return t
        t[..., 4][bad_obj] = rng.uniform(0.0, 4.0, size=int(bad_obj.sum()))
        t[..., 5:][bad_s] = rng.uniform(-2.5, 3.0, size=int(bad_s.sum()))
    raise AssertionError("no input with the margins found")


# the multi-label entry-point test: two heads, batch 2, the second head first in memory order of rows
LABEL_BATCH, LABEL_ANCHORS = 2, 3
LABEL_HEADS = (dict(h=4, w=6, classes=5, seed=41), dict(h=8, w=12, classes=80, seed=42))


def label_case():
    heads, off = [], 0
    for hd in LABEL_HEADS:
        t = label_logits(hd["seed"], LABEL_BATCH, hd["h"], hd["w"], LABEL_ANCHORS, hd["classes"])
        heads.append(dict(t=t, row_offset=off, new_coords=False))
        off += LABEL_ANCHORS * hd["h"] * hd["w"]
    return heads, off


# ---- the end-to-end network: tests/golden/cfg/mini.cfg with planted detection heads --------------------------------------------
# Both head convs get zero weights, so a head's logits are its biases at every cell and in every frame: anchor 0 of the fine
# head holds a box with TWO classes above the threshold (5, then 7), anchor 1 a box of class 7 only that scores below anchor
# 0's class 7 and overlaps it, so that the SECOND class of anchor 0's box suppresses it; everything else scores ~0.  Equal
# logits give every cell of an anchor the same score, and the order of equal scores is unspecified in Darknet and differs
# between the reference's suppression and this package's: the planted boxes are therefore small enough (about 7 x 7 pixels of
# the 48 x 32 input on a 4-pixel grid; 6 x 6 on the coarse head's 8-pixel grid) that boxes of ONE anchor in neighbouring cells
# overlap by an IoU of ~0.3 at most, under the float rule and the integer-pixel rule alike, and never suppress each other.
E2E_THRESH = 0.25
E2E_LOGITS = {          # (head index in cfg order, anchor): {attribute: logit}; the rest is -9 (tw, th: see E2E_SIZE)
    (1, 0): {4: 3.0, 5 + 5: 3.0, 5 + 7: 2.0},
    (1, 1): {4: 2.0, 5 + 7: 1.0},
    (0, 2): {4: 1.5, 5 + 2: 2.0},
}
# (tw, th) of the planted anchors (10 x 14, 23 x 27 and 344 x 319 pixels): anchors 0 and 1 of the fine head overlap by IoU ~0.9
E2E_SIZE = {(1, 0): (-0.3, -0.7), (1, 1): (-1.1, -1.3), (0, 2): (-4.0, -4.0)}


def e2e_head_bias(head, anchors=3, classes=80):
    bias = np.full((anchors, 5 + classes), -9.0, F)
    bias[:, :4] = 0.0
    for (hd, a), vals in E2E_LOGITS.items():
        if hd == head:
            for k, v in vals.items():
                bias[a, k] = v
            bias[a, 2], bias[a, 3] = E2E_SIZE[(hd, a)]
    return bias.reshape(-1)


def e2e_heads(batch, grids):
    """the planted logits as label() takes them; grids: [(h, w)] per head in cfg order"""
    heads, off = [], 0
    for head, (h, w) in enumerate(grids):
        bias = e2e_head_bias(head).reshape(3, -1)
        t = np.broadcast_to(bias, (batch, h, w) + bias.shape).astype(F).copy()
        heads.append(dict(t=t, row_offset=off, new_coords=False))
        off += 3 * h * w
    return heads, off
