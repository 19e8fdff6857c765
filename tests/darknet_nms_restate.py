"""Darknet's suppression rule (src/box.c: box_iou, box_diou, box_diounms; do_nms_sort, diounms_sort) restated in numpy float32
scalars, independent of the package, plus the inputs the tests of the GPU path share.

Boxes are float32 ``(x, y, w, h)``, centre and size.  Every operation rounds once to float32 (numpy scalar arithmetic), except
the power, which is ``math.pow`` on Python floats rounded to float32 once:

    overlap(x1,w1,x2,w2) = min(x1 + w1/2, x2 + w2/2) - max(x1 - w1/2, x2 - w2/2)       min(p,q) = p < q ? p : q, max likewise
    I   = (ow < 0 || oh < 0) ? 0 : ow * oh
    U   = a.w*a.h + b.w*b.h - I
    iou = (I == 0 || U == 0) ? 0 : I / U
    cw  = max(a.x + a.w/2, b.x + b.w/2) - min(a.x - a.w/2, b.x - b.w/2)     ch likewise in y
    c   = cw*cw + ch*ch         d = (a.x-b.x)^2 + (a.y-b.y)^2
    "iou"        m = iou
    "greedynms"  m = (c == 0) ? iou : iou - d / c
    "diounms"    m = (c == 0) ? iou : iou - (float)pow((double)(d / c), (double)beta)
    a suppresses b  iff  m > thresh

``keep`` is the greedy loop, pair by pair; ``keep_fast`` is the same loop with one survivor measured against all later
candidates of its class at once (numpy float32 array arithmetic rounds each operation as the scalars do; the power is still
``math.pow`` per element) -- for the inputs of thousands of boxes; tests/test_darknet_nms_host.py pins one against the other.
The greedy loop: candidates in canonical order (class ascending, score descending, higher index first), classes
independent, a suppressed box suppresses nobody.  ``pow_nudge`` moves every computed power one float32 ulp up (+1) or down (-1):
tests/test_darknet_nms_host.py uses it to show that no committed input decides a box by the last bit of ``pow``.
"""
import math

import numpy as np

F = np.float32
KINDS = ("iou", "greedynms", "diounms")
TWO = F(2)
ZERO = F(0)


def _min(p, q):
    return p if p < q else q


def _max(p, q):
    return p if p > q else q


def overlap(x1, w1, x2, w2):
    left = _max(x1 - w1 / TWO, x2 - w2 / TWO)
    right = _min(x1 + w1 / TWO, x2 + w2 / TWO)
    return right - left


def box_iou(a, b):
    ow, oh = overlap(a[0], a[2], b[0], b[2]), overlap(a[1], a[3], b[1], b[3])
    inter = ZERO if (ow < 0 or oh < 0) else ow * oh
    union = a[2] * a[3] + b[2] * b[3] - inter
    return ZERO if (inter == 0 or union == 0) else inter / union


def measure(a, b, kind, beta=0.6, pow_nudge=0):
    """m of the ordered pair (a, b): float32 scalar.  a, b: sequences of four numpy float32."""
    with np.errstate(all="ignore"):
        iou = box_iou(a, b)
        if kind == "iou":
            return iou
        cw = _max(a[0] + a[2] / TWO, b[0] + b[2] / TWO) - _min(a[0] - a[2] / TWO, b[0] - b[2] / TWO)
        ch = _max(a[1] + a[3] / TWO, b[1] + b[3] / TWO) - _min(a[1] - a[3] / TWO, b[1] - b[3] / TWO)
        c = cw * cw + ch * ch
        dx, dy = a[0] - b[0], a[1] - b[1]
        d = dx * dx + dy * dy
        if c == 0:
            return iou
        if kind == "greedynms":
            return iou - d / c
        if kind != "diounms":
            raise ValueError(kind)
        term = F(math.pow(float(d / c), float(F(beta))))
        if pow_nudge:
            term = np.nextafter(term, F(np.inf) if pow_nudge > 0 else F(-np.inf))
        return iou - term


def canonical_order(prob, cls):
    """Indices by (class ascending, score descending, index descending)."""
    n = len(prob)
    cls = np.zeros(n, np.int64) if cls is None else np.asarray(cls)
    return sorted(range(n), key=lambda i: (int(cls[i]), -float(prob[i]), -i))


def keep(xywh, prob, cls=None, thresh=0.45, kind="iou", beta=0.6, pow_nudge=0):
    """Kept indices in canonical order."""
    xywh = np.asarray(xywh)
    assert xywh.dtype == np.float32
    prob = np.asarray(prob, np.float32)
    thr = F(thresh)
    n = len(prob)
    cls = np.zeros(n, np.int64) if cls is None else np.asarray(cls)
    kept = []
    alive = {}                                   # class -> kept boxes of that class so far
    for i in canonical_order(prob, cls):
        b = tuple(xywh[i, :4])
        mine = alive.setdefault(int(cls[i]), [])
        if any(measure(a, b, kind, beta, pow_nudge) > thr for a in mine):
            continue
        mine.append(b)
        kept.append(i)
    return kept


def measure_many(a, B, kind, beta=0.6, pow_nudge=0):
    """``measure(a, b, ...)`` for every row b of B (m, 4) float32 at once: float32 array (m,)."""
    def mx(p, q):
        return np.where(p > q, p, q)

    def mn(p, q):
        return np.where(p < q, p, q)

    with np.errstate(all="ignore"):
        ax, ay, aw, ah = (np.full(len(B), v, np.float32) for v in a)
        bx, by, bw, bh = B[:, 0], B[:, 1], B[:, 2], B[:, 3]
        ow = mn(ax + aw / TWO, bx + bw / TWO) - mx(ax - aw / TWO, bx - bw / TWO)
        oh = mn(ay + ah / TWO, by + bh / TWO) - mx(ay - ah / TWO, by - bh / TWO)
        inter = np.where((ow < 0) | (oh < 0), ZERO, ow * oh)
        union = aw * ah + bw * bh - inter
        iou = np.where((inter == 0) | (union == 0), ZERO, inter / union)
        if kind == "iou":
            return iou
        cw = mx(ax + aw / TWO, bx + bw / TWO) - mn(ax - aw / TWO, bx - bw / TWO)
        ch = mx(ay + ah / TWO, by + bh / TWO) - mn(ay - ah / TWO, by - bh / TWO)
        c = cw * cw + ch * ch
        dx, dy = ax - bx, ay - by
        d = dx * dx + dy * dy
        q = d / c
        assert q.dtype == np.float32 and iou.dtype == np.float32
        if kind == "diounms":
            b64 = float(F(beta))
            q = np.array([math.pow(float(v), b64) for v in q], np.float64).astype(np.float32)
            if pow_nudge:
                q = np.nextafter(q, F(np.inf) if pow_nudge > 0 else F(-np.inf))
        elif kind != "greedynms":
            raise ValueError(kind)
        return np.where(c == 0, iou, iou - q)


def keep_fast(xywh, prob, cls=None, thresh=0.45, kind="iou", beta=0.6, pow_nudge=0):
    """``keep`` for finite boxes, one survivor against all later candidates of its class per step."""
    xywh = np.asarray(xywh)
    assert xywh.dtype == np.float32 and np.isfinite(xywh).all()
    prob = np.asarray(prob, np.float32)
    thr = F(thresh)
    n = len(prob)
    cls = np.zeros(n, np.int64) if cls is None else np.asarray(cls)
    order = np.array(canonical_order(prob, cls), np.int64)
    dead = np.zeros(n, bool)                     # by position in `order`
    ocls = cls[order]
    kept = []
    for pos in range(n):
        if dead[pos]:
            continue
        i = order[pos]
        kept.append(int(i))
        later = np.nonzero((ocls[pos + 1:] == ocls[pos]) & ~dead[pos + 1:])[0] + pos + 1
        if len(later):
            m = measure_many(tuple(xywh[i, :4]), xywh[order[later], :4], kind, beta, pow_nudge)
            dead[later[m > thr]] = True
    return kept


def clusters(seed, n, n_classes, per_cluster=12, centre_sigma=0.03, log_size_sigma=0.15):
    """``n`` boxes in clusters of ``per_cluster`` around random objects: (xywh float32 (n,4), prob float32, cls int64)."""
    rng = np.random.default_rng(seed)
    n_obj = (n + per_cluster - 1) // per_cluster
    ctr = rng.uniform(0.1, 0.9, size=(n_obj, 2))
    size = rng.uniform(0.05, 0.4, size=(n_obj, 2))
    ocls = rng.integers(0, n_classes, size=n_obj)
    obj = np.repeat(np.arange(n_obj), per_cluster)[:n]
    xy = ctr[obj] + rng.normal(0.0, centre_sigma, size=(n, 2))
    wh = size[obj] * np.exp(rng.normal(0.0, log_size_sigma, size=(n, 2)))
    prob = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    perm = rng.permutation(n)
    xywh = np.concatenate([xy, wh], 1).astype(np.float32)[perm]
    return xywh, prob[perm], ocls[obj][perm].astype(np.int64)


THRESH, BETA = 0.45, 0.6
# (seed, n, classes) of the committed inputs: in every one of them the three kinds keep three different sets, and none is
# fragile (tests/test_darknet_nms_host.py asserts both).
CASES = [(seed, n, nc) for n, nc in ((300, 1), (600, 3), (200, 80)) for seed in range(12)]
# one class of 2400 candidates (38 chunks of 64 on 16 wavefronts: the flag chain); 5000 candidates in 3 classes (more than
# the 4096 the kernel sorts in LDS: the global-memory sort)
BIG_CASES = [(100, 2400, 1), (101, 5000, 3)]


# ---- forward-output inputs of the Detector tests (built like _synthetic_outputs of tests/test_gpu_letterbox.py) -------------
DETECT_BATCH, DETECT_ROWS, DETECT_SEED, DETECT_PROB_THRESH = 16, 1500, 31, 0.6
DETECT_NET = (608, 608)
DETECT_SHAPES = [(1080, 1920), (427, 640), (640, 427), (608, 608), (2, 1500), (333, 1000), (480, 640), (720, 1280),
                 (1280, 720), (416, 416), (1000, 333), (500, 375), (375, 500), (1200, 1600), (600, 600), (768, 1024)]


def detector_inputs(batch=DETECT_BATCH, rows=DETECT_ROWS, seed=DETECT_SEED):
    rng = np.random.default_rng(seed)
    box = np.empty((batch, rows, 4), np.float32)
    box[..., :2] = rng.uniform(-0.3, 1.3, size=(batch, rows, 2))      # centres outside [0, 1] too
    box[..., 2:] = rng.uniform(0.0, 0.6, size=(batch, rows, 2))
    prob = rng.uniform(0.0, 1.0, size=(batch, rows)).astype(np.float32)
    cls = rng.integers(0, 5, size=(batch, rows)).astype(np.int64)
    return box, prob, cls


def detect_keep_rows(box, prob, cls, prob_thresh, thresh, kind, beta=0.6, pow_nudge=0):
    """One frame: the prediction rows Darknet's rule keeps among those with prob >= prob_thresh (float32), canonical order.
    box (rows, 4) float32: the boxes the rule sees (letterbox-corrected where that applies)."""
    rows = np.nonzero(prob >= F(prob_thresh))[0]
    kept = keep_fast(np.ascontiguousarray(box[rows]), prob[rows], cls[rows], thresh, kind, beta, pow_nudge)
    return [int(rows[k]) for k in kept]
