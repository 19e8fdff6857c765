"""Inputs that put ``detect_kernel`` (csrc/detect.hip) on its size limits and on its wide-box path.  Plain numpy, seeded, no
GPU: tests/test_detect_tail_host.py proves on the oracle alone that every case is what it claims to be, and
tests/test_gpu_detect_tail.py runs them through the kernel.

Forward-mode cases return ``(bbox_xywh (B, rows, 4) float32, class_prob (B, rows) float32, class_idx (B, rows) int64,
orig_hw [(H, W)] * B)``; NMS-mode cases return ``(tlbr (n, 4) int64, prob (n,) float32, cls (n,) int64)``.  Scores are distinct
within a class unless the case is about ties.

The kernel's sizes restated here: a class is cut into chunks of 64 candidates in score order; a chunk takes the 32-bit
suppression test only when every corner of every box in it lies strictly inside +-16000; phase 1 handles 8192 rows per pass;
the sort runs in LDS up to 4096 (padded) candidates; 1024 chunk flags serve the classes of more than one chunk."""
import numpy as np

F = np.float32
CHUNK = 64
I32_LIM = 16000          # box_fits_i32
PASS_ROWS = 8192         # kIt * kThreads
MAX_FLAGS = 1024         # kMaxFlags
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- the kernel's order and chunking ------------------------------------------------------------------------------------------
def sorted_chunks(prob, cls=None):
    """The documented order of the tail (class ascending, score descending, higher position first) and its chunking:
    ``(order, chunks)`` with ``order`` the positions 0..n-1 in that order and ``chunks`` a list of ``(class, j, positions)``,
    chunk ``j`` of a class holding its candidates ``64 * j .. 64 * j + 63`` in score order."""
    prob = np.asarray(prob, F)
    n = len(prob)
    cls = np.zeros(n, np.int64) if cls is None else np.asarray(cls, np.int64)
    order = np.lexsort((-np.arange(n), -prob.astype(np.float64), cls))
    chunks = []
    ocls = cls[order]
    starts = np.nonzero(np.r_[True, ocls[1:] != ocls[:-1]])[0] if n else np.zeros(0, np.int64)
    ends = np.r_[starts[1:], n]
    for s, e in zip(starts.tolist(), ends.tolist()):
        for j, c0 in enumerate(range(s, e, CHUNK)):
            chunks.append((int(ocls[s]), j, order[c0:min(c0 + CHUNK, e)]))
    return order, chunks


def scaled_tlbr(box, hw):
    """The reference's tail on one frame's boxes: float32 product with the frame size, truncation, corners = centre -/+
    size // 2.  int64 (n, 4)."""
    b = np.array(box, F, copy=True)
    b[:, [0, 2]] *= F(hw[1])
    b[:, [1, 3]] *= F(hw[0])
    b = b.astype(np.int64)
    half = b[:, 2:4] // 2
    return np.concatenate([b[:, :2] - half, b[:, :2] + half], axis=1)


def is_wide(tlbr):
    """Boxes the 32-bit test may not see: a corner with |v| >= 16000."""
    return (np.abs(np.asarray(tlbr)) >= I32_LIM).any(axis=1)


def _distinct_scores(rng, n, lo, hi):
    """n distinct float32 in (lo, hi), shuffled."""
    v = (lo + (hi - lo) * (np.arange(n) + 0.5) / max(n, 1)).astype(F)
    assert len(np.unique(v)) == n and (n == 0 or (v.min() > F(lo) and v.max() < F(hi)))
    return v[rng.permutation(n)]


def _clusters(rng, n, per, lo=0.05, hi=0.95, size=(0.05, 0.3), sigma=0.01, log_sigma=0.08):
    """n float32 boxes in clusters of about ``per`` around random objects; -> (xywh (n, 4), object of every box)."""
    n_obj = max(1, n // per)
    ctr = rng.uniform(lo, hi, size=(n_obj, 2))
    osz = rng.uniform(size[0], size[1], size=(n_obj, 2))
    obj = rng.integers(0, n_obj, size=n)
    xy = ctr[obj] + rng.normal(0.0, sigma, size=(n, 2))
    wh = osz[obj] * np.exp(rng.normal(0.0, log_sigma, size=(n, 2)))
    return np.concatenate([xy, wh], axis=1).astype(F), obj


# ---- wide coordinates, forward mode (c) ---------------------------------------------------------------------------------------
WIDE_HW = (20000, 24000)
WIDE_CONTROL_HW = (608, 608)
WIDE_PROB_THRESH, WIDE_IOU = 0.1, 0.3


def wide_forward(seed=5, rows=3000, n_classes=3, per=10):
    """One 20000 x 24000 frame whose candidates lie on both sides of +-16000.  Half of the objects sit ON the line (their
    right edge at x = 16000 +- a few pixels, or their lower edge at y = 16000), so near-identical boxes fall on either side
    of it and suppress each other across the two code paths.  The scores are then handed out by rank so that the chunks of
    a class go narrow-only, wide-only, mixed, mixed, ...: every combination of a chunk and an earlier chunk occurs."""
    rng = np.random.default_rng(seed)
    h, w = WIDE_HW
    n_obj = rows // per
    kind = rng.choice(4, size=n_obj, p=[0.4, 0.2, 0.25, 0.15])     # on the x line / narrow / wide / on the y line
    osz = rng.uniform(0.03, 0.06, size=(n_obj, 2))
    cx = np.where(kind == 1, rng.uniform(0.05, 0.55, n_obj), rng.uniform(0.72, 0.93, n_obj))
    cx = np.where(kind == 0, rng.uniform(0.660, 0.673, n_obj) - osz[:, 0] / 2, cx)
    cx = np.where(kind == 3, rng.uniform(0.05, 0.55, n_obj), cx)
    cy = rng.uniform(0.08, 0.70, n_obj)
    cy = np.where(kind == 3, rng.uniform(0.795, 0.806, n_obj) - osz[:, 1] / 2, cy)
    obj = rng.permutation(np.repeat(np.arange(n_obj), per))[:rows]
    xy = np.stack([cx, cy], 1)[obj] + rng.normal(0.0, 0.003, size=(rows, 2))
    wh = osz[obj] * np.exp(rng.normal(0.0, 0.06, size=(rows, 2)))
    box = np.concatenate([xy, wh], axis=1).astype(F)
    cls = (obj % n_classes).astype(np.int64)
    wide = is_wide(scaled_tlbr(box, WIDE_HW))
    prob = np.empty(rows, F)
    thr = WIDE_PROB_THRESH
    for c in range(n_classes):
        members = np.nonzero(cls == c)[0]
        ncand = int(round(0.9 * len(members)))
        pools = {False: list(rng.permutation(members[~wide[members]])), True: list(rng.permutation(members[wide[members]]))}
        ranked = []
        while len(ranked) < ncand:
            want = "NWMM"[(len(ranked) // CHUNK) % 4]
            pick_wide = want == "W" or (want == "M" and len(ranked) % 2 == 1)
            pool = pools[pick_wide] if pools[pick_wide] else pools[not pick_wide]
            ranked.append(pool.pop())
        rest = pools[False] + pools[True]
        prob[ranked] = np.sort(_distinct_scores(rng, ncand, thr + 0.01, 0.99))[::-1]
        prob[rest] = _distinct_scores(rng, len(rest), 0.001, thr - 0.001)
    return box[None], prob[None], cls[None], [WIDE_HW]


# ---- running out of chunk flags (e) -------------------------------------------------------------------------------------------
FLAG_HW = (1080, 1920)
FLAG_PROB_THRESH, FLAG_IOU, FLAG_DK_THRESH = 0.05, 0.3, 0.45


def flag_exhaustion(seed=11, n_small=520, small=65, big=700, spare=116):
    """520 classes of 65 candidates (two chunks each) and one class of 700 (eleven chunks): 1051 flags wanted, 1024 there.
    Which class goes without depends on the order of an atomicAdd, so two frames: frame 0 gives the long class the highest
    class index, frame 1 the lowest (``520 - class``).  In every class the lowest score is a copy of the top-scoring box, so
    the last chunk always has a candidate that a survivor of chunk 0 suppresses."""
    rng = np.random.default_rng(seed)
    boxes, probs, clss = [], [], []
    for c in range(n_small + 1):
        m = big if c == n_small else small
        xywh, _ = _clusters(rng, m, 8 if m == small else 10, size=(0.04, 0.2))
        p = _distinct_scores(rng, m, 0.1, 0.9)
        xywh[np.argmin(p)] = xywh[np.argmax(p)]
        boxes.append(xywh)
        probs.append(p)
        clss.append(np.full(m, c, np.int64))
    xywh, _ = _clusters(rng, spare, 8)
    boxes.append(xywh)
    probs.append(_distinct_scores(rng, spare, 0.0, 0.049))            # below the threshold: never candidates
    clss.append(rng.integers(0, n_small + 1, size=spare).astype(np.int64))
    box, prob, cls = np.concatenate(boxes), np.concatenate(probs), np.concatenate(clss)
    perm = rng.permutation(len(prob))
    box, prob, cls = box[perm], prob[perm], cls[perm]
    return np.stack([box, box]), np.stack([prob, prob]), np.stack([cls, n_small - cls]), [FLAG_HW, FLAG_HW]


# ---- candidate-count boundaries (a) -------------------------------------------------------------------------------------------
COUNTS = [0, 1, 2, 3, 63, 64, 65, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8193]
COUNT_SHAPES = [(1080, 1920), (427, 640), (640, 427), (608, 608), (2, 1500), (333, 1000), (480, 640), (720, 1280),
                (1280, 720), (416, 416), (1000, 333), (500, 375), (375, 500), (1200, 1600), (600, 600), (768, 1024)]
COUNT_PROB_THRESH, COUNT_IOU = 0.25, 0.3
# (rows, placement): candidates anywhere; or in the last rows (even frames) / around row 8192, the pass boundary (odd frames)
COUNT_LAYOUTS = [(8200, "scatter"), (8192, "tail"), (8193, "tail"), (16385, "tail")]


def count_rows(count, rows, placement, frame, rng):
    """The rows of a frame's candidates (at most ``rows`` of them)."""
    k = min(count, rows)
    if placement == "scatter":
        return np.sort(rng.choice(rows, size=k, replace=False))
    if frame % 2 == 1 and rows > PASS_ROWS:
        start = min(max(PASS_ROWS - k // 2, 0), rows - k)
        return np.arange(start, start + k)
    return np.arange(rows - k, rows)


def count_boundaries(rows, placement, seed=21):
    """16 frames of ``rows`` predictions with COUNTS candidates (the last frame holds min(8193, rows)).  A frame's lowest
    candidate scores the threshold exactly and its highest non-candidate one ulp less.  Six classes, a class per object."""
    rng = np.random.default_rng(seed + rows)
    batch = len(COUNTS)
    thr = F(COUNT_PROB_THRESH)
    box = np.empty((batch, rows, 4), F)
    prob = np.empty((batch, rows), F)
    cls = np.empty((batch, rows), np.int64)
    for f in range(batch):
        box[f], obj = _clusters(rng, rows, 8)
        cls[f] = obj % 6
        cand = count_rows(COUNTS[f], rows, placement, f, rng)
        other = np.setdiff1d(np.arange(rows), cand)
        sc = _distinct_scores(rng, len(cand), float(thr), 0.97)
        if len(sc):
            sc[np.argmin(sc)] = thr
        lo = _distinct_scores(rng, len(other), 0.0, float(thr) - 0.01)
        if len(lo):
            lo[np.argmax(lo)] = np.nextafter(thr, F(0))
        prob[f, cand] = sc
        prob[f, other] = lo
    return box, prob, cls, list(COUNT_SHAPES)


# ---- class-chunk boundaries (b) -----------------------------------------------------------------------------------------------
CLASS_SIZES = [64, 65, 127, 128, 129]
MANY_CLASSES = 1025
SIGNED_CLASSES = [INT32_MIN, -70000, -1, 0, 3, INT32_MAX]
SIGNED_SIZES = [64, 65, 127, 128, 129, 130]
CLASS_ROWS = 1100
CLASS_PROB_THRESH, CLASS_IOU = 0.2, 0.3


def class_chunks(seed=31):
    """Seven frames of 1100 rows: five with a single class of 64 / 65 / 127 / 128 / 129 overlapping candidates; one with 1025
    candidates in 1025 classes spread over all of int32 (both ends included) on one and the same box; one with six classes
    of 64 .. 130 candidates whose indices are negative, zero and large (signed order)."""
    rng = np.random.default_rng(seed)
    batch, rows = len(CLASS_SIZES) + 2, CLASS_ROWS
    box = np.empty((batch, rows, 4), F)
    prob = np.empty((batch, rows), F)
    cls = np.empty((batch, rows), np.int64)
    for f in range(batch):
        box[f], _ = _clusters(rng, rows, 6, lo=0.2, hi=0.8, size=(0.1, 0.3))
        cls[f] = rng.integers(0, 4, size=rows)
        if f < len(CLASS_SIZES):
            sizes, ids = [CLASS_SIZES[f]], [7]
        elif f == len(CLASS_SIZES):
            ends = np.asarray([INT32_MIN, -1, 0, 1, INT32_MAX], np.int64)
            extra = np.setdiff1d(rng.integers(INT32_MIN, INT32_MAX, size=2 * MANY_CLASSES), ends)
            ids = np.r_[ends, rng.choice(extra, MANY_CLASSES - len(ends), replace=False)].tolist()
            sizes = [1] * MANY_CLASSES
        else:
            sizes, ids = SIGNED_SIZES, SIGNED_CLASSES
        k = sum(sizes)
        cand = np.sort(rng.choice(rows, size=k, replace=False))
        other = np.setdiff1d(np.arange(rows), cand)
        prob[f, cand] = _distinct_scores(rng, k, CLASS_PROB_THRESH + 0.01, 0.99)
        prob[f, other] = _distinct_scores(rng, len(other), 0.0, CLASS_PROB_THRESH - 0.01)
        cls[f, cand] = rng.permutation(np.repeat(np.asarray(ids, np.int64), sizes))
        if f == len(CLASS_SIZES):
            box[f, cand] = box[f, cand[0]]
        else:                                                   # few objects: the candidates of a class overlap
            box[f, cand], _ = _clusters(rng, k, 8 if len(sizes) == 1 else 24, lo=0.2, hi=0.8, size=(0.1, 0.3))
    return box, prob, cls, [(608, 608)] * batch


# ---- wide coordinates, NMS mode (d) -------------------------------------------------------------------------------------------
NMS_THRESHOLDS = [0.3, 0.5, 1.0 / 3.0, 0.0, 1.0]
TRANSLATIONS = [0, 15990, 20000, -20000, 10 ** 9]


def borderline_boxes(thr, n=1500):
    """The generator of tests/test_gpu_parity.py::test_nms_borderline_ratios_match_oracle: small integer boxes, degenerate
    ones (x2 = x1 - 1) included, whose inter / union lands on the thresholds all the time.  -> (boxes, prob, four classes)."""
    rs = np.random.RandomState(int(thr * 1000) + 7)
    tl = rs.randint(0, 12, size=(n, 2))
    wh = rs.randint(-1, 7, size=(n, 2))
    boxes = np.concatenate([tl, tl + wh], axis=1).astype(np.int64)
    boxes[0] = [0, 0, 9, 0]
    boxes[1] = [7, 0, 9, 0]                        # inter 3, union 10 with box 0
    prob = (rs.permutation(n).astype(F) + 1) / (n + 1)
    prob[0], prob[1] = 2.0, 1.5
    return boxes, prob, rs.randint(0, 4, size=n).astype(np.int64)


def translated(boxes, t):
    return boxes + np.int64(t)


LINE_CORNERS = [-16001, -16000, -15999, -1, 0, 15999, 16000, 16001]
FAR_CORNERS = LINE_CORNERS + [-10 ** 9, -40000, 40000, 10 ** 9]


def corner_boxes(corners, seed=41, n=480):
    """Boxes whose corners are drawn from ``corners`` (x1 <= x2, y1 <= y2), each one jittered by 0 / 1 pixel in half of the
    cases -- and the plain ones, on the line exactly, kept.  LINE_CORNERS: every box spans at most 32003 pixels, the largest
    the 32-bit test was sized for, and sits on either side of +-16000.  FAR_CORNERS adds boxes 80001 and 2 * 10^9 + 1 pixels
    wide: their areas pass 2^31, and the sum of two of them stays below 2^63.  Classes: four, signed."""
    rng = np.random.default_rng(seed)
    v = np.asarray(corners, np.int64)
    inside = v[np.abs(v) < I32_LIM]                                # a third of the boxes: every corner inside the line
    xs = np.sort(np.concatenate([rng.choice(inside, size=(n // 3, 2)), rng.choice(v, size=(n - n // 3, 2))]), axis=1)
    ys = np.sort(np.concatenate([rng.choice(inside, size=(n // 3, 2)), rng.choice(v, size=(n - n // 3, 2))]), axis=1)
    boxes = np.stack([xs[:, 0], ys[:, 0], xs[:, 1], ys[:, 1]], axis=1)
    # the inner corners of half of the boxes move inwards by 0..3 pixels: many different ratios, corners still on the line
    jit = rng.integers(0, 4, size=(n, 4)) * np.array([1, 1, -1, -1]) * (rng.random((n, 1)) < 0.5)
    moved = boxes + jit
    ok = (moved[:, 0] <= moved[:, 2]) & (moved[:, 1] <= moved[:, 3])
    boxes = np.where(ok[:, None], moved, boxes).astype(np.int64)
    for k, v in enumerate((16001, 16000, 15999)):                 # the largest box on either side of the line, and on it
        boxes[k] = [-v, -v, v, v]
    prob = _distinct_scores(rng, n, 0.0, 1.0)
    cls = np.asarray([INT32_MIN, -1, 0, INT32_MAX], np.int64)[rng.integers(0, 4, size=n)]
    return boxes, prob, cls


# ---- scores that are not ordinary probabilities (f) ---------------------------------------------------------------------------
SCORE_THRESHOLDS = [0.0, 0.05, -1.0]
SCORE_HW = (427, 640)
SCORE_IOU = 0.3


def score_edges(thr, seed=51, rows=600, n_classes=3):
    """One frame whose ``class_prob`` holds NaN, -inf, +inf, -0.0, +0.0, subnormals of both signs, negative values and the
    values one ulp on either side of ``thr`` (and ``thr`` itself).  Distinct within a class, -0.0 / +0.0 counting as a tie:
    class 0 holds -0.0 only, class 1 +0.0 only, and class 2 holds both, on boxes far from every other box (and from each
    other), where the order of a tie decides nothing."""
    rng = np.random.default_rng(seed + SCORE_THRESHOLDS.index(thr))
    box, obj = _clusters(rng, rows, 8, lo=0.2, hi=0.8, size=(0.05, 0.25))
    cls = (obj % n_classes).astype(np.int64)
    prob = _distinct_scores(rng, rows, -2.0, 0.98)
    t = F(thr)
    special = [F(np.inf), F(-np.inf), F(np.nan), t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf)),
               F(1e-45), F(-1e-45), F(1e-40), F(-1e-40), F(5.8e-39), F(-5.8e-39), F(1.1754944e-38), F(3.0e38), F(-3.0e38)]
    zeros = {0: [F(-0.0)], 1: [F(0.0)], 2: [F(-0.0), F(0.0)]}
    for c in range(n_classes):
        members = rng.permutation(np.nonzero(cls == c)[0])
        vals = list(zeros[c])
        for v in special + [F(np.nan)]:                          # thr 0.0: thr and its neighbours are there already
            if np.isnan(v) or not any(v == u for u in vals):
                vals.append(v)
        rows_c = members[:len(vals)]
        prob[rows_c] = vals
        for k, r in enumerate(rows_c):
            if prob[r] == 0:                                    # +-0.0: alone, outside the frame, small
                box[r] = [3.0 + c + 0.25 * k, -2.0 - c, 0.05, 0.05]
    return box[None], prob[None], cls[None], [SCORE_HW]


TIE_HW = (608, 608)
TIE_PROB_THRESH, TIE_IOU = 0.3, 0.3


def tied_isolated(seed=61, n=200, n_classes=2):
    """200 boxes that overlap nothing, one per cell of a 15 x 15 grid, with scores from five values (and some below the
    threshold): exact ties everywhere, none of which decides anything."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(225, size=n, replace=False)
    xy = np.stack([(cells % 15 + 0.5) / 15.0, (cells // 15 + 0.5) / 15.0], axis=1)
    wh = rng.uniform(0.01, 0.05, size=(n, 2))                    # a cell is 40 pixels, a box at most 31
    box = np.concatenate([xy, wh], axis=1).astype(F)
    prob = np.asarray([0.9, 0.5, 0.5000001, 0.3, 0.31, 0.1], F)[rng.integers(0, 6, size=n)]
    cls = rng.integers(0, n_classes, size=n).astype(np.int64)
    return box[None], prob[None], cls[None], [TIE_HW]


def tied_overlapping(seed=62, n=900, n_classes=2):
    """Clusters of overlapping boxes with scores from four values: which of two tied boxes survives is the implementation's
    choice (the reference's depends on ``argsort``), so only determinism and the output order are asserted on it."""
    rng = np.random.default_rng(seed)
    box, obj = _clusters(rng, n, 9, lo=0.1, hi=0.9, size=(0.05, 0.25))
    prob = np.asarray([0.9, 0.6, 0.45, 0.2], F)[rng.integers(0, 4, size=n)]
    cls = (obj % n_classes).astype(np.int64)
    return box[None], prob[None], cls[None], [TIE_HW]
