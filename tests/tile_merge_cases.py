"""The case table of the seam merge (``y3_merge_tiled``): what ``y3_detect_tiled`` could have written for a batch of frames, as
data -- counts, int64 boxes, float32 scores, int64 classes, int32 combined rows, ``tile_rows`` -- in canonical order (class
ascending, score descending, row descending).  Built with no network and no GPU.  ``tile_rows`` is 1000 unless a case says
otherwise; slots past a frame's count hold a filler that nothing may read or write.

``CASES`` is the table, ``expected(case, frame, thr, wrong)`` the restatement's answer for one frame (computed once and shared),
``PLANTED`` the hand-computed answers of the named cases and ``RANDOM`` the names of the seeded random frames."""
import numpy as np

import tile_merge_restate as M

F = np.float32
FILL_BOX, FILL_PROB, FILL_CLS, FILL_ROW = 123456789, F(-3.0), 424242, 77


class Case(object):
    """One call: ``batch`` frames of ``capacity`` slots; thrs: the thresholds the call is made at."""

    def __init__(self, name, frames, tile_rows=1000, tiles=None, thrs=(0.5,), capacity=None):
        self.name, self.tile_rows, self.thrs = name, tile_rows, tuple(thrs)
        frames = [canonical(f) for f in frames]
        assert all(len(set(d[3] for d in f)) == len(f) for f in frames), "%s: a combined row appears twice" % name
        most_rows = max([d[3] for f in frames for d in f] + [0])
        if capacity is None:
            tiles = tiles if tiles is not None else most_rows // tile_rows + 1
            capacity = max(tiles * tile_rows, 1)
        assert capacity % tile_rows == 0 and most_rows < capacity and all(len(f) <= capacity for f in frames), name
        self.batch, self.capacity = len(frames), capacity
        self.count = np.array([len(f) for f in frames], np.int32)
        self.box = np.full((self.batch, capacity, 4), FILL_BOX, np.int64)
        self.prob = np.full((self.batch, capacity), FILL_PROB, F)
        self.cls = np.full((self.batch, capacity), FILL_CLS, np.int64)
        self.row = np.full((self.batch, capacity), FILL_ROW, np.int32)
        for b, f in enumerate(frames):
            for i, (box, score, c, r) in enumerate(f):
                self.box[b, i], self.prob[b, i], self.cls[b, i], self.row[b, i] = box, score, c, r

    def frame(self, b):
        """(boxes, scores, classes, rows) of frame b up to its count."""
        n = int(self.count[b])
        return self.box[b, :n], self.prob[b, :n], self.cls[b, :n], self.row[b, :n]

    def alone(self, b):
        """Frame b as a batch of one, same capacity and tile_rows."""
        c = Case.__new__(Case)
        c.name, c.tile_rows, c.thrs, c.batch, c.capacity = "%s[%d]" % (self.name, b), self.tile_rows, self.thrs, 1, self.capacity
        c.count, c.box, c.prob, c.cls, c.row = (a[b:b + 1].copy() for a in (self.count, self.box, self.prob, self.cls, self.row))
        return c


def canonical(dets):
    """[(box, score, class, row), ...] in canonical order; scores become float32 first."""
    dets = [(tuple(int(v) for v in box), F(score), int(c), int(r)) for box, score, c, r in dets]
    return sorted(dets, key=lambda d: (d[2], -float(d[1]), -d[3]))


def is_canonical(prob, cls, rows):
    key = [(int(c), -float(p), -int(r)) for p, c, r in zip(prob, cls, rows)]
    return all(a < b for a, b in zip(key, key[1:]))          # strictly: no two detections share class, score and row


_EXPECTED = {}


def expected(case, b, thr, wrong=None):
    """The restatement on frame b of the case: (boxes (k, 4) int64, scores float32, classes int64, rows int32, members int32)."""
    key = (case.name, b, thr, wrong)
    if key not in _EXPECTED:
        box, prob, cls, row = case.frame(b)
        o = M.merge(box.tolist(), prob.tolist(), cls.tolist(), row.tolist(), case.tile_rows, thr, wrong=wrong)
        keep = {r: i for i, r in enumerate(row.tolist())}      # rows are unique: the score bits come from the input
        idx = [keep[r] for r in o[3]]
        _EXPECTED[key] = (np.array(o[0], np.int64).reshape(-1, 4), prob[idx], np.array(o[2], np.int64),
                          np.array(o[3], np.int32), np.array(o[4], np.int32))
    return _EXPECTED[key]


# ---- the planted cases ------------------------------------------------------------------------------------------------------------
A20, B20, C20 = (0, 0, 19, 19), (10, 0, 29, 19), (20, 0, 39, 19)
NEAR_HALF = float(np.nextafter(0.5, 0.0))


def _planted():
    cases = [
        Case("two halves", [[((10, 10, 40, 50), 0.9, 0, 5), ((30, 10, 70, 50), 0.8, 0, 1005)]], thrs=(0.3,)),
        Case("exact tie", [[((0, 0, 9, 9), 0.9, 0, 5), ((5, 0, 14, 9), 0.8, 0, 1005)]], thrs=(0.5, NEAR_HALF)),
        Case("chain", [[(A20, 0.9, 0, 5), (B20, 0.8, 0, 1005), (C20, 0.7, 0, 2005)]], thrs=(0.4,)),
        Case("same tile", [[((0, 0, 19, 19), 0.9, 0, 5), ((2, 2, 17, 17), 0.8, 0, 6), ((1, 1, 18, 18), 0.1, 0, 1001)]]),
        Case("containment", [[((0, 0, 99, 99), 0.9, 3, 7), ((20, 30, 39, 59), 0.8, 3, 1007)]], thrs=(1.0, 0.999)),
        Case("other class", [[((0, 0, 99, 99), 0.9, 3, 7), ((0, 0, 99, 99), 0.8, 4, 1007), ((20, 30, 39, 59), 0.7, 5, 2007)]],
             thrs=(0.0, 0.5)),
        # degenerate boxes (x2 = x1 - 1: width 0; x2 < x1 - 1: negative width; the same in y) between matching neighbours
        Case("degenerate", [[((5, 5, 4, 30), 0.95, 0, 2001), ((0, 0, 19, 19), 0.9, 0, 5), ((10, 0, 9, 19), 0.8, 0, 1001),
                             ((10, 0, 5, 19), 0.7, 0, 1002), ((3, 12, 15, 11), 0.65, 0, 1003), ((3, 12, 15, 2), 0.64, 0, 3003),
                             ((1, 1, 18, 18), 0.6, 0, 1004), ((5, 5, 4, 30), 0.5, 0, 1005)]], thrs=(0.0, 0.5)),
        # the grown box of A reaches C, its original box does not; D lies in A's tile
        Case("grown", [[(A20, 0.9, 1, 5), (B20, 0.8, 1, 1005), ((25, 0, 44, 19), 0.7, 1, 2005), ((0, 0, 9, 9), 0.6, 1, 6)]],
             thrs=(0.2,)),
    ]
    answers = {
        ("two halves", 0.3): [((10, 10, 70, 50), 0.9, 5, 2)],
        ("exact tie", 0.5): [((0, 0, 9, 9), 0.9, 5, 1), ((5, 0, 14, 9), 0.8, 1005, 1)],
        ("exact tie", NEAR_HALF): [((0, 0, 14, 9), 0.9, 5, 2)],
        ("chain", 0.4): [((0, 0, 29, 19), 0.9, 5, 2), (C20, 0.7, 2005, 1)],
        ("same tile", 0.5): [((0, 0, 19, 19), 0.9, 5, 2), ((2, 2, 17, 17), 0.8, 6, 1)],
        ("containment", 1.0): [((0, 0, 99, 99), 0.9, 7, 1), ((20, 30, 39, 59), 0.8, 1007, 1)],
        ("containment", 0.999): [((0, 0, 99, 99), 0.9, 7, 2)],
        ("other class", 0.0): [((0, 0, 99, 99), 0.9, 7, 1), ((0, 0, 99, 99), 0.8, 1007, 1), ((20, 30, 39, 59), 0.7, 2007, 1)],
        ("degenerate", 0.5): [((5, 5, 4, 30), 0.95, 2001, 1), ((0, 0, 19, 19), 0.9, 5, 2), ((10, 0, 9, 19), 0.8, 1001, 1),
                              ((10, 0, 5, 19), 0.7, 1002, 1), ((3, 12, 15, 11), 0.65, 1003, 1), ((3, 12, 15, 2), 0.64, 3003, 1),
                              ((5, 5, 4, 30), 0.5, 1005, 1)],
    }
    return cases, answers


# ---- generated cases ----------------------------------------------------------------------------------------------------------------
def clustered(seed, sizes, tiles, tile_rows, origin=(0, 0), span=900, n_ties=0, whole=0.25, per_object=2.2, skew=1.0):
    """A frame of sum(sizes) detections, class c holding sizes[c] of them: every class has its own objects (about one per
    ``per_object`` detections, the first ones seen more often when ``skew`` > 1) scattered over ``span`` pixels from ``origin``; a detection is an object's whole box (jittered) or a random part
    of it that reaches a little past one side, seen from a random tile.  n_ties: per class, pairs of equal boxes shifted by
    exactly half their width, in different tiles, far from everything else: their IoS is exactly 1/2."""
    rng = np.random.default_rng(seed)
    total = int(sum(sizes))
    scores = rng.permutation(total * 4)[:total].astype(np.float64) / (total * 4) * 0.9 + 0.05     # all different in float32
    assert len(set(F(scores).tolist())) == total
    offsets = [rng.permutation(tile_rows).tolist() for _ in range(tiles)]     # per tile: every row of it at most once
    dets = []
    for c, size in enumerate(sizes):
        ties = min(n_ties, size // 4)
        n_obj = max(1, int((size - 2 * ties) / per_object))
        obj = []
        for _ in range(n_obj):
            w, h = int(rng.integers(20, 81)), int(rng.integers(20, 81))
            x, y = origin[0] + int(rng.integers(0, span)), origin[1] + int(rng.integers(0, span))
            obj.append((x, y, x + w - 1, y + h - 1))
        boxes = []
        for t in range(ties):
            w, h = 2 * int(rng.integers(5, 20)), int(rng.integers(8, 30))
            x, y = origin[0] + span + 200 + 100 * t, origin[1] - 300 - 100 * c
            t0 = int(rng.integers(0, tiles))
            boxes.append(((x, y, x + w - 1, y + h - 1), t0))
            boxes.append(((x + w // 2, y, x + w // 2 + w - 1, y + h - 1), (t0 + 1 + int(rng.integers(0, tiles - 1))) % tiles))
        while len(boxes) < size:
            x1, y1, x2, y2 = obj[int(n_obj * rng.random() ** skew)]
            if rng.random() < whole:
                j = rng.integers(-2, 3, size=4)
                box = (x1 + j[0], y1 + j[1], x2 + j[2], y2 + j[3])
            else:
                w, h = x2 - x1 + 1, y2 - y1 + 1
                pw, ph = int(rng.integers(w // 3, w + 1)), int(rng.integers(h // 3, h + 1))
                px, py = x1 + int(rng.integers(-3, w - pw + 4)), y1 + int(rng.integers(-3, h - ph + 4))
                box = (px, py, px + pw - 1, py + ph - 1)
            boxes.append((tuple(int(v) for v in box), int(rng.integers(0, tiles))))
        for box, tile in boxes:
            dets.append((box, scores[len(dets)], c, tile * tile_rows + offsets[tile].pop()))
    return dets


def _chunk_crossing(size, cls, tile_rows, x0=0):
    """``size`` detections of one class in score order: the first third are whole objects in tile 0 (keepers), the rest parts of
    object (index mod that third) seen from tiles 1 and 2 -- and every fifth of them from tile 0 itself, which stays.  With 129
    the keeper at lane 42 of chunk 0 takes lane 0 of chunk 2."""
    n_obj = max(1, size // 3)
    dets = []
    for i in range(size):
        k = i % n_obj
        x, y = x0 + 50 * (k % 40), 50 * (k // 40)
        if i < n_obj:
            box, tile = (x, y, x + 29, y + 29), 0
        else:
            part = i // n_obj
            box = (x + 3 * part, y + 2, x + 29, y + 20 + part % 7)
            tile = 0 if i % 5 == 0 else 1 + i % 2
        dets.append((box, 0.99 - 0.0005 * i, cls, tile * tile_rows + (7 * i + cls) % tile_rows))
    return dets


def _generated():
    cases = []
    # class segments of 1, 63, 64, 65, 129 and 1500 detections in one frame; absorptions cross the chunk boundaries
    sizes = (1, 63, 64, 65, 129, 1500)
    dets = []
    for c, size in enumerate(sizes):
        dets += _chunk_crossing(size, c, 2000)
    dets = [(box, score, c, (r // 2000) * 2000 + i) for i, (box, score, c, r) in enumerate(dets)]       # unique rows
    cases.append(Case("segments 1 63 64 65 129 1500", [dets], tile_rows=2000, tiles=3, thrs=(0.5,)))
    cases.append(Case("segments clustered", [clustered(5, sizes, 5, 2000)], tile_rows=2000, tiles=5, thrs=(0.5, 0.0)))
    # wide coordinates: negative, and past +-16000, where the int64 / float64 pair test runs
    cases.append(Case("wide", [clustered(6, (40, 90), 4, 1000, origin=(40000, -20900), span=300, n_ties=2)], tiles=4,
                      thrs=(0.5, NEAR_HALF)))
    cases.append(Case("negative", [clustered(7, (50, 70), 4, 1000, origin=(-16100, -15000), span=400, n_ties=2)], tiles=4,
                      thrs=(0.5, NEAR_HALF)))
    # one class whose first chunk is narrow and whose second is wide: 64 narrow keepers and parts, then boxes that start inside
    # the narrow range and end past 16000 (they overlap narrow ones), then far ones
    narrow = _chunk_crossing(64, 0, 1000, x0=13000)
    wide = []
    for i in range(40):
        x, y = 13000 + 50 * (i % 21), 50 * (i // 21)
        wide.append(((x + 5, y, 16500 + i, y + 29) if i % 2 else (x + 2, y + 2, x + 25, y + 25), 0.5 - 0.001 * i, 0,
                     (1 + i % 3) * 1000 + 500 + i))
        wide.append(((40000 + 40 * i, 7, 40000 + 40 * i + 59, 60), 0.4 - 0.001 * i, 0, (i % 4) * 1000 + 600 + i))
    cases.append(Case("narrow chunk meets wide chunk", [narrow + wide], tiles=4, thrs=(0.5, 0.1)))
    # more segments than waves: 80 classes; and 2000 classes of one detection each
    cases.append(Case("80 classes", [clustered(8, tuple(3 + (7 * c) % 23 for c in range(80)), 6, 1000)], tiles=6))
    one_each = [((10 * (c % 7), 0, 10 * (c % 7) + 30, 30), 0.9 - c * 1e-4, c - 1000, (c % 3) * 1000 + c // 3) for c in range(2000)]
    cases.append(Case("2000 classes", [one_each], tiles=3, thrs=(0.0,)))
    # a batch of three frames, counts 0, 1 and many, at two tile_rows that divide the capacity of 3000
    many = clustered(9, (70, 200, 30), 6, 500)
    for tile_rows in (500, 1000):
        cases.append(Case("batch tile_rows %d" % tile_rows, [[], [((3, 4, 50, 60), 0.7, 2, 2999)], many], tile_rows=tile_rows,
                          capacity=3000, thrs=(0.5,)))
    # count == capacity: 2 tiles of 150 rows, all 300 slots taken
    full = clustered(10, (120, 180), 2, 300)
    order = np.random.default_rng(10).permutation(300)        # every row exactly once
    full = [(box, score, c, int(order[i])) for i, (box, score, c, r) in enumerate(full)]
    cases.append(Case("count equals capacity", [full], tile_rows=150, capacity=300, thrs=(0.5,)))
    # one tile: nothing can match
    cases.append(Case("one tile", [clustered(11, (100, 100), 1, 1000)], tiles=1, thrs=(0.0, 0.5)))
    return cases


RANDOM_SEEDS = (101, 102, 103)
RANDOM = tuple("random %d" % s for s in RANDOM_SEEDS)


def _random():
    """Three seeded frames of 600 clustered integer boxes in 3 classes and 7 tiles, merged at 0.5.  The generator's settings
    are fixed so that the right rule keeps about 290 of the 600 in groups of up to 15 and every wrong rule of the restatement
    gives another answer on each frame (tests/test_tile_merge_host.py asserts both)."""
    return [Case("random %d" % s, [clustered(s, (200, 200, 200), 7, 1000, span=700, n_ties=3, per_object=2.45, skew=1.6)],
                 tiles=7, thrs=(0.5,)) for s in RANDOM_SEEDS]


_P, PLANTED = _planted()
CASES = _P + _generated() + _random()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# the planted case that tells each wrong rule from the right one, with its threshold
TELLS = {"ge": ("exact tie", 0.5), "iou": ("two halves", 0.3), "same_tile": ("same tile", 0.5), "absorbing": ("chain", 0.4),
         "grown": ("grown", 0.2)}
