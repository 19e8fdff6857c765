"""The inputs of tests/test_gpu_detect_tail.py are what they claim to be (no GPU): asserted on the oracle alone
(``oracle.darknet_oracle.postprocess`` / ``non_max_suppression``) and on ``sorted_chunks``, the kernel's documented order and
chunking restated in numpy.  These are conditions, not measurements: a case that stops reaching its path fails here."""
import time

import numpy as np
import pytest

from oracle import darknet_oracle as orc

import detect_tail_cases as C

F = np.float32
ORACLE_SECONDS = 10.0


def _oracle(case, prob_thresh, iou):
    box, prob, cls, hw = case
    t0 = time.perf_counter()
    want = orc.postprocess(box, prob, cls, hw, F(prob_thresh), iou, audit=True)
    dt = time.perf_counter() - t0
    print("oracle: %d frames, %d candidates, %d kept, %.2f s" % (len(want), sum(len(w[4]) for w in want),
                                                                 sum(len(w[3]) for w in want), dt))
    assert dt < ORACLE_SECONDS
    return want


def _iou(a, b):
    """(len(a), len(b)) float64: the reference's measure, +1 widths, int64 / int64."""
    iw = np.maximum(0, np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + 1)
    ih = np.maximum(0, np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + 1)
    inter = iw * ih
    area = lambda t: (t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def _frame(case, want, f, prob_thresh):
    """One frame's candidates: (rows, tlbr, prob, cls, kept mask), after checking the restated scaling against the oracle."""
    box, prob, cls, hw = case
    w_tlbr, w_prob, w_cls, w_rows, w_cand, _ = want[f]
    with np.errstate(invalid="ignore"):
        cand = np.nonzero(prob[f] >= F(prob_thresh))[0]
    assert np.array_equal(cand, w_cand)
    tlbr = C.scaled_tlbr(box[f, cand], hw[f])
    kept = np.isin(cand, w_rows)
    by_row = {int(r): k for k, r in enumerate(cand)}
    idx = [by_row[int(r)] for r in w_rows]
    assert np.array_equal(tlbr[idx], w_tlbr) and np.array_equal(cls[f, cand][idx], w_cls)
    assert np.abs(tlbr).max(initial=0) < 2 ** 62                      # no scaled coordinate near the ends of int64
    return cand, tlbr, prob[f, cand], cls[f, cand], kept


def _distinct_within_class(prob, cls):
    for c in np.unique(cls):
        p = prob[cls == c]
        assert len(np.unique(p)) == len(p), "class %d has tied scores" % c


def test_sorted_chunks_states_the_documented_order():
    prob = np.array([0.5, 0.9, 0.5, 0.1, 0.9, 0.7], F)
    cls = np.array([1, 0, 1, -3, 0, 1], np.int64)
    order, chunks = C.sorted_chunks(prob, cls)
    assert order.tolist() == [3, 4, 1, 5, 2, 0]                      # class ascending, score descending, higher position first
    assert [(c, j, p.tolist()) for c, j, p in chunks] == [(-3, 0, [3]), (0, 0, [4, 1]), (1, 0, [5, 2, 0])]
    order, chunks = C.sorted_chunks(np.linspace(0.0, 1.0, 130).astype(F))
    assert order.tolist() == list(range(129, -1, -1))
    assert [(j, len(p)) for _, j, p in chunks] == [(0, 64), (1, 64), (2, 2)]
    assert C.sorted_chunks(np.zeros(0, F))[1] == []


def test_wide_case_reaches_both_paths_and_every_chunk_pairing():
    case = C.wide_forward()
    want = _oracle(case, C.WIDE_PROB_THRESH, C.WIDE_IOU)
    cand, tlbr, prob, cls, kept = _frame(case, want, 0, C.WIDE_PROB_THRESH)
    _distinct_within_class(prob, cls)
    wide = C.is_wide(tlbr)
    print("candidates %d, wide %d, kept %d, wide kept %d" % (len(cand), wide.sum(), kept.sum(), (wide & kept).sum()))
    assert wide.sum() >= 200 and (~wide).sum() >= 200
    assert (wide & kept).sum() >= 20 and (wide & ~kept).sum() >= 20     # the oracle keeps some wide boxes and suppresses some
    assert (~wide & ~kept).sum() >= 20
    _, chunks = C.sorted_chunks(prob, cls)
    mixed = [1 for _, _, pos in chunks if wide[pos].any() and not wide[pos].all()]
    assert len(mixed) >= 10
    narrow_after_wide_survivor = wide_after_narrow_survivor = 0
    for c, j, pos in chunks:
        for c2, j2, pos2 in chunks:
            if c2 != c or j2 >= j:
                continue
            if not wide[pos].any() and (wide[pos2] & kept[pos2]).any():
                narrow_after_wide_survivor += 1
            if wide[pos].any() and not wide[pos2].any() and kept[pos2].any():
                wide_after_narrow_survivor += 1
    assert narrow_after_wide_survivor >= 1 and wide_after_narrow_survivor >= 1
    # and the two kinds meet: a narrow box suppressed by a wide survivor alone, a wide box by a narrow survivor alone
    m = _iou(tlbr, tlbr[kept]) > C.WIDE_IOU
    same = (cls[:, None] == cls[kept][None, :]) & (prob[:, None] < prob[kept][None, :])
    by_wide, by_narrow = (m & same & wide[kept][None, :]).any(1), (m & same & ~wide[kept][None, :]).any(1)
    assert (~kept & ~wide & by_wide & ~by_narrow).sum() >= 5 and (~kept & wide & by_narrow & ~by_wide).sum() >= 5
    # the same boxes on the control frame: nothing wide
    box, p, k, _ = case
    assert not C.is_wide(C.scaled_tlbr(box[0], C.WIDE_CONTROL_HW)).any()


def test_flag_case_asks_for_more_flags_than_there_are():
    case = C.flag_exhaustion()
    want = _oracle(case, C.FLAG_PROB_THRESH, C.FLAG_IOU)
    for f in range(2):
        cand, tlbr, prob, cls, kept = _frame(case, want, f, C.FLAG_PROB_THRESH)
        assert len(cand) == 520 * 65 + 700
        _distinct_within_class(prob, cls)
        _, chunks = C.sorted_chunks(prob, cls)
        per_class = {}
        for c, j, pos in chunks:
            per_class.setdefault(c, []).append(pos)
        flags = sum(len(v) for v in per_class.values() if len(v) > 1)
        assert flags == 520 * 2 + 11 > C.MAX_FLAGS
        assert max(len(v) for v in per_class.values()) >= 10
        assert (max(per_class, key=lambda c: len(per_class[c])) == 520) == (f == 0)      # the long class: last, then first
        for c, parts in per_class.items():
            assert len(parts) > 1
            found = False
            for j in range(1, len(parts)):
                lost = parts[j][~kept[parts[j]]]
                earlier = np.concatenate(parts[:j])
                earlier = earlier[kept[earlier]]
                if len(lost) and len(earlier) and (_iou(tlbr[lost], tlbr[earlier]) > C.FLAG_IOU).any():
                    found = True
                    break
            assert found, "class %d: nothing in a later chunk is suppressed by a survivor of an earlier one" % c


@pytest.mark.parametrize("rows,placement", C.COUNT_LAYOUTS)
def test_count_case_has_exactly_the_stated_candidates(rows, placement):
    case = C.count_boundaries(rows, placement)
    box, prob, cls, hw = case
    want = _oracle(case, C.COUNT_PROB_THRESH, C.COUNT_IOU)
    assert prob.shape == (16, rows)
    for f, count in enumerate(C.COUNTS):
        cand, tlbr, p, c, kept = _frame(case, want, f, C.COUNT_PROB_THRESH)
        assert len(cand) == min(count, rows)
        _distinct_within_class(p, c)
        if len(cand):
            assert p.min() == F(C.COUNT_PROB_THRESH)                                   # on the threshold: a candidate
        if len(cand) < rows:
            assert np.delete(prob[f], cand).max() == np.nextafter(F(C.COUNT_PROB_THRESH), F(0))     # one ulp below: none
        if len(cand) > 3:
            assert 0 < kept.sum() < len(cand)
        if placement == "tail" and len(cand):
            if f % 2 == 1 and rows > C.PASS_ROWS:
                assert cand[0] < C.PASS_ROWS <= cand[-1] or len(cand) == 1              # across the pass boundary
            else:
                assert cand[-1] == rows - 1 and cand[0] == rows - len(cand)
    assert len(want[-1][4]) == min(8193, rows)


def test_class_case_has_exactly_the_stated_class_sizes():
    case = C.class_chunks()
    want = _oracle(case, C.CLASS_PROB_THRESH, C.CLASS_IOU)
    for f, size in enumerate(C.CLASS_SIZES):
        cand, tlbr, p, c, kept = _frame(case, want, f, C.CLASS_PROB_THRESH)
        assert len(cand) == size and len(np.unique(c)) == 1
        _distinct_within_class(p, c)
        assert 0 < kept.sum() < size
        if size > 64:                                                # something past the first chunk goes
            order, _ = C.sorted_chunks(p, c)
            assert not kept[order[64:]].all()
    f = len(C.CLASS_SIZES)
    cand, tlbr, p, c, kept = _frame(case, want, f, C.CLASS_PROB_THRESH)
    assert len(cand) == len(np.unique(c)) == C.MANY_CLASSES == 1025 and kept.all()
    assert c.min() == C.INT32_MIN and c.max() == C.INT32_MAX and (c < 0).sum() > 100 and (c > 0).sum() > 100
    assert (tlbr == tlbr[0]).all()                                   # one box: only the classes keep them apart
    cand, tlbr, p, c, kept = _frame(case, want, f + 1, C.CLASS_PROB_THRESH)
    assert [int((c == k).sum()) for k in C.SIGNED_CLASSES] == C.SIGNED_SIZES and len(cand) == sum(C.SIGNED_SIZES)
    _distinct_within_class(p, c)
    for k in C.SIGNED_CLASSES:
        assert 0 < kept[c == k].sum() < (c == k).sum()


@pytest.mark.parametrize("thr", C.NMS_THRESHOLDS)
def test_translated_borderline_boxes_mix_the_paths(thr):
    boxes, prob, cls = C.borderline_boxes(thr)
    assert len(np.unique(prob)) == len(prob) and min(np.bincount(cls)) > 64
    assert not C.is_wide(boxes).any()
    t0 = time.perf_counter()
    want = sorted(int(i) for i in orc.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=thr))
    assert time.perf_counter() - t0 < ORACLE_SECONDS
    for t in C.TRANSLATIONS:
        moved = C.translated(boxes, t)
        assert moved.dtype == np.int64
        wide = C.is_wide(moved)
        for k in (None, cls):
            _, chunks = C.sorted_chunks(prob, k)
            mixed = sum(1 for _, _, pos in chunks if wide[pos].any() and not wide[pos].all())
            if t == 15990:
                assert mixed >= 10                                   # some boxes cross 16000: chunks of both kinds
            else:
                assert mixed == 0 and wide.all() == (t != 0)
        # a translation changes no intersection and no union
        assert sorted(int(i) for i in orc.non_max_suppression(moved, prob, class_idx=cls, iou_thresh=thr)) == want
    if thr in (0.5, 1.0):                                            # pairs ON the threshold exist: > and >= differ
        m = _iou(boxes, boxes)
        assert ((m == thr) & (cls[:, None] == cls[None, :]) & ~np.eye(len(prob), dtype=bool)).any()


@pytest.mark.parametrize("name", ["line", "far"])
def test_corner_boxes_sit_on_the_line(name):
    corners = C.LINE_CORNERS if name == "line" else C.FAR_CORNERS
    boxes, prob, cls = C.corner_boxes(corners)
    assert boxes.dtype == np.int64 and (boxes[:, 0] <= boxes[:, 2]).all() and (boxes[:, 1] <= boxes[:, 3]).all()
    assert len(np.unique(prob)) == len(prob) and min(np.unique(cls, return_counts=True)[1]) > 64
    for v in (15999, 16000, 16001, -15999, -16000, -16001):
        assert (boxes == v).any()
    wide = C.is_wide(boxes)
    assert wide.sum() > 64 and (~wide).sum() > 64
    area = (boxes[:, 2] - boxes[:, 0] + 1).astype(object) * (boxes[:, 3] - boxes[:, 1] + 1).astype(object)
    assert 2 * max(area) < 2 ** 63                                   # the reference's int64 sums do not wrap
    if name == "far":
        assert sum(a >= 2 ** 31 for a in area) > 64                  # what 32-bit integers cannot hold
    else:
        assert max(area) == 32003 ** 2
    for k in (None, cls):
        for thr in (0.3, 0.5):
            t0 = time.perf_counter()
            kept = orc.non_max_suppression(boxes, prob, class_idx=k, iou_thresh=thr)
            assert time.perf_counter() - t0 < ORACLE_SECONDS
            assert 10 < len(kept) < len(prob) - 10
            assert wide[kept].any() and not wide[kept].all()


@pytest.mark.parametrize("thr", C.SCORE_THRESHOLDS)
def test_score_case_holds_every_special_value(thr):
    case = C.score_edges(thr)
    box, prob, cls, hw = case
    want = _oracle(case, thr, C.SCORE_IOU)
    cand, tlbr, p, c, kept = _frame(case, want, 0, thr)
    t = F(thr)
    bits = prob[0].view(np.uint32)
    for k in range(3):
        mine = prob[0][cls[0] == k]
        assert np.isnan(mine).sum() >= 2 and np.isposinf(mine).sum() == 1 and np.isneginf(mine).sum() == 1
        for v in (t, np.nextafter(t, F(np.inf)), np.nextafter(t, F(-np.inf)), F(1e-45), F(-1e-45), F(1e-40), F(-3.0e38)):
            assert (mine == v).sum() == 1 or (v == 0 and (mine == 0).sum() in (1, 2))
        fin = mine[~np.isnan(mine)]
        nonzero = fin[fin != 0]
        assert len(np.unique(nonzero)) == len(nonzero)               # distinct; +-0.0 is the one tie
        assert (fin < 0).sum() > 20
    assert (bits == 0x80000000).sum() == 2 and (bits == 0).sum() == 2
    with np.errstate(invalid="ignore"):
        assert not np.isnan(p).any() and (p >= t).all() and len(cand) == int((prob[0] >= t).sum())
    assert np.isposinf(p).sum() == 3 and (p == t).sum() >= 3 and (p == np.nextafter(t, F(-np.inf))).sum() == 0
    if thr <= 0.0:
        assert (p == 0).sum() == 4 and kept[p == 0].all()
        zeros = np.nonzero(p == 0)[0]
        m = _iou(tlbr[zeros], tlbr)
        m[np.arange(len(zeros)), zeros] = 0
        assert np.nan_to_num(m).max() == 0                           # the tied zeros touch nothing
    if thr < 0.0:
        assert (p < 0).sum() > 50
    assert 0 < kept.sum() < len(cand)


def test_tie_cases_are_ties():
    case = C.tied_isolated()
    want = _oracle(case, C.TIE_PROB_THRESH, C.TIE_IOU)
    cand, tlbr, p, c, kept = _frame(case, want, 0, C.TIE_PROB_THRESH)
    assert kept.all() and 64 < max(np.bincount(c)) and len(cand) < 200
    m = _iou(tlbr, tlbr)
    np.fill_diagonal(m, 0)
    assert m.max() == 0
    assert all(len(np.unique(p[c == k])) <= 5 for k in np.unique(c))
    box, prob, cls, hw = C.tied_overlapping()
    cand = np.nonzero(prob[0] >= F(C.TIE_PROB_THRESH))[0]
    tlbr, p, c = C.scaled_tlbr(box[0, cand], hw[0]), prob[0, cand], cls[0, cand]
    m = (_iou(tlbr, tlbr) > C.TIE_IOU) & (p[:, None] == p[None, :]) & (c[:, None] == c[None, :])
    np.fill_diagonal(m, False)
    assert m.sum() > 100 and max(np.bincount(c)) > 64
