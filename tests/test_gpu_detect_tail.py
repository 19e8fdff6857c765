"""``detect_kernel`` (csrc/detect.hip) at its size limits and on its wide-box path (-m gpu), the default rule, EXACTLY.

The inputs are those of tests/detect_tail_cases.py, which tests/test_detect_tail_host.py proves to reach what they are meant
to reach.  The expected side is the oracle's ``postprocess(..., audit=True)`` / ``non_max_suppression``: both sides receive
the same float32 numbers, scaling is one float32 product with an exactly representable size (-ffp-contract=off), everything
after truncation is integer or float64 -- so every comparison is equality of the kept rows and of box, score bits and class at
every row.  The audit is used for the row indices only: no row is exempt.  Every output is also held to the canonical order of
the kernel's header (class ascending, score descending, higher row first).

Out of scope: class indices outside int32 -- the kernel stores a class as ``int``, so such indices are not supported and not
tested."""
import time

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import _hip

import darknet_nms_restate as D
import detect_tail_cases as C
from detect_util import F, assert_canonical_order, assert_equals_oracle, dev, direct_detect, run_detector, same

pytestmark = pytest.mark.gpu


def _against_oracle(case, prob_thresh, iou):
    """``y3_detect`` on the whole batch in one launch against the oracle, frame by frame; -> the kernel's frames."""
    box, prob, cls, hw = case
    want = orc.postprocess(box, prob, cls, hw, F(prob_thresh), iou, audit=True)
    got = direct_detect(box, prob, cls, hw, prob_thresh, iou)
    assert len(got) == len(want) == len(hw)
    for f in range(len(hw)):
        print("frame %d: %d candidates, kept %d (oracle %d)" % (f, len(want[f][4]), len(got[f][3]), len(want[f][3])))
        assert_equals_oracle(got[f], want[f])
    return got


def _one_frame(case, f):
    box, prob, cls, hw = case
    return box[f:f + 1], prob[f:f + 1], cls[f:f + 1], hw[f:f + 1]


# ---- (a) candidate-count boundaries ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,placement", C.COUNT_LAYOUTS, ids=["%d_%s" % l for l in C.COUNT_LAYOUTS])
def test_candidate_counts_on_every_boundary(rows, placement):
    """16 frames in one launch with 0, 1, 2, 3, 63, 64, 65, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097 and 8193 candidates
    (chunk of 64, gather of 1024, LDS sort up to 4096, compaction pass of 8192 rows) among 8200 rows, and in the last rows /
    across row 8192 of 8192, 8193 and 16385 rows (with 8192 rows the last frame has 8192 candidates: every row).  Each frame
    alone gives what it gives inside the batch."""
    case = C.count_boundaries(rows, placement)
    got = _against_oracle(case, C.COUNT_PROB_THRESH, C.COUNT_IOU)
    for f in range(len(C.COUNTS)):
        same(direct_detect(*_one_frame(case, f), C.COUNT_PROB_THRESH, C.COUNT_IOU), [got[f]])


# ---- (b) class-chunk boundaries ---------------------------------------------------------------------------------------------------
def test_class_sizes_on_the_chunk_boundaries_and_signed_classes():
    """Single classes of 64, 65, 127, 128 and 129 overlapping candidates; 1025 candidates in 1025 classes from INT32_MIN to
    INT32_MAX; six classes of 64 .. 130 candidates with negative, zero and large indices (classes sort as signed numbers).
    Class indices outside int32 are out of scope: the kernel stores classes as ``int``."""
    case = C.class_chunks()
    got = _against_oracle(case, C.CLASS_PROB_THRESH, C.CLASS_IOU)
    many = got[len(C.CLASS_SIZES)]
    assert len(many[2]) == C.MANY_CLASSES and many[2][0] == C.INT32_MIN and many[2][-1] == C.INT32_MAX
    assert (np.diff(many[2]) > 0).all()
    signed = got[len(C.CLASS_SIZES) + 1]
    assert np.unique(signed[2]).tolist() == sorted(C.SIGNED_CLASSES)
    for f in range(len(got)):
        same(direct_detect(*_one_frame(case, f), C.CLASS_PROB_THRESH, C.CLASS_IOU), [got[f]])


# ---- (c) wide coordinates, forward mode ----------------------------------------------------------------------------------------
def test_wide_frame_takes_the_64_bit_path_like_the_oracle():
    """A 20000 x 24000 frame: candidates on both sides of +-16000 in chunks that are narrow, wide and mixed, in every order
    (test_detect_tail_host.py), so suppression switches between the 32-bit test and the int64 / float64 test, against
    earlier chunks and inside a chunk, inside a class.  The same boxes on a 608 x 608 frame, where nothing is wide, are the control."""
    box, prob, cls, hw = C.wide_forward()
    wide = _against_oracle((box, prob, cls, hw), C.WIDE_PROB_THRESH, C.WIDE_IOU)
    assert (np.abs(wide[0][0]) >= C.I32_LIM).any(axis=1).sum() >= 20
    control = _against_oracle((box, prob, cls, [C.WIDE_CONTROL_HW]), C.WIDE_PROB_THRESH, C.WIDE_IOU)
    assert np.abs(control[0][0]).max() < 1000
    # through the public Detector as well: the same detections
    same(run_detector(box, prob, cls, hw, C.WIDE_PROB_THRESH, C.WIDE_IOU), wide)


# ---- (d) wide coordinates, NMS mode -------------------------------------------------------------------------------------------
def _nms(boxes, prob, cls, thr):
    got = yolov3.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=thr)
    assert isinstance(got, list) and len(set(got)) == len(got)
    assert_canonical_order(prob[got], np.zeros(len(got), np.int64) if cls is None else cls[got], got)
    return got


@pytest.mark.parametrize("thr", C.NMS_THRESHOLDS)
def test_nms_translated_across_the_line_keeps_the_same_list(thr):
    """The borderline-ratio boxes (inter / union on the threshold all the time, degenerate boxes included) moved by 0, 15990
    (some boxes cross 16000: chunks of both kinds), 20000, -20000 and 10^9.  A translation changes no intersection and no
    union, so every run returns the IDENTICAL list, and that list is the oracle's keep set: the int64 / float64-division code
    decides every pair as the 32-bit test and as numpy do -- ``>``, not ``>=``, at thresholds 0.5 and 1.0 that pairs sit on.
    Class-agnostic (1500 boxes, 24 chunks of one class) and in four classes of more than 64 boxes."""
    boxes, prob, cls = C.borderline_boxes(thr)
    for k in (None, cls):
        want = sorted(int(i) for i in orc.non_max_suppression(boxes, prob, class_idx=k, iou_thresh=thr))
        home = _nms(boxes, prob, k, thr)
        assert sorted(home) == want
        print("thr %.3f %s: kept %d of %d" % (thr, "agnostic" if k is None else "4 classes", len(home), len(prob)))
        for t in C.TRANSLATIONS[1:]:
            assert _nms(C.translated(boxes, t), prob, k, thr) == home, "translated by %d" % t


@pytest.mark.parametrize("name", ["line", "far"])
def test_nms_corners_on_the_line(name):
    """Boxes whose corners are exactly +-15999, +-16000 and +-16001 (the largest boxes the 32-bit test was sized for, and the
    first it must not see), and with corners at +-40000 and +-10^9 beside them: areas that 32-bit integers cannot hold.
    Class-agnostic and in four signed classes, more than 64 boxes each."""
    boxes, prob, cls = C.corner_boxes(C.LINE_CORNERS if name == "line" else C.FAR_CORNERS)
    for k in (None, cls):
        for thr in (0.3, 0.5):
            want = sorted(int(i) for i in orc.non_max_suppression(boxes, prob, class_idx=k, iou_thresh=thr))
            got = _nms(boxes, prob, k, thr)
            print("%s thr %.1f %s: kept %d of %d" % (name, thr, "agnostic" if k is None else "4 classes", len(got), len(prob)))
            assert sorted(got) == want


# ---- (e) running out of chunk flags -----------------------------------------------------------------------------------------
def test_classes_without_chunk_flags_run_on_one_wave_and_change_nothing():
    """520 classes of 65 candidates and one of 700 ask for 1051 chunk flags where 1024 exist: some classes -- which ones is
    decided by the order of an atomicAdd -- run all their chunks on one wavefront while the others chain across wavefronts.
    Two frames (the long class sorting last / first), three launches: each equals the oracle, so all are identical.  The
    same boxes under Darknet's ``iou`` rule equal the restatement of tests/darknet_nms_restate.py.

    Observed on an MI355X: 0.014 s for the three default-rule launches of 2 x 34616 rows with their host copies (printed), 0.7 s
    for the whole test, most of it the two restatements on the CPU."""
    case = C.flag_exhaustion()
    box, prob, cls, hw = case
    want = orc.postprocess(box, prob, cls, hw, F(C.FLAG_PROB_THRESH), C.FLAG_IOU, audit=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runs = [direct_detect(box, prob, cls, hw, C.FLAG_PROB_THRESH, C.FLAG_IOU) for _ in range(3)]
    print("three launches with their copies: %.3f s" % (time.perf_counter() - t0))
    for got in runs:
        for f in range(2):
            assert_equals_oracle(got[f], want[f])
        same(got, runs[0])
    dk = run_detector(box, prob, cls, hw, C.FLAG_PROB_THRESH, C.FLAG_DK_THRESH, nms_kind="iou")
    for f in range(2):
        rows = D.detect_keep_rows(box[f], prob[f], cls[f], C.FLAG_PROB_THRESH, C.FLAG_DK_THRESH, "iou")
        assert dk[f][3].tolist() == rows and len(rows) > 1024


# ---- (f) scores that are not ordinary probabilities ------------------------------------------------------------------------
@pytest.mark.parametrize("thr", C.SCORE_THRESHOLDS)
def test_scores_nan_zeros_subnormals_negatives_and_inf(thr):
    """``class_prob`` with NaN (never a candidate: it fails ``>=``), -inf, +inf, -0.0 and +0.0 (both pass a threshold of 0.0),
    subnormals of both signs, negative scores (candidates at threshold -1.0) and the threshold's two neighbours: the candidate
    set and every detection equal the oracle's, and the sort key built from the bit pattern orders them as numbers."""
    case = C.score_edges(thr)
    got = _against_oracle(case, thr, C.SCORE_IOU)
    kept = got[0][1]
    assert np.isposinf(kept).any() and not np.isnan(kept).any() and (kept >= F(thr)).all()
    if thr <= 0.0:
        assert sorted(kept[kept == 0].view(np.uint32).tolist()) == [0, 0, 0x80000000, 0x80000000]
    same(run_detector(*case, thr, C.SCORE_IOU), got)


def test_tied_scores():
    """Exact ties among boxes that overlap nothing: the oracle's detections, as sets.  Exact ties among overlapping boxes:
    the survivor is the implementation's choice (the reference's depends on ``argsort``), so three runs agree with each other
    and obey the canonical order -- among equal scores the higher row first."""
    _against_oracle(C.tied_isolated(), C.TIE_PROB_THRESH, C.TIE_IOU)
    box, prob, cls, hw = C.tied_overlapping()
    runs = [direct_detect(box, prob, cls, hw, C.TIE_PROB_THRESH, C.TIE_IOU) for _ in range(3)]
    for got in runs:
        same(got, runs[0])
    tlbr, p, c, rows = runs[0][0]
    assert_canonical_order(p, c, rows)
    n_cand = int((prob[0] >= F(C.TIE_PROB_THRESH)).sum())
    assert 20 < len(rows) < n_cand and (p >= F(C.TIE_PROB_THRESH)).all()
    assert np.array_equal(p.view(np.uint32), prob[0, rows].view(np.uint32)) and np.array_equal(c, cls[0, rows])
    assert np.array_equal(tlbr, C.scaled_tlbr(box[0, rows], hw[0]))
    # greedy with ANY order of the ties: no two survivors of a class exceed the threshold, every candidate that went has a
    # survivor of its class with at least its score that does
    cand = np.nonzero(prob[0] >= F(C.TIE_PROB_THRESH))[0]
    ct = C.scaled_tlbr(box[0, cand], hw[0])

    def iou(a, b):
        iw = np.maximum(0, np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]) + 1)
        ih = np.maximum(0, np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]) + 1)
        area = lambda t: (t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1)
        return iw * ih / (area(a)[:, None] + area(b)[None, :] - iw * ih)
    hit = (iou(ct, tlbr) > C.TIE_IOU) & (cls[0, cand][:, None] == c[None, :])
    among = hit[np.isin(cand, rows)]
    assert among.sum() == len(rows)                                  # a survivor meets itself only
    gone = ~np.isin(cand, rows)
    assert (hit[gone] & (p[None, :] >= prob[0, cand][gone][:, None])).any(axis=1).all()


# ---- (g) pack_records -------------------------------------------------------------------------------------------------------------
def test_pack_records_values():
    """``y3_pack_records`` (no other test asserts its values): counts of 0, below, equal to and above ``kmax``; corners beyond
    +-2^31 saturate; a valid record carries the frame's true count; padding records are all zero."""
    lib = _hip.lib()
    rng = np.random.default_rng(71)
    batch, rows, kmax = 5, 12, 4
    count = np.array([0, 2, 4, 9, 12], np.int32)
    tlbr = rng.integers(-3000, 3000, size=(batch, rows, 4)).astype(np.int64)
    tlbr[1, 0] = [2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1]
    tlbr[2, 3] = [2 ** 40, -2 ** 40, 2 ** 62, -2 ** 62]
    tlbr[3, 1] = [np.iinfo(np.int64).max, np.iinfo(np.int64).min, 0, -1]
    prob = rng.uniform(-1, 1, size=(batch, rows)).astype(F)
    prob[1, 1], prob[2, 0] = F(np.inf), F(-0.0)
    cls = rng.integers(-2 ** 31, 2 ** 31, size=(batch, rows)).astype(np.int64)
    row = rng.integers(0, 2 ** 31 - 1, size=(batch, rows)).astype(np.int32)
    d = dev()
    T = lambda a: torch.from_numpy(a).to(d)
    bufs = [T(count), T(tlbr), T(prob), T(cls), T(row)]
    rec = torch.full((batch, kmax, 8), -1, dtype=torch.int32, device=d)
    rec_count = torch.full((batch,), -1, dtype=torch.int32, device=d)
    _hip.check(lib.y3_pack_records(*[b.data_ptr() for b in bufs], batch, rows, kmax, rec.data_ptr(), rec_count.data_ptr(),
                                   _hip.stream_ptr()))
    want = np.concatenate([np.clip(tlbr, -2 ** 31, 2 ** 31 - 1).astype(np.int32), prob.view(np.int32)[..., None],
                           cls.astype(np.int32)[..., None], row[..., None], np.broadcast_to(count[:, None, None], (batch, rows, 1))],
                          axis=2)[:, :kmax]
    want = np.where(np.arange(kmax)[None, :, None] < count[:, None, None], want, 0).astype(np.int32)
    assert np.array_equal(rec.cpu().numpy(), want)
    assert rec_count.cpu().numpy().tolist() == count.tolist()
    assert (want[1, 0, :4] == [2 ** 31 - 1, 2 ** 31 - 1, -2 ** 31, -2 ** 31]).all() and (want[0] == 0).all()
