"""The planted inputs of the default soft-max decode (tests/yolo_decode_cases.py), proved on the references alone: no GPU.

Every box is a clear maximum or an exact tie; every tie placement relative to the four-lane split occurs; every saturation and
range value sits in every case; the oracle's float32 ``yolo_decode`` agrees with the float64 restatement within a tenth of the
tolerance the kernels get (so nine tenths of that budget are the kernels'); the extremes reach what they are planted for."""
import numpy as np
import pytest
import torch

import darknet_scores_restate as S
import yolo_decode_cases as Y
import yolov4_restate as V4
from oracle import darknet_oracle as orc

F = np.float32
# reference against reference: one tenth of the kernels' bounds (tests/test_gpu_yolo_decode.py)
SCORE_RTOL, SCORE_ATOL = 1e-6, 1e-8
BOX_RTOL, BOX_ATOL = 1e-6, 1e-7


def _flat(c):
    return c["t"].reshape(-1, c["t"].shape[-1])


def _oracle(t, anchors, net, sxy):
    """the oracle's float32 decode plus Darknet.forward's w, h / net division; with a scale_x_y, the oracle's decode as
    tests/yolov4_restate.py extends it (bit-equal to the oracle's at 1)"""
    b, h, w, a, n = t.shape
    x = torch.from_numpy(np.ascontiguousarray(np.transpose(t, (0, 3, 4, 1, 2))).reshape(b, a * n, h, w))
    box, prob, idx = orc.yolo_decode(x, list(anchors))
    if sxy != 1.0:
        box4, prob4, idx4 = V4.yolo_decode(x, list(anchors), sxy)
        assert torch.equal(prob4, prob) and torch.equal(idx4, idx) and torch.equal(box4[..., 2:], box[..., 2:])
        box = box4
    box = box.clone()
    box[..., 2] /= net[0]
    box[..., 3] /= net[1]
    return box.numpy(), prob.numpy(), idx.numpy()


def _excess(got, want, atol):
    """the largest (|got - want| - atol) / |want| over the finite, non-zero ``want``: within rtol exactly when allclose holds there"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = np.isfinite(want) & (want != 0)
    return float(((np.abs(got[ok] - want[ok]) - atol) / np.abs(want[ok])).max()) if ok.any() else 0.0


def _agree(t, anchors, grid, net, sxy, label):
    box, prob, idx = _oracle(np.asarray(t), anchors, net, sxy)
    wbox, wprob, wcls = Y.softmax_decode64(t, anchors, grid, net, sxy)
    print("%s: oracle against float64: score excess %.3g (rtol %g), box excess %.3g (rtol %g), %d exact ties, %d inf sizes" % (
        label, _excess(prob, wprob, SCORE_ATOL), SCORE_RTOL, _excess(box, wbox, BOX_ATOL), BOX_RTOL,
        int(Y.classify(t)[1].sum()), int(np.isinf(wbox).sum())))
    assert np.array_equal(idx, wcls), "%s: arg-max" % label
    np.testing.assert_allclose(prob, wprob, rtol=SCORE_RTOL, atol=SCORE_ATOL, err_msg=label)
    assert np.array_equal(np.isinf(box), np.isinf(wbox)) and not np.isnan(box).any() and not np.isnan(wbox).any()
    np.testing.assert_allclose(box, wbox, rtol=BOX_RTOL, atol=BOX_ATOL, err_msg=label)      # (inf equals inf of the same sign)


# ---- the table ------------------------------------------------------------------------------------------------------------------
def test_table_covers_the_shapes():
    cases = [Y.case(n) for n in Y.CASE_NAMES]
    assert {c["t"].shape[-1] - 5 for c in cases} >= {1, 2, 3, 4, 5, 7, 80, 81, 122}
    assert {len(c["anchors"]) for c in cases} == {1, 2, 3, 8}
    for c in cases:
        b, h, w, a, n = c["t"].shape
        assert c["t"].dtype == F and (h, w) in Y.GRIDS and b in (2, 3) and (b * h * w) % 32 != 0
        assert c["rows_total"] >= c["row_offset"] + a * h * w and len(c["recipe"]) == b * h * w * a >= 81
    mid = [c for c in cases if c["row_offset"] > 0]
    assert len(mid) == 2 and all(c["rows_total"] > c["row_offset"] + len(c["anchors"]) * c["grid"][0] * c["grid"][1] for c in mid)
    assert sorted(c["sxy"] for c in cases if c["sxy"] != 1.0) == [1.2, 2.0]
    # the class counts below 4 leave lanes empty: three, two and one of them
    assert [sum(len(Y.lane_range(k, n)) == 0 for k in range(4)) for n in (1, 2, 3, 4)] == [3, 2, 1, 0]


@pytest.mark.parametrize("name", Y.CASE_NAMES)
def test_no_ambiguous_box(name):
    c = Y.case(name)
    clear, tie = Y.classify(c["t"])
    assert int((~clear & ~tie).sum()) == 0, "a box that is neither a clear maximum nor an exact tie"
    assert int((clear & tie).sum()) == 0
    z = c["t"][..., 5:]
    assert not np.isnan(c["t"]).any() and not (z == np.inf).any() and np.isfinite(z.max(-1)).all()
    # what the recipe column says is what the logits are
    named_tie = np.isin(c["recipe"], Y.TIE_RECIPES).reshape(tie.shape)
    assert np.array_equal(named_tie, tie)
    if z.shape[-1] >= 2:
        assert int(tie.sum()) >= 3
    # a tie is won by its lowest class, in float64 as in the oracle
    _, _, wcls = Y.want(c)
    flat_cls = np.moveaxis(wcls.reshape(z.shape[0], z.shape[3], z.shape[1], z.shape[2]), 1, 3)
    first = np.argmax(z == z.max(-1, keepdims=True), axis=-1)
    assert np.array_equal(flat_cls, first)


def test_every_tie_placement_occurs():
    found = {n: Y.tie_placements(Y.case(n)["t"]) for n in Y.CASE_NAMES}
    for n, f in found.items():
        print("%-11s %s" % (n, sorted(f)))
    assert set().union(*found.values()) == Y.ALL_PLACEMENTS
    # ... in the 80-class register path (whose lanes are all full), and in the generic class loop
    coco = set().union(*(f for n, f in found.items() if Y.CASE_TABLE[n][3] == 80))
    assert coco == Y.ALL_PLACEMENTS - {"ragged last"}
    for ncls in (81, 122, 27, 7):
        assert set().union(*(f for n, f in found.items() if Y.CASE_TABLE[n][3] == ncls)) == Y.ALL_PLACEMENTS, ncls
    # the small class counts: what their lanes allow
    by = {Y.CASE_TABLE[n][3]: f for n, f in found.items()}
    assert by[1] == set() and by[2] == {"boundary 0", "lanes 0 1", "all equal"}
    assert by[3] >= {"boundary 0", "boundary 1", "lanes 0 1", "lanes 0 2", "lanes 1 2", "all equal"}
    assert by[4] >= {"boundary 2", "lanes 2 3", "lanes 0 3", "three way", "all equal"}
    assert by[5] >= {"same lane", "ragged last"}


@pytest.mark.parametrize("name", Y.CASE_NAMES)
def test_saturation_and_range_in_every_case(name):
    c = Y.case(name)
    flat = _flat(c)
    ncls = flat.shape[1] - 5
    for col, values in ((0, Y.XY_EXTREMES), (1, Y.XY_EXTREMES), (2, Y.WH_EXTREMES), (3, Y.WH_EXTREMES), (4, Y.OBJ_EXTREMES)):
        for v in values:
            assert bool((flat[:, col] == F(v)).any()), "attribute %d never holds %g" % (col, v)
        assert bool((np.abs(flat[:, col]) <= 4.0).sum() >= len(flat) // 2), "attribute %d: ordinary values are the majority" % col
    z = flat[:, 5:]
    for v in Y.WINNERS:
        rows = np.nonzero(c["recipe"] == "winner_%d" % v)[0]
        assert len(rows) and bool((z[rows].max(1) == F(v)).all())
        if ncls > 1:
            assert bool((np.sort(z[rows], 1)[:, -2] <= 4.0).all()), "the rest is ordinary"
    assert len(c["shift_triples"]) >= 2
    for base, plus, minus in c["shift_triples"]:
        assert list(c["recipe"][[base, plus, minus]]) == ["shift_base", "shift_plus", "shift_minus"]
        assert float(z[plus].min()) > 490 and float(z[minus].max()) < -490 and flat[base, 4] == flat[plus, 4] == flat[minus, 4]
    gone = np.isneginf(z)
    assert not gone.all(1).any()
    if ncls >= 2:
        assert int(gone.any(1).sum()) >= 4
        # a whole lane of -inf, the first lane and the last
        per = Y.lane_per(ncls)
        last = Y.lane_range((ncls - 1) // per, ncls)
        assert bool(gone[:, :per].all(1).any()) and bool(gone[:, list(last)].all(1).any())
    else:
        assert not gone.any()
    # boxes whose score is the point keep an objectness that leaves it alone
    assert bool((flat[np.isin(c["recipe"], Y.SCORE_RECIPES), 4] > -4.5).all())


# ---- reference against reference -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Y.CASE_NAMES)
def test_oracle_agrees_with_the_float64_restatement(name):
    c = Y.case(name)
    _agree(c["t"], c["anchors"], c["grid"], c["net"], c["sxy"], name)


@pytest.mark.parametrize("classes", S.DECODE_CLASSES)
@pytest.mark.parametrize("grid", S.DECODE_GRIDS)
def test_oracle_agrees_on_the_darknet_scores_inputs(grid, classes):
    """the inputs of tests/test_gpu_darknet_scores.py's decode test, whose flag-less result tests/test_gpu_yolo_decode.py pins"""
    t = S.decode_case(grid, classes)
    clear, tie = Y.classify(t)
    assert int((~clear & ~tie).sum()) == 0
    _agree(t, S_ANCHORS, grid, (32.0 * grid[1], 32.0 * grid[0]), 1.0, "darknet_scores %s x %d" % (grid, classes))


S_ANCHORS = ((10.0, 14.0), (23.0, 27.0), (37.0, 58.0))          # tests/yolo_op_util.py's default


def test_extremes_reach_their_targets():
    for name in Y.CASE_NAMES:
        c = Y.case(name)
        b, h, w, a, n = c["t"].shape
        box, prob, idx = _oracle(np.asarray(c["t"]), c["anchors"], c["net"], c["sxy"])
        wbox, wprob, wcls = Y.want(c)
        rows = lambda v: np.ascontiguousarray(np.moveaxis(v, 3, 1)).reshape(b, a * h * w)
        t2, t3, t4 = rows(c["t"][..., 2]), rows(c["t"][..., 3]), rows(c["t"][..., 4])
        # exp(90) is inf in float32, in the oracle and in the restatement alike; exp(88) * anchor is finite only for an anchor side of 1 or 2
        for col, tk in ((2, t2), (3, t3)):
            assert bool(np.isposinf(box[..., col][(tk == 90) | (tk == np.inf)]).all())
            assert bool(np.isposinf(wbox[..., col][(tk == 90) | (tk == np.inf)]).all())
            side = np.asarray([p[col - 2] for p in c["anchors"]])
            small = np.broadcast_to((side <= 2)[None, :, None], (b, a, h * w)).reshape(b, -1)
            at88 = tk == 88
            assert at88.any()
            assert bool(np.isfinite(box[..., col][at88 & small]).all() and np.isposinf(box[..., col][at88 & ~small]).all())
            assert bool((box[..., col][at88 & small] > 1e35).all())
            assert bool((box[..., col][np.isneginf(tk)] == 0).all())
        # an objectness of -90 (and -inf) gives a score of exactly 0 in float32; +90 and +inf the class probability itself
        assert bool((prob[(t4 == -90) | np.isneginf(t4)] == 0).all()) and bool((t4 == -90).any())
        # the +-500 shift leaves the float64 score where it was
        flat_score = np.moveaxis(wprob.reshape(b, a, h, w), 1, 3).reshape(-1)
        flat_cls = np.moveaxis(wcls.reshape(b, a, h, w), 1, 3).reshape(-1)
        for base, plus, minus in c["shift_triples"]:
            assert abs(flat_score[plus] - flat_score[base]) <= 1e-12 and abs(flat_score[minus] - flat_score[base]) <= 1e-12
            assert flat_cls[base] == flat_cls[plus] == flat_cls[minus]
            assert flat_score[base] > 1e-3
        # a winner at 1000: probability 1, no overflowing exponential
        flat = _flat(c)
        for k in np.nonzero(c["recipe"] == "winner_1000")[0]:
            assert abs(flat_score[k] - Y.sigmoid64(flat[k, 4])) <= 1e-15
    # a finite exp(88) * anchor is looked at in at least one case per column
    seen = {2: False, 3: False}
    for name in Y.CASE_NAMES:
        c = Y.case(name)
        for col in (2, 3):
            for k, p in enumerate(c["anchors"]):
                seen[col] |= p[col - 2] <= 2 and bool((c["t"][:, :, :, k, col] == 88).any())
    assert seen[2] and seen[3]


# ---- the planted detection heads -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n_sets", [("c80_a3_mid", 8), ("c27_a8", 3), ("c5_a8", 3)])
def test_head_biases_walk_every_recipe(name, n_sets):
    c = Y.case(name)
    sets = Y.head_boxes(name, n_sets)
    na, n_attr = len(c["anchors"]), c["t"].shape[-1]
    assert len(sets) == n_sets and all(len(s) == na for s in sets)
    picked = [k for s in sets for k in s]
    assert len(set(picked)) == len(picked)
    assert set(Y.RECIPES[k % len(Y.RECIPES)] for k in picked) == set(Y.RECIPES)
    t = np.stack([Y.head_bias(name, s).reshape(na, n_attr) for s in sets])
    want = Y.tie_placements(c["t"])
    assert Y.tie_placements(t) == want and len(want) >= 9
    flat = _flat(c)
    for s in sets:
        bias = Y.head_bias(name, s)
        assert bias.dtype == F and bias.shape == (na * n_attr,) and np.array_equal(bias.reshape(na, n_attr), flat[list(s)])
    # the extremes ride along: some set holds an infinite and a +-90 value in the box attributes and in the objectness
    assert np.isinf(t[..., :4]).any() and (np.abs(t[..., :5]) == 90).any() and np.isneginf(t[..., 5:]).any()
