"""Darknet class scores on every decode path, ``y3_expand_labels``, and multi-label detection end to end (-m gpu).

Decode: one-op Y3_OP_YOLO plans through ``y3_op_run`` on planted logits (tests/darknet_scores_restate.py: +-20, +-90, planted
ties) in the sequential float32 form and the four-lane form, and a head conv + YOLO pair at fuse_head 0 / 1 / 2 / 3 / 4 in bf16
and fp16.  Labels: the entry point against the restatement on two strided heads, capacity, padding, NaN, a one-row head and
its memory footprint.  End to end: tests/golden/cfg/mini.cfg with planted heads through ``inference()`` and
``detect_in_frames()``."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.preprocess import correct_letterbox_boxes
from yolov3.synthdata import synth_frames

import darknet_nms_restate as D
import darknet_scores_restate as S
import footprint_util as fu
from golden_util import GOLDEN, ROOT
from yolo_op_util import yolo_op as _yolo_op
from oracle import darknet_oracle as orc

pytestmark = pytest.mark.gpu

F = np.float32
SCORE_RTOL, SCORE_ATOL = 5e-4, 2e-5            # tests/test_gpu_yolov4.py's bounds for decoded scores
MINI = os.path.join(GOLDEN, "cfg", "mini.cfg")


def _conv(f, k, s=1, act="mish", bn=True):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % (
        "batch_normalize=1\n" if bn else "", f, k, s, act)


def _write(tmp_path, text, name):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _run(net, frames, f32_input):
    out = net.forward(torch.from_numpy(orc.frames_to_input(list(frames)))) if f32_input else net.forward_frames(frames)
    torch.cuda.synchronize()
    return out


# ---- the decode with the flag: one-op plans -----------------------------------------------------------------------------------------
# (tests/yolo_op_util.py: shared with tests/test_gpu_yolo_decode.py)


_WANT = {}


def _decode_want(grid, classes):
    key = (grid, classes)
    if key not in _WANT:
        t = S.decode_case(grid, classes)
        prob, cls = S.decode_scores(S.head_rows(t, 0)[0])
        _WANT[key] = (t, prob, cls)
    return _WANT[key]


@pytest.mark.parametrize("classes", S.DECODE_CLASSES)
@pytest.mark.parametrize("grid", S.DECODE_GRIDS)
def test_decode_with_the_flag_matches_the_restatement(grid, classes):
    t, want_prob, want_cls = _decode_want(grid, classes)
    outs = {}
    for name, dtype in (("sequential", _hip.Y3_F32), ("four lanes", _hip.Y3_BF16)):
        rc, box0, prob0, cls0 = _yolo_op(t, dtype, 0)
        assert rc == 0
        rc, box, prob, cls = _yolo_op(t, dtype, _hip.F_SCORES_DARKNET)
        assert rc == 0, _hip.lib().y3_last_error()
        d = np.abs(prob.astype(np.float64) - want_prob) - SCORE_RTOL * np.abs(want_prob)
        print("%s grid %s classes %d: max |dscore| - rtol * |score| = %.3g (atol %g)" % (name, grid, classes, d.max(), SCORE_ATOL))
        assert box.tobytes() == box0.tobytes(), "%s: the flag changed the boxes" % name
        np.testing.assert_allclose(prob, want_prob, rtol=SCORE_RTOL, atol=SCORE_ATOL, err_msg=name)
        assert np.array_equal(cls, want_cls), name
        if classes > 1:
            assert not np.array_equal(prob, prob0), "%s: the flag is ignored" % name
        outs[name] = prob
    # the four-lane form against the sequential one: test_split_class_decode_matches_sequential_decode's bound
    np.testing.assert_allclose(outs["four lanes"], outs["sequential"], rtol=2e-6, atol=1e-9)


def test_flag_changes_nothing_on_a_new_coords_op():
    t = S.logistic(S.decode_case((5, 7), 80))                      # probabilities, as a logistic head conv stores them
    for dtype in (_hip.Y3_F32, _hip.Y3_BF16):
        a = _yolo_op(t, dtype, _hip.F_NEW_COORDS)
        b = _yolo_op(t, dtype, _hip.F_NEW_COORDS | _hip.F_SCORES_DARKNET)
        assert a[0] == b[0] == 0
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[1:], b[1:]))


# ---- head conv + YOLO pair at every fuse_head -------------------------------------------------------------------------------------
def _pair_cfg(h, w, classes):
    return ("[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (8 * w, 8 * h) + _conv(32, 3, 2) + _conv(64, 3, 2) + _conv(128, 3, 2) +
            _conv(256, 1) + _conv(3 * (5 + classes), 1, act="linear", bn=False) +
            "[yolo]\nmask=0,1,2\nanchors=10,14, 23,27, 37,58\nclasses=%d\nnum=3\n" % classes)


PAIR_HEAD = 4


def _pair_params(cfg):
    blocks, net_info = parse_config(cfg)
    calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
    return W.synth_params(blocks, net_info, seed=5, obj_bias=-1.0, calib=calib)


def _bits(out):
    return tuple(out[k].cpu().numpy().tobytes() for k in ("bbox_xywh", "class_prob", "class_idx"))


@pytest.mark.parametrize("grid,classes", [((5, 7), 80), ((13, 13), 81), ((13, 13), 3), ((5, 7), 1)])
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_head_pair_every_fuse_head(tmp_path, dtype, grid, classes):
    cfg = _write(tmp_path, _pair_cfg(grid[0], grid[1], classes), "pair.cfg")
    params = _pair_params(cfg)
    frames = synth_frames(17, 3, 8 * grid[0], 8 * grid[1])
    heads = (0,) if dtype == "float32" else (0, 1, 2, 3, 4)
    outs, names = {}, {}
    for fh in heads:
        net = yolov3.Darknet(cfg, device="cuda", dtype=dtype, keep_all=fh == 0, fuse=True, options={"fuse_head": fh},
                             scores="darknet").set_params(params).eval()
        outs[fh] = _run(net, frames, dtype == "float32")
        report = net.plan_report()
        names[fh] = report[-2]["kernel"]
        assert report[-1]["scores"] == "darknet"
        if fh == 0:
            logits = net.block_output(PAIR_HEAD).cpu().numpy()         # (B, C, h, w): the head conv's own float32 output
        del net
    for fh in heads[1:]:
        assert _bits(outs[fh]) == _bits(outs[0]), "%s fuse_head %d (%s) differs from the two-launch path" % (dtype, fh, names[fh])
    if dtype != "float32" and classes == 80:                       # (255 channels: the fused head kernels take up to 256)
        assert all("head_decode" in names[fh] for fh in (1, 2, 3, 4)), names
    plain = yolov3.Darknet(cfg, device="cuda", dtype=dtype, keep_all=True, fuse=True, options={"fuse_head": 0}).set_params(params)
    ref = _run(plain, frames, dtype == "float32")
    assert plain.plan_report()[-1]["scores"] == "reference"
    assert ref["bbox_xywh"].cpu().numpy().tobytes() == outs[0]["bbox_xywh"].cpu().numpy().tobytes()
    b, c, h, w = logits.shape
    t = logits.reshape(b, 3, c // 3, h, w).transpose(0, 3, 4, 1, 2)
    want_prob, want_cls = S.decode_scores(S.head_rows(np.ascontiguousarray(t), 0)[0])
    got_prob, got_cls = outs[0]["class_prob"].cpu().numpy(), outs[0]["class_idx"].cpu().numpy()
    np.testing.assert_allclose(got_prob, want_prob, rtol=SCORE_RTOL, atol=SCORE_ATOL)
    _, p64 = S.probabilities64(S.head_rows(np.ascontiguousarray(t), 0)[0])
    if classes > 1:
        top = np.sort(p64, -1)[..., -2:]
        clear = (top[..., 1] - top[..., 0]) > S.MARGIN                 # (conv outputs are not planted: compare where no last bit decides)
        assert clear.any() and np.array_equal(got_cls[clear], want_cls[clear])
        assert not np.array_equal(got_prob, ref["class_prob"].cpu().numpy())


# ---- y3_expand_labels ---------------------------------------------------------------------------------------------------------------
def _expand(heads, bbox, thresh, cap, pad=3):
    """heads: restatement dicts; every head lives in a buffer of pixel stride ld > A * n_attr whose other channels are NaN"""
    lib = _hip.lib()
    batch, rows_total = bbox.shape[:2]
    keep, views = [], (_hip.Y3HeadView * len(heads))()
    for v, hd in zip(views, heads):
        b, h, w, a, n = hd["t"].shape
        ld = a * n + pad
        x = torch.full((b, h, w, ld), float("nan"), dtype=torch.float32)
        x[..., :a * n] = torch.from_numpy(hd["t"].reshape(b, h, w, a * n))
        x = x.cuda()
        keep.append(x)
        v.d_head, v.h, v.w, v.ld, v.n_anchor, v.n_attr = x.data_ptr(), h, w, ld, a, n
        v.row_offset, v.new_coords = hd["row_offset"], int(bool(hd.get("new_coords")))
    d_bbox = torch.from_numpy(bbox).cuda()
    nws = lib.y3_expand_labels_workspace_bytes(batch, rows_total, cap)
    ws = torch.full((nws,), 0xFF, dtype=torch.uint8, device="cuda")
    vbbox = torch.full((batch, cap, 4), float("nan"), dtype=torch.float32, device="cuda")
    vprob = torch.full((batch, cap), float("nan"), dtype=torch.float32, device="cuda")
    vcls = torch.full((batch, cap), -7, dtype=torch.int64, device="cuda")
    vrow = torch.full((batch, cap), -7, dtype=torch.int32, device="cuda")
    vcount = torch.full((batch,), -7, dtype=torch.int32, device="cuda")
    _hip.check(lib.y3_expand_labels(views, len(heads), d_bbox.data_ptr(), batch, rows_total, ctypes.c_float(thresh), cap,
                                    ws.data_ptr(), nws, vbbox.data_ptr(), vprob.data_ptr(), vcls.data_ptr(), vrow.data_ptr(),
                                    vcount.data_ptr(), _hip.stream_ptr()))
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in (vbbox, vprob, vcls, vrow, vcount))


def _check_labels(heads, bbox, thresh, cap, got):
    vbbox, vprob, vcls, vrow, vcount = got
    want = S.labels(heads, thresh)
    for f, (rows, cls, score) in enumerate(want):
        assert vcount[f] == len(rows), "frame %d: true count" % f
        n = min(len(rows), cap)
        assert np.array_equal(vrow[f, :n], rows[:n]) and np.array_equal(vcls[f, :n], cls[:n]), "frame %d" % f
        np.testing.assert_allclose(vprob[f, :n], score[:n], rtol=SCORE_RTOL, atol=SCORE_ATOL)
        assert vbbox[f, :n].tobytes() == bbox[f, rows[:n]].tobytes()
        assert bool((vprob[f, n:] == -1).all() and (vcls[f, n:] == 0).all() and (vrow[f, n:] == -1).all())
        assert vbbox[f, n:].tobytes() == bytes(16 * (cap - n))
    return [len(w[0]) for w in want]


def _label_bbox(batch, rows_total, seed=3):
    box = np.random.default_rng(seed).uniform(0.0, 1.0, size=(batch, rows_total, 4)).astype(F)
    if rows_total > 5:
        box[0, 5] = [np.nan, -0.0, np.inf, 1e-42]                      # copied bit for bit, whatever the bits
    return box


@pytest.mark.parametrize("thresh", S.THRESHOLDS)
def test_expand_labels_equals_the_restatement(thresh):
    heads, rows_total = S.label_case()
    bbox = _label_bbox(S.LABEL_BATCH, rows_total)
    cap = sum(3 * hd["h"] * hd["w"] * hd["classes"] for hd in S.LABEL_HEADS)      # every (row, class) fits
    counts = _check_labels(heads, bbox, thresh, cap, _expand(heads, bbox, thresh, cap))
    print("thresh %g: labels per frame %s of %d" % (thresh, counts, cap))
    assert min(counts) > 0
    # a capacity below the count: the true count, and the first `cap` labels in (row, c) order
    small = min(counts) // 2 + 1
    _check_labels(heads, bbox, thresh, small, _expand(heads, bbox, thresh, small))
    # heads given in the other order, and a capacity of one
    _check_labels(heads, bbox, thresh, 1, _expand(heads[::-1], bbox, thresh, 1))


def test_best_label_of_a_row_is_the_decodes_score_bit_for_bit():
    """Each head of the label inputs through a one-op float32 Y3_OP_YOLO with the flag, then through y3_expand_labels: the
    best label of every row carries the decode's score, bit for bit, and its class (hundreds of distinct scores per head)."""
    heads, _ = S.label_case()
    for hd in heads:
        rc, box, prob, cls = _yolo_op(hd["t"], _hip.Y3_F32, _hip.F_SCORES_DARKNET)
        assert rc == 0
        rows = prob.shape[1]
        cap = rows * (hd["t"].shape[-1] - 5)
        alone = [dict(t=hd["t"], row_offset=0, new_coords=False)]
        vbbox, vprob, vcls, vrow, vcount = _expand(alone, box, 0.0, cap)
        for f in range(prob.shape[0]):
            n = int(vcount[f])
            assert n == cap                                              # at threshold 0 every (row, class) is a label
            assert vbbox[f, :n].tobytes() == box[f, vrow[f, :n]].tobytes()
            best = np.full(rows, -1.0, F)
            np.maximum.at(best, vrow[f, :n], vprob[f, :n])
            assert best.tobytes() == prob[f].tobytes()
            first = {}
            for r, c, s in zip(vrow[f, :n].tolist(), vcls[f, :n].tolist(), vprob[f, :n]):
                if s == best[r] and r not in first:
                    first[r] = c
            assert [first[r] for r in range(rows)] == cls[f].tolist()
        assert len(np.unique(prob)) > 100


def test_expand_labels_one_row_one_class_nan_and_new_coords():
    t = np.zeros((2, 1, 1, 1, 6), F)
    t[0, ..., 4], t[0, ..., 5] = 2.0, 1.0
    t[1, ..., 4], t[1, ..., 5] = 2.0, -3.0
    heads = [dict(t=t, row_offset=0, new_coords=False)]
    bbox = _label_bbox(2, 1)
    got = _expand(heads, bbox, 0.25, 4)
    assert _check_labels(heads, bbox, 0.25, 4, got) == [1, 0]
    # a NaN objectness, a NaN class value: no label from them, nothing else disturbed
    heads, rows_total = S.label_case()
    bbox = _label_bbox(S.LABEL_BATCH, rows_total)
    base = S.labels(heads, 0.001)
    heads[0]["t"][0, 1, 2, 1, 4] = np.nan
    heads[1]["t"][1, 3, 5, 2, 5 + 17] = np.nan
    row_a = heads[0]["row_offset"] + 1 * 4 * 6 + 1 * 6 + 2
    row_b = heads[1]["row_offset"] + 2 * 8 * 12 + 3 * 12 + 5
    cap = 40000
    got = _expand(heads, bbox, 0.001, cap)
    counts = _check_labels(heads, bbox, 0.001, cap, got)
    assert row_a not in got[3][0, :counts[0]]
    assert not any(r == row_b and c == 17 for r, c in zip(got[3][1, :counts[1]], got[2][1, :counts[1]]))
    assert counts[0] == len(base[0][0]) - int((base[0][0] == row_a).sum())
    assert counts[1] == len(base[1][0]) - int(((base[1][0] == row_b) & (base[1][1] == 17)).sum())
    # new_coords: the stored values are used as they are
    p = dict(t=S.logistic(heads[1]["t"]), row_offset=0, new_coords=True)
    bb = _label_bbox(S.LABEL_BATCH, 3 * 8 * 12)
    _check_labels([p], bb, 0.25, cap, _expand([p], bb, 0.25, cap))


def test_expand_labels_footprint():
    """poisoned outputs, guards round every buffer, strided head views whose margins are NaN: nothing outside the output bodies
    and the workspace changes, and the outputs equal the restatement's"""
    heads, rows_total = S.label_case()
    bbox = _label_bbox(S.LABEL_BATCH, rows_total)
    # 0.001 with a small capacity: every frame is cut off at it; 0.25 with a large one: padding slots behind the labels
    for thresh, cap, cut in ((0.001, 3000, True), (0.25, 30000, False)):
        counts = _footprint_run(heads, bbox, rows_total, thresh, cap)
        assert (min(counts) > cap) if cut else (0 < max(counts) < cap), counts


def _footprint_run(heads, bbox, rows_total, thresh, cap):
    lib = _hip.lib()
    batch = S.LABEL_BATCH
    nws = int(lib.y3_expand_labels_workspace_bytes(batch, rows_total, cap))
    ops, data = [], {}
    for k, hd in enumerate(heads):
        b, h, w, a, n = hd["t"].shape
        c0, ld = fu.strided_ld(a * n, 1, k)
        ops.append(fu.Operand("head%d" % k, "in", "float32", b * h * w, ld, [(c0, a * n)]))
        data["head%d" % k] = [torch.from_numpy(hd["t"].reshape(b * h * w, a * n))]
    ops.append(fu.flat("bbox", "in", "float32", batch * rows_total * 4))
    data["bbox"] = [torch.from_numpy(bbox).reshape(1, -1)]
    ops += [fu.flat("workspace", "scratch", "u8", nws), fu.flat("vbbox", "out", "float32", batch * cap * 4),
            fu.flat("vprob", "out", "float32", batch * cap), fu.flat("vcls", "out", "i64", batch * cap),
            fu.flat("vrow", "out", "i32", batch * cap), fu.flat("vcount", "out", "i32", batch)]
    lay = fu.Layout(ops)
    raw = torch.empty(lay.total + fu.ALIGN, dtype=torch.uint8, device="cuda")
    shift = -raw.data_ptr() % fu.ALIGN
    alloc = raw[shift:shift + lay.total]
    base = alloc.data_ptr()
    fu.fill(alloc, lay, data, poisoned=True)
    torch.cuda.synchronize()
    before = alloc.clone()
    views = (_hip.Y3HeadView * len(heads))()
    for k, (v, hd) in enumerate(zip(views, heads)):
        b, h, w, a, n = hd["t"].shape
        v.d_head, v.h, v.w, v.ld, v.n_anchor, v.n_attr = lay["head%d" % k].ptr(base), h, w, lay["head%d" % k].ld, a, n
        v.row_offset, v.new_coords = hd["row_offset"], 0
    p = {o.name: o.ptr(base) for o in ops}
    import kernel_census as census
    del census.LAUNCHED[:]
    census.logged(lambda: _hip.check(lib.y3_expand_labels(views, len(heads), p["bbox"], batch, rows_total, ctypes.c_float(thresh), cap,
                                                       p["workspace"], nws, p["vbbox"], p["vprob"], p["vcls"], p["vrow"], p["vcount"],
                                                       _hip.stream_ptr())))
    torch.cuda.synchronize()
    census.assert_census("y3_expand_labels")
    msg = fu.footprint_violations(before, alloc, lay)
    assert msg is None, msg
    out = {name: fu.read_slice(alloc, lay[name], 0, dt).cpu().numpy()
           for name, dt in (("vbbox", torch.float32), ("vprob", torch.float32), ("vcls", torch.int64), ("vrow", torch.int32),
                            ("vcount", torch.int32))}
    got = (out["vbbox"].reshape(batch, cap, 4), out["vprob"].reshape(batch, cap), out["vcls"].reshape(batch, cap),
           out["vrow"].reshape(batch, cap), out["vcount"].reshape(batch))
    return _check_labels(heads, bbox, thresh, cap, got)


# ---- end to end on mini.cfg with planted heads --------------------------------------------------------------------------------------
def _mini_params():
    blocks, net_info = parse_config(MINI)
    params = W.synth_params(blocks, net_info, seed=2, obj_bias=-4.0)
    head = 0
    convs = [b for b in blocks if b["type"] == "convolutional"]
    for p, blk in zip(params, convs):
        if not blk.get("batch_normalize") and blk["filters"] == 255:
            p["weight"] = np.zeros_like(p["weight"])
            p["bias"] = S.e2e_head_bias(head).astype(np.float32)
            head += 1
    assert head == 2
    return params


def _mini(dtype="float32", **kw):
    return yolov3.Darknet(MINI, device="cuda", dtype=dtype, **kw).set_params(_mini_params()).eval()


E2E_SHAPES = [(32, 48), (64, 96), (90, 60), (32, 48)]


def _mini_frames(shapes):
    return [synth_frames(50 + k, 1, h, w)[0] for k, (h, w) in enumerate(shapes)]


_E2E = {}


def _e2e_reference():
    """the planted labels as virtual candidates over the product's own boxes, shared by the end-to-end tests"""
    if not _E2E:
        net = _mini(scores="darknet", multi_label=True)
        x = torch.from_numpy(orc.frames_to_input([synth_frames(50, 1, 32, 48)[0]] * len(E2E_SHAPES)))
        fwd = {k: v.cpu().numpy() for k, v in net.forward(x).items()}
        grids = [(v.h, v.w) for v in net.label_heads()]
        heads, rows_total = S.e2e_heads(len(E2E_SHAPES), grids)
        assert rows_total == fwd["class_prob"].shape[1]
        labels = S.labels(heads, S.E2E_THRESH)
        # float32 network: the best label of a row is forward()'s class_prob bit for bit (checked on the device's own labels below)
        _E2E.update(net=net, fwd=fwd, labels=labels, heads=heads, rows_total=rows_total)
    return _E2E


@pytest.mark.parametrize("nms_kind", [None, "iou", "diounms"])
@pytest.mark.parametrize("letterbox", [False, True])
def test_mini_multi_label_through_inference(letterbox, nms_kind):
    e = _e2e_reference()
    net, fwd = e["net"], e["fwd"]
    # (without letterboxing the reference's resize wants one frame size per batch: net-sized frames there)
    shapes = E2E_SHAPES if letterbox else [(32, 48)] * len(E2E_SHAPES)
    frames = _mini_frames(shapes)
    kw = dict(prob_thresh=S.E2E_THRESH, nms_iou_thresh=0.45, letterbox=letterbox, nms_kind=nms_kind)
    got = yolov3.inference(net, frames, device="cuda", return_rows=True, **kw)
    # the planted heads ignore the image: every frame's forward is the same, and so are its labels
    for f, (rows, cls, score) in enumerate(e["labels"]):
        vbox = fwd["bbox_xywh"][f][rows]
        shape = shapes[f]
        seen = correct_letterbox_boxes(vbox[None], [shape], 32, 48)[0] if letterbox else vbox
        if nms_kind is None:
            want = orc.postprocess(seen[None], score[None], cls[None], [shape], S.E2E_THRESH, 0.45, audit=True)[0]
            keep = want[3]
            want_boxes = want[0]
        else:
            keep = np.asarray(D.detect_keep_rows(seen, score, cls, S.E2E_THRESH, 0.45, nms_kind), np.int64)
            want_boxes = None
        tlbr, p, c, r = got[f]
        want_set = sorted(zip(rows[keep].tolist(), cls[keep].tolist()))
        assert sorted(zip(r.tolist(), c.tolist())) == want_set, "frame %d" % f
        assert len(want_set) > 2
        if want_boxes is not None:
            order = {k: i for i, k in enumerate(zip(rows[keep].tolist(), cls[keep].tolist()))}
            for i, k in enumerate(zip(r.tolist(), c.tolist())):
                assert np.array_equal(tlbr[i], want_boxes[order[k]]), "frame %d label %s" % (f, k)
        # one box keeps two classes; the class-7 box of anchor 1 is suppressed by the SECOND class of anchor 0's box in its cell
        by_row = {}
        for rr, cc in zip(r.tolist(), c.tolist()):
            by_row.setdefault(rr, []).append(cc)
        assert any(sorted(v) == [5, 7] for v in by_row.values()), "frame %d: no box with two classes" % f
    single = yolov3.inference(_mini(scores="darknet"), frames, device="cuda", return_rows=True, **kw)
    off = e["heads"][1]["row_offset"]
    hw = e["heads"][1]["t"].shape[1] * e["heads"][1]["t"].shape[2]
    n_a1 = lambda det: sum(1 for rr in det[3].tolist() if off + hw <= rr < off + 2 * hw)      # anchor 1 of the fine head
    assert sum(n_a1(d) for d in single) > sum(n_a1(d) for d in got), "the second class suppressed nothing"
    # detect_in_frames: the same lists
    streamed = list(yolov3.detect_in_frames(net, frames, batch_size=3, **kw))
    for a, b in zip(streamed, got):
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b[:3]))


def test_mini_best_label_is_forwards_score_and_capacity_error():
    e = _e2e_reference()
    net = e["net"]
    frame = synth_frames(50, 1, 32, 48)[0]
    out = net.forward_frames(np.stack([frame] * 2), fresh=False)
    heads = net.label_heads()
    rows_total = e["rows_total"]
    from yolov3.inference import Detector
    det = Detector(2, rows_total, out["class_prob"].device)
    det.run(out, np.asarray([(32, 48)] * 2, np.int32), float(F(S.E2E_THRESH)), 1.0, labels=heads)
    torch.cuda.synchronize()
    lb = det._label_run
    n = int(lb.vcount[0])
    vrow, vprob, vcls = lb.vrow[0, :n].cpu().numpy(), lb.vprob[0, :n].cpu().numpy(), lb.vcls[0, :n].cpu().numpy()
    prob, cls = out["class_prob"][0].cpu().numpy(), out["class_idx"][0].cpu().numpy()
    assert n == len(e["labels"][0][0]) and np.array_equal(vrow, e["labels"][0][0])
    for row in np.unique(vrow):
        k = np.nonzero(vrow == row)[0]
        best = k[np.argmax(vprob[k])]
        assert vprob[best].tobytes() == prob[row].tobytes() and vcls[best] == cls[row]
    res = det.fetch(return_rows=True)
    assert len(res[0][1]) == n                                         # iou_thresh 1.0 suppresses nothing
    # the capacity: an error naming frame, count and the argument, never a truncation
    with pytest.raises(RuntimeError, match=r"frame 0 has %d labels.*label_capacity=%d" % (n, n - 1)):
        yolov3.inference(net, [frame], device="cuda", prob_thresh=S.E2E_THRESH, label_capacity=n - 1)
    with pytest.raises(RuntimeError, match="label_capacity=%d" % (n - 1)):
        list(yolov3.detect_in_frames(net, [frame] * 3, batch_size=2, prob_thresh=S.E2E_THRESH, label_capacity=n - 1))
    assert len(yolov3.inference(net, [frame], device="cuda", prob_thresh=S.E2E_THRESH, nms_iou_thresh=1.0, label_capacity=n)[0][1]) == n
    # 16-bit storage: the heads stay float32, the path is the same
    net16 = _mini("bf16", scores="darknet", multi_label=True)
    got = yolov3.inference(net16, [frame], device="cuda", prob_thresh=S.E2E_THRESH, nms_iou_thresh=1.0, return_rows=True)[0]
    assert sorted(zip(got[3].tolist(), got[2].tolist())) == sorted(zip(e["labels"][0][0].tolist(), e["labels"][0][1].tolist()))


# ---- a process group, a capacity that is not the row count, frames over kmax -------------------------------------------------------
_GROUP_SCRIPT = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[3])
import numpy as np, torch, torch.distributed as dist, yolov3
from yolov3.pipeline import Pipeline
from yolov3.synthdata import synth_frames
import darknet_scores_restate as S
import test_gpu_darknet_scores as T
torch.cuda.set_device(0)
dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%s" % sys.argv[4], rank=0, world_size=1, device_id=torch.device("cuda", 0))
net = T._mini(scores="darknet", multi_label=True)
frames = np.stack([synth_frames(50 + k, 1, 32, 48)[0] for k in range(3)])
kw = dict(prob_thresh=S.E2E_THRESH, nms_iou_thresh=0.45)
out = {}
for cap in (330, 500):                                   # below and above the 360 prediction rows (a frame has 312 labels)
    want = yolov3.inference(net, list(frames), label_capacity=cap, return_rows=True, **kw)
    pipe = Pipeline(net, 3, in_flight=2, kmax=8, world=1, label_capacity=cap, **kw)
    assert pipe.gathers[0].collective and pipe.dets[0].rows == cap != pipe.rows
    ok = True
    for rep in range(3):
        got = pipe.results(pipe.submit(frames), return_rows=True)
        ok = ok and len(got) == len(want) and all(len(g) == len(w) and all(np.array_equal(a, b) for a, b in zip(g, w)) for g, w in zip(got, want))
    pipe.synchronize()
    out[str(cap)] = dict(equal=bool(ok), kept=[len(w[1]) for w in want])
print(json.dumps(out))
dist.destroy_process_group()
"""


def test_regather_with_a_label_capacity_that_is_not_the_row_count():
    """Under a process group (one rank) a frame that keeps more than kmax boxes is packed again from the ticket's detector
    buffers, whose frame stride in multi-label mode is the label capacity, not the number of prediction rows: frames 1 and 2
    come out right only with that stride."""
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    here = os.path.dirname(os.path.abspath(__file__))
    proc = subprocess.run([sys.executable, "-c", _GROUP_SCRIPT, os.path.join(ROOT, "pytorch-yolov3_amd"), here, ROOT, str(port)],
                          capture_output=True, text=True, timeout=300, env=env)
    assert proc.returncode == 0, proc.stderr[-2500:]
    d = json.loads([ln for ln in proc.stdout.splitlines() if ln.startswith("{")][0])
    for cap, r in d.items():
        assert r["equal"] and min(r["kept"]) > 8, (cap, r)
