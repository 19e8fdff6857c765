"""Darknet's suppression rule on the GPU (-m gpu): ``y3_nms_darknet`` / ``y3_detect_darknet`` against the restatement in
tests/darknet_nms_restate.py -- EXACT equality of the kept index lists -- and the public entry points with ``nms_kind=...``.
The inputs are those tests/test_darknet_nms_host.py shows to be robust (no box decided by the last bit of ``pow``) and to tell
the three kinds apart.  ``nms_kind=None`` must stay today's path bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3.inference import Detector
from yolov3.pipeline import Pipeline
from yolov3.preprocess import correct_letterbox_boxes, letterbox_u8
from yolov3.synthdata import synth_frames

import darknet_nms_restate as D
from detect_util import dev as _dev, direct_detect as _direct_detect, out as _out, run_detector as _run, same as _same
from golden_util import GOLDEN, MODELS, SAMPLE_IMAGES, golden_params, golden_weights_path, load_jpeg_bgr

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
F = np.float32
nms = yolov3.non_max_suppression_darknet


# ---- y3_nms_darknet / non_max_suppression_darknet ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("case", D.CASES, ids=lambda c: "seed%d_n%d_c%d" % c)
def test_nms_darknet_equals_restatement(case, kind):
    x, p, c = D.clusters(*case)
    want = D.keep_fast(x, p, c, D.THRESH, kind, D.BETA)
    got = nms(x, p, c, thresh=D.THRESH, nms_kind=kind, beta_nms=D.BETA)
    print("case %s %s: kept %d of %d" % (case, kind, len(got), len(p)))
    assert got == want


@pytest.mark.parametrize("kind", D.KINDS)
@pytest.mark.parametrize("case", D.BIG_CASES, ids=["one_class_2400_flag_chain", "5000_global_sort"])
def test_nms_darknet_many_chunks_and_global_sort(case, kind):
    x, p, c = D.clusters(*case)
    want = D.keep_fast(x, p, c, D.THRESH, kind, D.BETA)
    got = nms(x, p, c, thresh=D.THRESH, nms_kind=kind, beta_nms=D.BETA)
    print("case %s %s: kept %d of %d" % (case, kind, len(got), len(p)))
    assert got == want
    assert len(got) > 64


@pytest.mark.parametrize("kind", D.KINDS)
def test_nms_darknet_edges(kind):
    one = np.array([[0.5, 0.5, 0.2, 0.3]], F)
    assert nms(one, [0.7], [3], nms_kind=kind) == [0]
    assert nms(one, [0.7], None, nms_kind=kind) == [0]
    assert nms(np.zeros((0, 4), F), np.zeros(0, F), nms_kind=kind) == []
    # class_idx=None: one class
    x, p, c = D.clusters(3, 300, 5)
    assert nms(x, p, None, thresh=D.THRESH, nms_kind=kind) == D.keep_fast(x, p, None, D.THRESH, kind, D.BETA)
    assert nms(x, p, c, thresh=D.THRESH, nms_kind=kind) == D.keep_fast(x, p, c, D.THRESH, kind, D.BETA)
    # all boxes identical: m = 1 for every pair, the best one stays (thresh 1: 1 > 1 is false, all stay)
    same = np.tile(one, (200, 1))
    ps = np.random.default_rng(0).uniform(0.1, 1, 200).astype(F)
    assert nms(same, ps, None, thresh=0.45, nms_kind=kind) == [int(np.argmax(ps))] == D.keep_fast(same, ps, None, 0.45, kind)
    assert nms(same, ps, None, thresh=1.0, nms_kind=kind) == D.canonical_order(ps, None)
    # all boxes disjoint: every measure is <= 0, all stay even at thresh 0
    grid = np.array([[0.05 + 0.1 * (i % 10), 0.05 + 0.1 * (i // 10), 0.05, 0.05] for i in range(100)], F)
    pg = np.random.default_rng(1).uniform(0.1, 1, 100).astype(F)
    assert nms(grid, pg, None, thresh=0.0, nms_kind=kind) == D.canonical_order(pg, None)
    # thresh 0 and 1 on overlapping boxes
    for thresh in (0.0, 1.0):
        assert nms(x, p, c, thresh=thresh, nms_kind=kind) == D.keep_fast(x, p, c, thresh, kind, D.BETA)
    assert len(nms(x, p, c, thresh=1.0, nms_kind=kind)) == len(p)
    # zero-size boxes at one point (c == 0): nobody is suppressed
    dots = np.tile(np.array([[0.5, 0.5, 0.0, 0.0]], F), (70, 1))
    assert nms(dots, ps[:70], None, thresh=0.0, nms_kind=kind) == D.canonical_order(ps[:70], None)


def test_nms_darknet_beta_matters():
    x, p, c = D.clusters(1, 300, 1)
    a, b = nms(x, p, c, thresh=D.THRESH, nms_kind="diounms", beta_nms=0.6), nms(x, p, c, thresh=D.THRESH, nms_kind="diounms", beta_nms=1.0)
    assert a == D.keep_fast(x, p, c, D.THRESH, "diounms", 0.6) and b == D.keep_fast(x, p, c, D.THRESH, "diounms", 1.0)
    assert a != b
    assert b == nms(x, p, c, thresh=D.THRESH, nms_kind="greedynms")          # beta 1: the penalty is d / c itself


# ---- Detector.run(nms_kind=...) ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("kind", D.KINDS)
def test_detector_darknet_rows_equal_restatement(kind, letterbox):
    box, prob, cls = D.detector_inputs()
    shapes = D.DETECT_SHAPES if letterbox else [D.DETECT_NET] * D.DETECT_BATCH
    lb = D.DETECT_NET if letterbox else None
    seen = correct_letterbox_boxes(box, shapes, *D.DETECT_NET) if letterbox else box
    got = _run(box, prob, cls, shapes, D.DETECT_PROB_THRESH, D.THRESH, lb, nms_kind=kind, beta_nms=D.BETA)
    # the default rule at iou_thresh 1.0 suppresses nothing that is not a +1-area IoU above 1: every candidate, by row
    every = _run(box, prob, cls, shapes, D.DETECT_PROB_THRESH, 1.0, lb)
    for f in range(D.DETECT_BATCH):
        want = D.detect_keep_rows(seen[f], prob[f], cls[f], D.DETECT_PROB_THRESH, D.THRESH, kind, D.BETA)
        tlbr, p, c, rows = got[f]
        print("frame %d %s letterbox=%s: kept %d" % (f, kind, letterbox, len(rows)))
        assert rows.tolist() == want, "frame %d" % f
        assert len(want) > 10
        assert tlbr.dtype == np.int64 and p.dtype == np.float32 and c.dtype == np.int64
        by_row = {int(r): k for k, r in enumerate(every[f][3])}
        assert len(by_row) == int((prob[f] >= F(D.DETECT_PROB_THRESH)).sum())
        for k, r in enumerate(rows.tolist()):
            j = by_row[r]
            assert np.array_equal(tlbr[k], every[f][0][j]) and p[k].tobytes() == every[f][1][j].tobytes() and c[k] == every[f][2][j]
            assert p[k].tobytes() == prob[f, r].tobytes() and c[k] == cls[f, r]
    # frames are independent: a frame alone gives what it gives inside the batch
    for f in (0, 4, 15):
        alone = _run(box[f:f + 1], prob[f:f + 1], cls[f:f + 1], shapes[f:f + 1], D.DETECT_PROB_THRESH, D.THRESH, lb,
                     nms_kind=kind, beta_nms=D.BETA)
        _same(alone, [got[f]])


def test_detector_darknet_letterbox_net_sized_is_the_identity():
    box, prob, cls = D.detector_inputs(3, 1000, 5)
    shapes = [D.DETECT_NET] * 3
    a = _run(box, prob, cls, shapes, 0.6, D.THRESH, D.DETECT_NET, nms_kind="diounms")
    b = _run(box, prob, cls, shapes, 0.6, D.THRESH, None, nms_kind="diounms")
    _same(a, b)


def test_detector_reuses_one_object_for_both_rules():
    """One Detector alternating between the rules (as a Pipeline whose nms_kind is changed does): neither disturbs the other."""
    box, prob, cls = D.detector_inputs(4, 1200, 8)
    shapes = [D.DETECT_NET] * 4
    det = Detector(4, 1200, _dev())
    out = _out(box, prob, cls)
    hw = np.asarray(shapes, np.int32)
    res = []
    for kind in (None, "diounms", None, "iou", "diounms"):
        det.run(out, hw, float(F(0.6)), D.THRESH, nms_kind=kind)
        res.append(det.fetch(return_rows=True))
    _same(res[0], res[2])
    _same(res[1], res[4])
    _same(res[0], _direct_detect(box, prob, cls, shapes, 0.6, D.THRESH))
    assert [r[3].tolist() for r in res[3]] == [D.detect_keep_rows(box[f], prob[f], cls[f], 0.6, D.THRESH, "iou") for f in range(4)]


# ---- nms_kind=None is today's path ---------------------------------------------------------------------------------------------
def _tiny(dtype="float32"):
    return yolov3.Darknet(MODELS["yolov3-tiny"], device="cuda", dtype=dtype).set_params(golden_params("yolov3-tiny")).eval()


def test_none_is_the_default_path_bit_for_bit():
    box, prob, cls = D.detector_inputs()
    shapes = D.DETECT_SHAPES
    want = _direct_detect(box, prob, cls, shapes, 0.6, 0.3)
    _same(_run(box, prob, cls, shapes, 0.6, 0.3), want)
    _same(_run(box, prob, cls, shapes, 0.6, 0.3, nms_kind=None, beta_nms=0.6), want)
    # inference() and Pipeline on a network's own outputs
    net = _tiny()
    frames = synth_frames(21, 16, 416, 416)
    fwd = {k: v.cpu().numpy() for k, v in net.forward_frames(frames).items()}
    hw = [(416, 416)] * 16
    want = _direct_detect(fwd["bbox_xywh"], fwd["class_prob"], fwd["class_idx"], hw, 0.05, 0.3)
    assert sum(len(w[1]) for w in want) > 0
    _same(yolov3.inference(net, list(frames), return_rows=True), want)
    _same(yolov3.inference(net, list(frames), return_rows=True, nms_kind=None), want)
    for kw in ({}, {"nms_kind": None}):
        pipe = Pipeline(net, 16, **kw)
        ticket = pipe.submit(torch.from_numpy(frames))
        _same(pipe.results(ticket, return_rows=True), want)
        pipe.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_tiny_end_to_end_inference_frames_cli_and_restatement(tmp_path):
    net = _tiny()
    dim = net.net_info["height"]
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES] + list(synth_frames(5, 9, dim, dim))
    assert len(images) == 18                                   # a full batch of 16 and a short one through Pipeline
    kw = dict(prob_thresh=0.05, nms_iou_thresh=D.THRESH, nms_kind="diounms", beta_nms=D.BETA)
    one = yolov3.inference(net, images, device="cuda", return_rows=True, **kw)
    streamed = list(yolov3.detect_in_frames(net, images, batch_size=16, **kw))
    _same([r[:3] for r in one], streamed)
    # the restatement fed the forward's own outputs (frames stretched to the network size, as inference() does)
    from yolov3.preprocess import prepare_frames
    stretched, _ = prepare_frames(images, dim, dim)
    fwd = {k: v.cpu().numpy() for k, v in net.forward_frames(stretched).items()}
    kept = 0
    for f in range(len(images)):
        def rows(nudge, kind="diounms"):
            return D.detect_keep_rows(fwd["bbox_xywh"][f], fwd["class_prob"][f], fwd["class_idx"][f], 0.05, D.THRESH, kind,
                                      D.BETA, nudge)
        want = rows(0)
        assert want == rows(1) == rows(-1), "frame %d: an input decided by the last bit of pow" % f
        assert one[f][3].tolist() == want, "frame %d" % f
        kept += len(want)
    assert kept > 0
    # and the other modes give something else somewhere
    default = yolov3.inference(net, images, device="cuda", return_rows=True, prob_thresh=0.05, nms_iou_thresh=D.THRESH)
    assert any(a[3].tolist() != b[3].tolist() for a, b in zip(one, default))
    # the command line
    img = os.path.join(GOLDEN, "images", SAMPLE_IMAGES[0])
    dump = tmp_path / "det.json"
    cmd = [sys.executable, "-m", "yolov3", "-c", MODELS["yolov3-tiny"], "-w", golden_weights_path("yolov3-tiny"), "-I", img,
           "-p", "0.05", "-i", str(D.THRESH), "--nms-kind", "diounms", "--beta-nms", str(D.BETA), "--json", str(dump)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pytorch-yolov3_amd")))
    assert res.returncode == 0, res.stderr[-2000:]
    with open(dump) as fh:
        coco = json.load(fh)
    tlbr, prob, cls = streamed[0]
    assert len(coco["annotations"]) == len(prob) > 0
    got = sorted((a["category_id"], a["score"], tuple(a["bbox"])) for a in coco["annotations"])
    want = sorted((int(c), float(p), (int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])))
                  for b, p, c in zip(tlbr.tolist(), prob.tolist(), cls.tolist()))
    assert got == want


def test_letterbox_and_darknet_nms_together_through_inference():
    net = _tiny()
    dim = net.net_info["height"]
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES[:4]]
    got = yolov3.inference(net, images, device="cuda", return_rows=True, prob_thresh=0.05, nms_iou_thresh=D.THRESH, letterbox=True,
                           nms_kind="greedynms")
    boxed = np.stack([letterbox_u8(im, dim, dim) for im in images])
    fwd = {k: v.cpu().numpy() for k, v in net.forward_frames(boxed).items()}
    fixed = correct_letterbox_boxes(fwd["bbox_xywh"], [im.shape[:2] for im in images], dim, dim)
    for f in range(len(images)):
        assert got[f][3].tolist() == D.detect_keep_rows(fixed[f], fwd["class_prob"][f], fwd["class_idx"][f], 0.05, D.THRESH,
                                                        "greedynms")


# ---- beside a kernel that saturates the memory system ---------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["iou", "diounms"])
def test_darknet_tail_beside_a_copy_kernel(kind):
    """The chunk chain of a class spins on LDS flags while other wavefronts work: 16 frames of one class of 2400 candidates
    (38 chunks each) next to ``y3_copy_bytes`` from pinned host memory equal the tail's own quiet output (the pattern of
    tests/test_gpu_contention.py)."""
    lib = _hip.lib()
    dev = _dev()
    frames = [D.clusters(200 + f, 2400, 1) for f in range(16)]
    box, prob, cls = (np.stack([fr[k] for fr in frames]) for k in range(3))
    out = _out(box, prob, cls)
    hw = torch.tensor([[608, 608]] * 16, dtype=torch.int32, device=dev)
    det = Detector(16, 2400, dev)

    def launch():
        det.run(out, hw, float(F(0.05)), D.THRESH, nms_kind=kind, beta_nms=D.BETA)

    launch()
    alone = det.fetch(return_rows=True, kmax=2400)
    assert alone[0][3].tolist() == D.detect_keep_rows(box[0], prob[0], cls[0], 0.05, D.THRESH, kind, D.BETA)
    host = torch.zeros(16 * 608 * 608 * 3, dtype=torch.uint8).pin_memory()
    dst = torch.zeros(16 * 608 * 608 * 3, dtype=torch.uint8, device=dev)
    cs, st = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for i in range(20):
        _hip.check(lib.y3_copy_bytes(host.data_ptr(), dst.data_ptr(), host.numel(), 8, _hip.stream_ptr(cs)))
        with torch.cuda.stream(st):
            for _ in range(6):
                launch()
        if i % 5 == 4:
            torch.cuda.synchronize()
            _same(det.fetch(return_rows=True, kmax=2400), alone)
    torch.cuda.synchronize()
