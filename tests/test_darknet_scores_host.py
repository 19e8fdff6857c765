"""Darknet class scores and multi-label detections: everything that needs no GPU.

The restatement (tests/darknet_scores_restate.py) against a float64 evaluation on every input the GPU tests use, with the
margins that keep decisions off the last bit of expf; the C ABI additions in the header and the ctypes mirror; argument
checks of the Python surface and of ``y3_expand_labels``; the command line flags; a new_coords network compiles to the same ops
with and without ``scores="darknet"``."""
import ctypes
import os
import re

import numpy as np
import pytest

import yolov3
from yolov3 import _hip
from yolov3.__main__ import build_parser
from yolov3.darknet import yolo_decode_flags
from yolov3.plan import build_plan

import darknet_scores_restate as S
from golden_util import GOLDEN, MODEL_DIR, ROOT

MINI = os.path.join(GOLDEN, "cfg", "mini.cfg")
CSP = os.path.join(MODEL_DIR, "yolov4-csp.cfg")
HEADER = os.path.join(ROOT, "include", "yolov3_hip.h")


# ---- the restatement and its inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classes", S.DECODE_CLASSES)
@pytest.mark.parametrize("grid", S.DECODE_GRIDS)
def test_decode_inputs_and_restatement_against_float64(grid, classes):
    t = S.decode_case(grid, classes)
    assert t.shape == (3, grid[0], grid[1], 3, 5 + classes) and t.dtype == np.float32
    for v in (20.0, -20.0, 90.0, -90.0):
        assert bool((t[..., 4] == v).any()), "objectness logit %g missing" % v
    ties = S.check_argmax(t)
    if classes >= 2:
        assert ties >= 4, "planted ties missing"
        assert bool((t[..., 5:] >= 20.0).sum(-1).max() >= 2), "no pair of logits above 20"
    if classes >= 3:
        assert bool((t[..., 5:] == -90.0).any() and (t[..., 5:] == -20.0).any())
    prob, cls = S.decode_scores(t)
    obj, p = S.probabilities64(t)
    want = p.max(-1) * obj
    np.testing.assert_allclose(prob, want, rtol=1e-6, atol=1e-30)
    # the class: the first index whose float32 probability is the largest; away from planted ties that is float64's arg-max
    _, p32 = S.probabilities(t)
    assert np.array_equal(cls, np.argmax(p32, -1))
    if classes > 1:
        top = np.sort(p, -1)[..., -2:]
        clear = (top[..., 1] - top[..., 0]) > S.MARGIN
        assert np.array_equal(cls[clear], np.argmax(p, -1)[clear])
    assert bool(np.isfinite(prob).all()) and float(prob.max()) <= 1.0 and float(prob.min()) >= 0.0


def test_label_inputs_and_restatement_against_float64():
    heads, rows_total = S.label_case()
    assert rows_total == 3 * (4 * 6 + 8 * 12)
    for hd in heads:
        S.check_margins(hd["t"], S.THRESHOLDS)
    counts = {}
    for th in S.THRESHOLDS:
        got = S.labels(heads, th)
        for f, (rows, cls, score) in enumerate(got):
            key = rows * 1000 + cls
            assert bool((np.diff(key) > 0).all()), "labels not in ascending (row, c) order"
            want = set()
            for hd in heads:
                flat, rr = S.head_rows(hd["t"], hd["row_offset"])
                obj, p = S.probabilities64(flat[f])
                s = obj[:, None] * p
                r, c = np.nonzero((obj > th)[:, None] & (s > th))
                want |= set(zip(rr[r].tolist(), c.tolist()))
                for a, b, v in zip(rows.tolist(), cls.tolist(), score.tolist()):
                    if rr[0] <= a <= rr[-1]:
                        assert abs(v - s[a - rr[0], b]) <= 1e-6 * s[a - rr[0], b] + 1e-30
            assert set(zip(rows.tolist(), cls.tolist())) == want
            counts[(th, f)] = len(rows)
    # the thresholds separate: a fraction at 0.25, most at 0.001, every (row, class) at 0
    per_frame = sum(3 * hd["h"] * hd["w"] * hd["classes"] for hd in S.LABEL_HEADS)
    assert counts[(0.0, 0)] == per_frame and 0 < counts[(0.25, 0)] < counts[(0.001, 0)] < per_frame


def test_label_rule_edges():
    t = np.full((1, 1, 1, 1, 7), 2.0, np.float32)
    heads = [dict(t=t, row_offset=0, new_coords=False)]
    assert [len(x[0]) for x in S.labels(heads, 0.25)] == [2]
    nan_obj = t.copy()
    nan_obj[..., 4] = np.nan
    assert len(S.labels([dict(t=nan_obj, row_offset=0)], 0.0)[0][0]) == 0
    nan_cls = t.copy()
    nan_cls[..., 5] = np.nan
    rows, cls, _ = S.labels([dict(t=nan_cls, row_offset=0)], 0.0)[0]
    assert cls.tolist() == [1]
    # strict comparisons: a score equal to the threshold is no label; new_coords uses the stored values as they are
    half = np.zeros((1, 1, 1, 1, 6), np.float32)
    half[..., 4], half[..., 5] = 1.0, 0.25
    assert len(S.labels([dict(t=half, row_offset=0, new_coords=True)], 0.25)[0][0]) == 0
    assert len(S.labels([dict(t=half, row_offset=0, new_coords=True)], 0.2)[0][0]) == 1


def test_e2e_planted_logits_keep_the_margins():
    heads, _ = S.e2e_heads(2, [(4, 6), (8, 12)])
    for hd in heads:
        S.check_margins(hd["t"], (S.E2E_THRESH,))
    rows, cls, score = S.labels(heads, S.E2E_THRESH)[0]
    per_row = {}
    for r, c in zip(rows.tolist(), cls.tolist()):
        per_row.setdefault(r, []).append(c)
    assert sorted(set(map(tuple, per_row.values()))) == [(2,), (5, 7), (7,)]


# ---- the C ABI additions ---------------------------------------------------------------------------------------------------------
def test_header_and_ctypes_mirror_agree():
    text = open(HEADER).read()

    def define(name):
        return int(re.search(r"#define %s (\d+)u?\b" % name, text).group(1))
    assert define("Y3_F_SCORES_DARKNET") == 2048 == _hip.F_SCORES_DARKNET
    assert define("Y3_CAP_SCORES_DARKNET") == 128 == _hip.CAP_SCORES_DARKNET
    assert define("Y3_CAP_MULTI_LABEL") == 256 == _hip.CAP_MULTI_LABEL
    assert define("Y3_ABI_VERSION") == 6 == _hip.ABI_VERSION
    assert ctypes.sizeof(_hip.Y3Op) == 248
    m = re.search(r"typedef struct \{\s*const float \*d_head;\s*int32_t ([^;]+);\s*\} y3_head_view;", text)
    assert m, "y3_head_view not declared"
    names = [n.strip() for n in m.group(1).split(",")]
    assert ["d_head"] + names == [f[0] for f in _hip.Y3HeadView._fields_]
    assert ctypes.sizeof(_hip.Y3HeadView) == 40
    for name in ("y3_expand_labels_workspace_bytes", "y3_expand_labels"):
        assert re.search(r"\b%s\(" % name, text) and name in _hip.PROTOTYPES
    assert len(_hip.PROTOTYPES["y3_expand_labels"][1]) == 15 and len(_hip.PROTOTYPES["y3_expand_labels_workspace_bytes"][1]) == 3


def test_library_reports_the_capabilities_and_the_entry_points():
    lib = _hip.lib()
    assert lib.y3_abi_version() == 6
    caps = _hip.capabilities()
    assert caps & _hip.CAP_SCORES_DARKNET and caps & _hip.CAP_MULTI_LABEL
    _hip.require_capabilities(_hip.CAP_SCORES_DARKNET | _hip.CAP_MULTI_LABEL, "test")
    assert lib.y3_expand_labels_workspace_bytes(2, 360, 360) >= 2 * 6 * 4
    assert lib.y3_expand_labels_workspace_bytes(16, 22743, 22743) >= 16 * 356 * 4


def test_require_capabilities_names_the_new_bits(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: 0)
    with pytest.raises(_hip.HipLibraryError, match="Darknet class scores"):
        _hip.require_capabilities(_hip.CAP_SCORES_DARKNET, "x.cfg")
    with pytest.raises(_hip.HipLibraryError, match="multi-label"):
        _hip.require_capabilities(_hip.CAP_MULTI_LABEL, "x.cfg")


def _expand(heads, thresh=0.25, cap=8, rows_total=8, batch=1):
    """y3_expand_labels with addresses that are never dereferenced: every argument check happens before any launch"""
    fake = 1 << 20
    views = (_hip.Y3HeadView * len(heads))(*heads)
    return _hip.lib().y3_expand_labels(views, len(heads), fake, batch, rows_total, ctypes.c_float(thresh), cap, fake, 1 << 16,
                                       fake, fake, fake, fake, fake, None)


def _view(**kw):
    d = dict(d_head=1 << 20, h=2, w=2, ld=16, n_anchor=2, n_attr=7, row_offset=0, new_coords=0)
    d.update(kw)
    return _hip.Y3HeadView(**d)


@pytest.mark.parametrize("kw", [dict(thresh=-0.1), dict(thresh=float("nan")), dict(thresh=float("inf")), dict(cap=0),
                                dict(cap=-3), dict(batch=0), dict(rows_total=0)])
def test_expand_labels_refuses_bad_scalars(kw):
    assert _expand([_view()], **kw) == -1
    assert _hip.lib().y3_last_error()


@pytest.mark.parametrize("view", [dict(ld=12), dict(n_attr=5), dict(row_offset=4), dict(row_offset=-1), dict(d_head=None),
                                  dict(h=0)])
def test_expand_labels_refuses_bad_heads(view):
    assert _expand([_view(**view)]) == -1


def test_expand_labels_refuses_overlapping_heads_and_too_many():
    assert _expand([_view(), _view(row_offset=4)], rows_total=16) == -1
    assert _expand([_view(n_anchor=1, row_offset=k * 4) for k in range(9)], rows_total=36) == -1
    assert _expand([], rows_total=8) == -1


def test_scores_flag_on_another_op_kind_is_invalid():
    lib = _hip.lib()
    op = _hip.Y3Op()
    op.kind, op.dtype, op.batch = _hip.OP_MAXPOOL, _hip.Y3_F32, 1
    op.in_h = op.in_w = op.out_h = op.out_w = 4
    op.in_c = op.out_c = op.in_ld = op.out_ld = 8
    op.ksize, op.stride = 2, 2
    op.flags = _hip.F_SCORES_DARKNET
    op.d_in = op.d_out = 1 << 20
    assert lib.y3_op_run(ctypes.byref(op), None, 1 << 20, None) == -1
    assert b"Y3_F_SCORES_DARKNET" in lib.y3_last_error()
    handle = ctypes.c_void_p()
    assert lib.y3_plan_create((_hip.Y3Op * 1)(op), 1, 1 << 20, ctypes.byref(handle)) == -1


# ---- the Python surface ----------------------------------------------------------------------------------------------------------
def test_constructor_modes():
    net = yolov3.Darknet(MINI)
    assert net.scores == "reference" and net.multi_label is False
    net = yolov3.Darknet(MINI, scores="darknet", multi_label=True)
    assert net.scores == "darknet" and net.multi_label is True
    for attr in ("scores", "multi_label"):
        with pytest.raises(AttributeError):
            setattr(net, attr, "reference")
    with pytest.raises(ValueError, match="scores"):
        yolov3.Darknet(MINI, scores="softmax")
    with pytest.raises(ValueError, match="multi_label=True needs scores"):
        yolov3.Darknet(MINI, multi_label=True)
    # a network all of whose heads are new_coords scores the Darknet way already
    assert yolov3.Darknet(CSP, multi_label=True).multi_label is True
    with pytest.raises(RuntimeError, match="multi_label=True"):
        yolov3.Darknet(MINI, scores="darknet").label_heads()


def test_new_coords_network_compiles_to_the_same_ops_in_both_modes():
    net = yolov3.Darknet(CSP)
    desc = build_plan(net.blocks, net.net_info, 2, 512, 512, 2)
    yolo = [od for od in desc["ops"] if od["kind"] == "yolo"]
    assert len(yolo) == 3
    for od in yolo:
        assert yolo_decode_flags(od, "darknet") == yolo_decode_flags(od, "reference") == (_hip.F_NEW_COORDS, _hip.CAP_NEW_COORDS)
    mini = yolov3.Darknet(MINI)
    for od in build_plan(mini.blocks, mini.net_info, 2, 32, 48, 4)["ops"]:
        if od["kind"] == "yolo":
            assert yolo_decode_flags(od, "reference") == (0, 0)
            assert yolo_decode_flags(od, "darknet") == (_hip.F_SCORES_DARKNET, _hip.CAP_SCORES_DARKNET)


def test_keep_heads_only_extends_the_head_tensors_lives():
    net = yolov3.Darknet(MINI)
    a = build_plan(net.blocks, net.net_info, 2, 32, 48, 2)
    b = build_plan(net.blocks, net.net_info, 2, 32, 48, 2, keep_heads=True)
    strip = lambda ops: [{k: v for k, v in od.items() if k not in ("inp", "out", "res")} for od in ops]
    assert strip(a["ops"]) == strip(b["ops"])
    heads = [od["inp"].buf for od in b["ops"] if od["kind"] == "yolo"]
    assert len(heads) == 2
    spans = []
    for buf in heads:
        assert b["live"][1][buf] == len(b["ops"]) - 1
        spans.append((b["offsets"][buf], b["offsets"][buf] + b["buffers"][buf]))
    # no other buffer that is written after a head conv shares its bytes
    for buf, off in b["offsets"].items():
        if buf in heads:
            continue
        for hb, (lo, hi) in zip(heads, spans):
            overlap = off < hi and lo < off + b["buffers"][buf]
            assert not (overlap and b["live"][1][buf] >= b["live"][0][hb]), (buf, hb)


def test_command_line_flags():
    base = ["-I", "x.jpg", "-c", "a.cfg", "-w", "a.weights"]
    args = build_parser().parse_args(base)
    assert args.darknet_scores is False and args.multi_label is False
    args = build_parser().parse_args(base + ["--darknet-scores"])
    assert args.darknet_scores is True and args.multi_label is False
    args = build_parser().parse_args(base + ["--letterbox", "--darknet-pool", "--darknet-scores", "--multi-label", "--nms-kind",
                                             "greedynms", "-p", "0.25", "-i", "0.45"])
    assert args.multi_label and args.darknet_scores and args.nms_kind == "greedynms"


def test_label_capacity_error_names_frame_count_and_capacity():
    from yolov3.inference import raise_label_overflow
    raise_label_overflow([3, 8], 8)
    with pytest.raises(RuntimeError, match=r"frame 1 has 9 labels.*label_capacity=8"):
        raise_label_overflow([3, 9], 8)


def test_to_coco_emits_one_annotation_per_label():
    from yolov3.stream import to_coco
    box = np.array([[1, 2, 11, 22], [1, 2, 11, 22]], np.int64)          # one box, two classes
    coco = to_coco(["a.jpg"], [[box, np.array([0.9, 0.4], np.float32), np.array([5, 7], np.int64)]], [str(i) for i in range(8)])
    assert [(a["category_id"], a["bbox"]) for a in coco["annotations"]] == [(5, [1, 2, 10, 20]), (7, [1, 2, 10, 20])]
