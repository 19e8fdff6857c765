"""Darknet's suppression rule without a GPU: the restatement (tests/darknet_nms_restate.py) on hand-computed pairs, the argument
handling of the public entry points, and a condition on the INPUTS of tests/test_gpu_darknet_nms.py: no committed input decides a
box by the last bit of ``pow``."""
import ctypes
import os

import numpy as np
import pytest

import yolov3
from yolov3 import _hip
from yolov3.preprocess import correct_letterbox_boxes

import darknet_nms_restate as D
from golden_util import ROOT

F = np.float32


def _box(x, y, w, h):
    return tuple(F(v) for v in (x, y, w, h))


# ---- the rule on pairs computed by hand -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", D.KINDS)
def test_identical_boxes_measure_one(kind):
    a = _box(0.5, 0.5, 0.25, 0.5)
    assert D.measure(a, a, kind) == F(1)          # I = U, d = 0: every kind gives exactly 1


def test_disjoint_boxes():
    a, b = _box(0.25, 0.25, 0.25, 0.25), _box(0.75, 0.75, 0.25, 0.25)
    assert D.measure(a, b, "iou") == 0
    # cw = ch = 0.875 - 0.125 = 0.75, c = 1.125, d = 0.5^2 * 2 = 0.5, d / c = 4 / 9: both DIoU measures are negative
    ratio = F(0.5) / F(1.125)
    assert D.measure(a, b, "greedynms") == -ratio
    assert D.measure(a, b, "diounms", 1.0) == -ratio
    assert D.measure(a, b, "diounms", 0.6) == -F(float(ratio) ** float(F(0.6)))
    for kind in D.KINDS:
        assert D.keep(np.array([a, b], F), [0.9, 0.8], None, 0.0, kind) == [0, 1]


def test_side_by_side_half_overlap():
    # two unit squares, centres 0.5 apart: I = 0.5, U = 1.5, iou = 1/3; cw = 1.5, ch = 1, c = 3.25, d = 0.25
    a, b = _box(1.0, 1.0, 1.0, 1.0), _box(1.5, 1.0, 1.0, 1.0)
    third = F(0.5) / F(1.5)
    assert D.measure(a, b, "iou") == third
    assert D.measure(a, b, "greedynms") == third - F(0.25) / F(3.25)
    boxes = np.array([a, b], F)
    assert D.keep(boxes, [0.9, 0.8], None, 0.3, "iou") == [0]                  # 0.333 > 0.3: suppressed
    assert D.keep(boxes, [0.9, 0.8], None, 0.3, "greedynms") == [0, 1]         # 0.333 - 0.077 = 0.256: kept
    assert D.keep(boxes, [0.9, 0.8], None, 0.3, "diounms", 0.6) == [0, 1]      # 0.333 - 0.077^0.6 = 0.119: kept
    assert D.keep_fast(boxes, [0.9, 0.8], None, 0.3, "iou") == [0]
    assert D.keep_fast(boxes, [0.9, 0.8], None, 0.3, "greedynms") == [0, 1]


@pytest.mark.parametrize("kind", D.KINDS)
def test_two_zero_size_boxes_at_one_point(kind):
    a = _box(0.5, 0.5, 0.0, 0.0)
    assert D.measure(a, a, kind) == 0             # I = 0 -> iou = 0; c = 0 -> m = iou, no division
    assert D.keep(np.array([a, a], F), [0.5, 0.5], None, 0.0, kind) == [1, 0]   # equal scores: higher index first


def test_order_classes_and_suppressed_boxes_suppress_nobody():
    # a chain a - b - c along x where only neighbours overlap above the threshold: b falls to a, so c stays
    boxes = np.array([_box(1.0, 1, 1, 1), _box(1.3, 1, 1, 1), _box(1.6, 1, 1, 1)], F)
    assert D.keep(boxes, [0.9, 0.8, 0.7], None, 0.45, "iou") == [0, 2]
    assert D.keep(boxes, [0.9, 0.8, 0.7], [1, 0, 1], 0.45, "iou") == [1, 0, 2]  # classes are independent, class ascending
    assert D.keep_fast(boxes, [0.9, 0.8, 0.7], None, 0.45, "iou") == [0, 2]


def test_vectorised_restatement_equals_the_scalar_one():
    for seed, n, nc in D.CASES[0:2] + D.CASES[12:14] + D.CASES[24:26]:
        x, p, c = D.clusters(seed, n, nc)
        for kind in D.KINDS:
            for nudge in (0, 1):
                assert D.keep(x, p, c, D.THRESH, kind, D.BETA, nudge) == D.keep_fast(x, p, c, D.THRESH, kind, D.BETA, nudge)


# ---- robustness of the GPU tests' inputs --------------------------------------------------------------------------------------
def _fragile(keep_fn):
    base = keep_fn(0)
    return base != keep_fn(1) or base != keep_fn(-1)


def test_gpu_test_inputs_do_not_hang_on_the_last_bit_of_pow():
    fragile = []
    for seed, n, nc in D.CASES + D.BIG_CASES:
        x, p, c = D.clusters(seed, n, nc)
        if _fragile(lambda nudge: D.keep_fast(x, p, c, D.THRESH, "diounms", D.BETA, nudge)):
            fragile.append((seed, n, nc))
    box, prob, cls = D.detector_inputs()
    fixed = correct_letterbox_boxes(box, D.DETECT_SHAPES, *D.DETECT_NET)
    for name, boxes in (("plain", box), ("letterbox", fixed)):
        for f in range(D.DETECT_BATCH):
            if _fragile(lambda nudge: D.detect_keep_rows(boxes[f], prob[f], cls[f], D.DETECT_PROB_THRESH, D.THRESH, "diounms",
                                                         D.BETA, nudge)):
                fragile.append((name, f))
    assert fragile == []


def test_gpu_test_inputs_tell_the_three_kinds_apart():
    for seed, n, nc in D.CASES + D.BIG_CASES:
        x, p, c = D.clusters(seed, n, nc)
        kept = {kind: tuple(D.keep_fast(x, p, c, D.THRESH, kind, D.BETA)) for kind in D.KINDS}
        assert len(set(kept.values())) == 3, (seed, n, nc, {k: len(v) for k, v in kept.items()})
    box, prob, cls = D.detector_inputs()
    for f in range(D.DETECT_BATCH):
        kept = {kind: tuple(D.detect_keep_rows(box[f], prob[f], cls[f], D.DETECT_PROB_THRESH, D.THRESH, kind, D.BETA))
                for kind in D.KINDS}
        assert len(set(kept.values())) == 3, (f, {k: len(v) for k, v in kept.items()})


# ---- argument handling that needs no GPU --------------------------------------------------------------------------------------
def test_hip_declares_the_new_symbols_and_capability():
    assert (_hip.NMS_IOU, _hip.NMS_GREEDY, _hip.NMS_DIOU, _hip.CAP_NMS_DARKNET) == (0, 1, 2, 64)
    assert _hip.NMS_KINDS == {"iou": 0, "greedynms": 1, "diounms": 2}
    for name in ("y3_detect_darknet_workspace_bytes", "y3_detect_darknet", "y3_nms_darknet_workspace_bytes", "y3_nms_darknet"):
        assert name in _hip.PROTOTYPES and name in _hip._OPTIONAL
        assert hasattr(_hip.lib(), name)
    assert _hip.capabilities() & _hip.CAP_NMS_DARKNET
    _hip.require_capabilities(_hip.CAP_NMS_DARKNET, "test")
    with open(os.path.join(ROOT, "include", "yolov3_hip.h")) as fh:
        header = fh.read()
    for line in ("#define Y3_NMS_IOU 0", "#define Y3_NMS_GREEDY 1", "#define Y3_NMS_DIOU 2", "#define Y3_CAP_NMS_DARKNET 64u",
                 "#define Y3_ABI_VERSION 6"):
        assert line in header


def test_stale_library_is_refused(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: _hip.CAP_LETTERBOX)
    with pytest.raises(_hip.HipLibraryError, match="Darknet NMS"):
        _hip.require_capabilities(_hip.CAP_NMS_DARKNET | _hip.CAP_LETTERBOX, "test")


def test_workspace_queries_and_c_abi_argument_errors():
    lib = _hip.lib()
    assert lib.y3_detect_darknet_workspace_bytes(16, 22743) >= lib.y3_detect_workspace_bytes(16, 22743) + 16 * 22743 * 16
    assert lib.y3_detect_darknet_workspace_bytes(0, 10) == 0
    assert lib.y3_nms_darknet_workspace_bytes(0) == 256 and lib.y3_nms_darknet_workspace_bytes(1000) > 0
    # the existing queries answer what they answered before the mode existed
    assert (lib.y3_detect_workspace_bytes(2, 1000), lib.y3_detect_workspace_bytes(16, 22743)) == (147968, 28580352)
    assert (lib.y3_nms_workspace_bytes(10), lib.y3_nms_workspace_bytes(5000)) == (2304, 405504)
    count = ctypes.c_int32(7)
    # checked before anything touches a device: kind, then beta (finite and > 0, whatever the kind)
    for kind, beta, word in ((3, 0.6, b"nms_kind"), (-1, 0.6, b"nms_kind"), (2, 0.0, b"beta_nms"), (0, -1.0, b"beta_nms"),
                             (2, float("inf"), b"beta_nms"), (2, float("nan"), b"beta_nms")):
        rc = lib.y3_nms_darknet(None, None, None, 0, 0.45, kind, beta, None, 0, None, ctypes.addressof(count), None)
        assert rc == -1 and word in lib.y3_last_error(), (kind, beta, lib.y3_last_error())
    rc = lib.y3_detect_darknet(None, None, None, 1, 10, None, 0.5, 0.45, None, 0, None, None, None, None, None, 0, 0, 1, 0.6, None)
    assert rc == -1 and b"null pointer" in lib.y3_last_error()


def test_nms_mode_validates_kind_and_beta():
    assert _hip.nms_mode(None) is None and _hip.nms_mode(None, beta_nms=-3) is None
    assert _hip.nms_mode("iou") == (0, float(F(0.6)))
    assert _hip.nms_mode("greedynms", 1.0) == (1, 1.0)
    assert _hip.nms_mode("diounms", 0.25) == (2, 0.25)
    for bad in ("cornersnms", "DIOUNMS", "", 2, b"iou"):
        with pytest.raises(ValueError):
            _hip.nms_mode(bad)
    for beta in (0, -0.5, float("inf"), float("nan"), 1e60, 1e-60):      # the last two are inf / 0 as float32
        with pytest.raises(ValueError):
            _hip.nms_mode("diounms", beta)


def test_non_max_suppression_darknet_refuses_bad_arguments_without_a_gpu():
    nms = yolov3.non_max_suppression_darknet
    assert "non_max_suppression_darknet" in yolov3.__all__
    box = np.array([[0.5, 0.5, 0.2, 0.2], [0.5, 0.5, 0.2, 0.2]], F)
    prob = np.array([0.9, 0.8], F)
    with pytest.raises(ValueError):
        nms(box, prob, nms_kind="cornersnms")
    with pytest.raises(ValueError):
        nms(box, prob, nms_kind=None)
    with pytest.raises(ValueError):
        nms(box, prob, nms_kind="diounms", beta_nms=0.0)
    with pytest.raises(ValueError):
        nms(box, prob, nms_kind="iou", beta_nms=float("nan"))
    for dtype in (np.float64, np.float16, np.int64):
        with pytest.raises(TypeError):
            nms(box.astype(dtype), prob)
    for bad in (np.nan, np.inf, -np.inf):
        broken = box.copy()
        broken[1, 2] = bad
        with pytest.raises(ValueError):
            nms(broken, prob)
    with pytest.raises(ValueError):
        nms(box, prob[:1])
    with pytest.raises(ValueError):
        nms(box, prob, class_idx=[1])
    with pytest.raises(ValueError):
        nms(box[:, :3], prob)
    assert nms(np.zeros((0, 4), F), np.zeros(0, F)) == []
    assert nms(np.zeros((0, 4), F), np.zeros(0, F), class_idx=np.zeros(0, np.int64), nms_kind="diounms") == []


def test_entry_points_refuse_an_unknown_kind_before_touching_a_gpu():
    from yolov3.pipeline import Pipeline
    from yolov3.inference import Detector
    net = object()                                                  # never reached
    with pytest.raises(ValueError):
        yolov3.inference(net, [np.zeros((8, 8, 3), np.uint8)], nms_kind="cornersnms")
    with pytest.raises(ValueError):
        yolov3.inference(net, [np.zeros((8, 8, 3), np.uint8)], nms_kind="diounms", beta_nms=0)
    with pytest.raises(ValueError):
        Pipeline(net, 1, nms_kind="cornersnms")
    with pytest.raises(ValueError):
        next(yolov3.detect_in_frames(net, [], nms_kind="cornersnms"))
    with pytest.raises(ValueError):
        yolov3.detect_in_images(net, os.path.join(ROOT, "tests", "golden", "images"), nms_kind="cornersnms")
    with pytest.raises(ValueError):
        yolov3.detect_in_cam(net, nms_kind="cornersnms")
    with pytest.raises(ValueError):
        Detector.run(object(), {}, None, 0.5, 0.45, nms_kind="cornersnms")


_CFG = """[net]
width=64
height=64
channels=3

[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=18
activation=linear

[yolo]
mask = 0,1,2
anchors = 10,14, 23,27, 37,58
classes=1
num=3
%s
"""


@pytest.mark.parametrize("keys,want", [
    ("", None),
    ("nms_kind=greedynms\nbeta_nms=0.6", ("greedynms", 0.6)),
    ("nms_kind=diounms\nbeta_nms=0.5", ("diounms", 0.5)),
    ("nms_kind=diounms", ("diounms", 0.6)),
    ("beta_nms=1", ("iou", 1.0)),
    ("nms_kind=cornersnms\nbeta_nms=0.6", ("cornersnms", 0.6)),
])
def test_nms_hint_reads_the_last_yolo_block(tmp_path, keys, want):
    path = tmp_path / "hint.cfg"
    path.write_text(_CFG % keys)
    net = yolov3.Darknet(str(path))
    assert net.nms_hint == want
    with pytest.raises(AttributeError):
        net.nms_hint = ("iou", 0.6)
    if want is not None and want[0] == "cornersnms":
        with pytest.raises(ValueError):                             # a hint whose use raises what any unknown kind does
            yolov3.inference(net, [np.zeros((64, 64, 3), np.uint8)], nms_kind=net.nms_hint[0], beta_nms=net.nms_hint[1])
    elif want is not None:
        assert _hip.nms_mode(*net.nms_hint)[0] == _hip.NMS_KINDS[want[0]]


def test_shipped_cfgs_give_no_hint_and_nothing_turns_the_mode_on():
    from golden_util import MODEL_DIR
    for name in ("yolov3", "yolov4", "yolov4-csp"):
        assert yolov3.Darknet(os.path.join(MODEL_DIR, name + ".cfg")).nms_hint is None
    import inspect
    for fn in (yolov3.inference, yolov3.detect_in_frames, yolov3.detect_in_images, yolov3.detect_in_video, yolov3.detect_in_cam):
        sig = inspect.signature(fn).parameters
        assert sig["nms_kind"].default is None and sig["beta_nms"].default == 0.6, fn
    from yolov3.pipeline import Pipeline
    from yolov3.inference import Detector
    for fn in (Pipeline.__init__, Detector.run):
        sig = inspect.signature(fn).parameters
        assert sig["nms_kind"].default is None and sig["beta_nms"].default == 0.6, fn
    sig = inspect.signature(yolov3.non_max_suppression_darknet).parameters
    assert (sig["thresh"].default, sig["nms_kind"].default, sig["beta_nms"].default) == (0.45, "iou", 0.6)


def test_cli_parser_accepts_the_two_flags():
    from yolov3.__main__ import build_parser
    base = ["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg"]
    args = build_parser().parse_args(base)
    assert args.nms_kind is None and args.beta_nms == 0.6
    args = build_parser().parse_args(base + ["--nms-kind", "diounms", "--beta-nms", "0.5", "--letterbox", "--darknet-pool"])
    assert (args.nms_kind, args.beta_nms, args.letterbox, args.darknet_pool) == ("diounms", 0.5, True, True)
    for kind in ("iou", "greedynms"):
        assert build_parser().parse_args(base + ["--nms-kind", kind]).nms_kind == kind
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--nms-kind", "cornersnms"])


# ---- the built device code ---------------------------------------------------------------------------------------------------
def test_code_object_holds_the_new_kernels_without_spills_or_more_lds():
    import code_object
    if not os.path.exists(code_object.LIB):
        pytest.skip("library not built")
    kern = [k for k in code_object.library_kernels() if "detect_kernel" in k[".name"]]
    by_name = {k[".name"]: k for k in kern}
    # detect_kernel<NMS_MODE, DK>: DK 0 = the reference's rule, 1 / 2 / 3 = Darknet's iou / greedynms / diounms
    base = {}
    for mode in ("0", "1"):
        for dk in "0123":
            name = [n for n in by_name if "detect_kernelILb%sELi%sEE" % (mode, dk) in n]
            assert len(name) == 1, (mode, dk, sorted(by_name))
            k = by_name[name[0]]
            assert k[".private_segment_fixed_size"] == 0, (name, "spills")
            assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128, name      # 16 waves of one workgroup on one CU
            if dk == "0":
                base[mode] = k[".group_segment_fixed_size"]
                assert base[mode] <= 64 * 1024
            assert k[".group_segment_fixed_size"] <= base[mode], name
