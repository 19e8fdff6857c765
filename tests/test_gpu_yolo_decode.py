"""The default soft-max decode on planted logits, in every compiled form (-m gpu).

One-op Y3_OP_YOLO plans through ``y3_op_run`` run every case of tests/yolo_decode_cases.py in the sequential float32 form and in
the four-lane form (generic class loop; 80-class register path) against the float64 restatement: classes equal with no exemption
(every box is a clear maximum or a planted exact tie: tests/test_yolo_decode_host.py), scores and boxes within the bounds of
tests/test_gpu_parity.py::test_yolo_decode_op_any_class_count, the rows outside the head untouched.  Then a head conv with zero
weights and a planted bias puts the same boxes through the tiled and the direct-weights fused head kernels at every fuse_head."""
import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

import darknet_scores_restate as S
import yolo_decode_cases as Y
from oracle import darknet_oracle as orc
from yolo_op_util import ANCHORS, prefill, yolo_op

pytestmark = pytest.mark.gpu

F = np.float32
# tests/test_gpu_parity.py::test_yolo_decode_op_any_class_count's bounds, against the float64 restatement (the oracle's own float32
# rounding uses a tenth of them: tests/test_yolo_decode_host.py)
SCORE_RTOL, SCORE_ATOL = 1e-5, 1e-8
BOX_RTOL, BOX_ATOL = 2e-6, 1e-7
# tests/test_gpu_parity.py::test_split_class_decode_matches_sequential_decode's bound: four lanes against the sequential loop
LANES_RTOL, LANES_ATOL = 2e-6, 1e-9
FORMS = (("sequential", _hip.Y3_F32), ("four lanes", _hip.Y3_BF16))


def _excess(got, want, atol):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    ok = np.isfinite(want) & (want != 0)
    return float(((np.abs(got[ok] - want[ok]) - atol) / np.abs(want[ok])).max()) if ok.any() else 0.0


def _check(label, box, prob, cls, want):
    wbox, wprob, wcls = want
    wrong = int((cls != wcls).sum())
    print("%s: %d of %d classes differ; score excess %.3g (rtol %g), box excess %.3g (rtol %g)" % (
        label, wrong, wcls.size, _excess(prob, wprob, SCORE_ATOL), SCORE_RTOL, _excess(box, wbox, BOX_ATOL), BOX_RTOL))
    assert prob.dtype == F and box.dtype == F and cls.dtype == np.int64
    assert wrong == 0, "%s: arg-max differs at rows %s" % (label, np.argwhere(cls != wcls)[:8].tolist())
    assert not np.isnan(prob).any() and not np.isnan(box).any(), label
    np.testing.assert_allclose(prob, wprob, rtol=SCORE_RTOL, atol=SCORE_ATOL, err_msg=label)
    assert np.array_equal(np.isinf(box), np.isinf(wbox)), label
    np.testing.assert_allclose(box, wbox, rtol=BOX_RTOL, atol=BOX_ATOL, err_msg=label)         # (inf equals inf of the same sign)


def _one_op(label, t, want, anchors, row_offset, rows_total, sxy):
    b, h, w, a, _ = t.shape
    rows = a * h * w
    head = slice(row_offset, row_offset + rows)
    outside = np.ones(rows_total, bool)
    outside[head] = False
    before = [v.numpy() for v in prefill(b, rows_total)]
    outs = {}
    for form, dtype in FORMS:
        rc, box, prob, cls = yolo_op(t, dtype, 0, anchors, row_offset, rows_total, None if sxy == 1.0 else sxy)
        assert rc == 0, _hip.lib().y3_last_error()
        for got, was in zip((box, prob, cls), before):
            assert got[:, outside].tobytes() == was[:, outside].tobytes(), "%s %s: a row outside the head changed" % (label, form)
        outs[form] = (box[:, head], prob[:, head], cls[:, head])
        _check("%s %s" % (label, form), *outs[form], want)
    (box4, prob4, cls4), (box1, prob1, cls1) = outs["four lanes"], outs["sequential"]
    assert box4.tobytes() == box1.tobytes(), "%s: the boxes of the two forms differ" % label
    assert np.array_equal(cls4, cls1)
    np.testing.assert_allclose(prob4, prob1, rtol=LANES_RTOL, atol=LANES_ATOL, err_msg=label)


# ---- a. one-op plans ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Y.CASE_NAMES)
def test_one_op_decode_equals_the_float64_restatement(name):
    c = Y.case(name)
    _one_op(name, c["t"], Y.want(c), c["anchors"], c["row_offset"], c["rows_total"], c["sxy"])


@pytest.mark.parametrize("classes", S.DECODE_CLASSES)
@pytest.mark.parametrize("grid", S.DECODE_GRIDS)
def test_one_op_decode_on_the_darknet_scores_inputs(grid, classes):
    """the flag-less run that tests/test_gpu_darknet_scores.py only uses as the baseline of its boxes"""
    t = S.decode_case(grid, classes)
    want = Y.softmax_decode64(t, ANCHORS, grid, (32.0 * grid[1], 32.0 * grid[0]))
    _one_op("darknet_scores %s x %d" % (grid, classes), t, want, ANCHORS, 0, 3 * grid[0] * grid[1], 1.0)


# ---- b. fused heads on planted logits -------------------------------------------------------------------------------------------
GRID, BATCH, HEAD_BLOCK = (5, 7), 3, 4           # 105 pixels: the last tile of 32, 48, 64 or 96 of them is ragged
# head: (case the boxes come from, channels in front of the head conv, scale_x_y, the sets of tests/yolo_decode_cases.py::head_boxes)
HEADS = {
    "coco_256": ("c80_a3_mid", 256, 1.0, range(8)),          # 3 x 85 = 255 channels; direct weights (fuse_head 2: tiled)
    "coco_128": ("c80_a3_mid", 128, 1.0, range(8)),          # the tiled head kernel at every fuse_head
    "a8_128": ("c27_a8", 128, 1.0, range(3)),                # 8 x 32 = 256 channels, eight anchors
    "a8_256_s12": ("c27_a8", 256, 1.2, range(3)),
    "small": ("c5_a8", 128, 1.0, range(3)),                  # 8 x 10 = 80 channels: the two kernels stay
}
HEAD_SETS = {"c80_a3_mid": 8, "c27_a8": 3, "c5_a8": 3}
HEAD_PARAMS = [(head, k) for head, spec in HEADS.items() for k in spec[3]]


def _conv(f, k, s=1, act="leaky", bn=True):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % (
        "batch_normalize=1\n" if bn else "", f, k, s, act)


def _head_cfg(mid, anchors, classes, sxy):
    na = len(anchors)
    return ("[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (8 * GRID[1], 8 * GRID[0]) + _conv(32, 3, 2) + _conv(64, 3, 2) +
            _conv(128, 3, 2) + _conv(mid, 1) + _conv(na * (5 + classes), 1, act="linear", bn=False) +
            "[yolo]\nmask=%s\nanchors=%s\nclasses=%d\nnum=%d\n%s" % (
                ",".join(str(k) for k in range(na)), ", ".join("%d,%d" % (aw, ah) for aw, ah in anchors), classes, na,
                "" if sxy == 1.0 else "scale_x_y=%g\n" % sxy))


def _run(net, frames, f32_input):
    out = net.forward(torch.from_numpy(orc.frames_to_input(list(frames)))) if f32_input else net.forward_frames(frames)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("head,which", HEAD_PARAMS)
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_fused_heads_on_planted_logits(tmp_path, dtype, head, which):
    case_name, mid, sxy, _ = HEADS[head]
    c = Y.case(case_name)
    anchors, n_attr = c["anchors"], c["t"].shape[-1]
    na, channels = len(anchors), len(anchors) * n_attr
    boxes = Y.head_boxes(case_name, HEAD_SETS[case_name])[which]
    bias = Y.head_bias(case_name, boxes)
    cfg = tmp_path / "head.cfg"
    cfg.write_text(_head_cfg(mid, anchors, n_attr - 5, sxy))
    blocks, net_info = parse_config(str(cfg))
    calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
    params = W.synth_params(blocks, net_info, seed=5, obj_bias=-1.0, calib=calib)
    assert params[-1]["weight"].shape[0] == channels and "bias" in params[-1]
    params[-1]["weight"] = np.zeros_like(params[-1]["weight"])
    params[-1]["bias"] = bias.copy()
    frames = synth_frames(17, BATCH, 8 * GRID[0], 8 * GRID[1])
    modes = (0,) if dtype == "float32" else (0, 1, 2, 3, 4)
    outs, names = {}, {}
    for fh in modes:
        net = yolov3.Darknet(str(cfg), device="cuda", dtype=dtype, keep_all=fh == 0, fuse=True,
                             options={"fuse_head": fh}).set_params(params).eval()
        outs[fh] = _run(net, frames, dtype == "float32")
        report = net.plan_report()
        names[fh] = report[-2]["kernel"]
        assert report[-1]["scores"] == "reference"
        if fh == 0:
            logits = net.block_output(HEAD_BLOCK).cpu().numpy()            # (B, C, h, w): the head conv's own float32 output
        del net
    # zero weights: the logits are the bias at every cell, exactly -- so the planted boxes are what the decode sees
    assert logits.shape == (BATCH, channels) + GRID
    assert np.array_equal(logits, np.broadcast_to(bias[None, :, None, None], logits.shape)), "the head conv's output is not its bias"
    # which kernels ran
    assert "head_decode" not in names[0], names
    if dtype != "float32":
        if channels <= 128:                                                # (the fused tile is 256 channels wide)
            assert not any("head_decode" in names[fh] for fh in modes), names
        elif mid == 128:
            assert all("conv_head_decode_" in names[fh] and "_dw_" not in names[fh] for fh in (1, 2, 3, 4)), names
        else:
            assert all("conv_head_decode_dw_" in names[fh] and names[fh].endswith("_48x256") for fh in (1, 3)), names
            assert "conv_head_decode_dw_" in names[4] and names[4].endswith("_96x256"), names
            assert "conv_head_decode_" in names[2] and "_dw_" not in names[2], names
    for fh in modes[1:]:
        for k in ("bbox_xywh", "class_prob", "class_idx"):
            assert outs[fh][k].tobytes() == outs[0][k].tobytes(), "%s fuse_head %d (%s): %s differs from the two-launch path" % (
                dtype, fh, names[fh], k)
    t = np.broadcast_to(bias.reshape(na, n_attr), (BATCH,) + GRID + (na, n_attr))
    want = Y.softmax_decode64(t, anchors, GRID, (8.0 * GRID[1], 8.0 * GRID[0]), sxy)
    _check("%s set %d %s (%s)" % (head, which, dtype, [str(c["recipe"][k]) for k in boxes]),
           outs[0]["bbox_xywh"], outs[0]["class_prob"], outs[0]["class_idx"], want)
