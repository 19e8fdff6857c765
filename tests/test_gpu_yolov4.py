"""YOLOv4 and YOLOv4-tiny on the GPU (-m gpu), with calibrated procedural weights, against the float32 CPU restatement of
mish, grouped routes and scale_x_y (tests/yolov4_restate.py):

* float32, batch 2: the forward outputs under the gates the YOLOv3 float32 tests use, then ``inference()`` on sample images
  against the oracle's post-processing of the restatement's outputs (kept rows, classes, scores);
* bf16 / fp16 at batch 16 (the plans the throughput path runs): every block, fed with the product's own input, at one storage
  ulp (test_gpu_bf16.py's teacher-forced gate) on the first and the last frame;
* yolov4-tiny through ``detect_in_frames`` at batch 16 equals ``inference()`` frame by frame.
"""
import os

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.preprocess import resize_bilinear_u8
from yolov3.synthdata import synth_frames

import yolov4_restate as R
from golden_util import MODEL_DIR, SAMPLE_IMAGES, load_jpeg_bgr
from test_gpu_bf16 import MODES, _close_bf16, _flip_slack
from test_gpu_parity import BOX_ATOL, SCORE_ATOL

pytestmark = pytest.mark.gpu

DIMS = {"yolov4-tiny": 416, "yolov4": 608}
OBJ_BIAS = -5.0


def _cfg(model):
    return os.path.join(MODEL_DIR, model + ".cfg")


def _params(model):
    blocks, net_info = parse_config(_cfg(model))
    return W.synth_params(blocks, net_info, seed=0, obj_bias=OBJ_BIAS, calib=W.load_calibration(model))


def _weights_path(model):
    """the procedural parameters as a Darknet .weights file (once per machine and user): the ordinary load_weights path"""
    cache = os.path.join(os.environ.get("TMPDIR", "/tmp"), "y3_golden_weights_%d" % os.getuid())
    os.makedirs(cache, exist_ok=True)
    path = os.path.join(cache, "%s_seed0_ob%g.weights" % (model, OBJ_BIAS))
    blocks, net_info = parse_config(_cfg(model))
    want = 20 + 4 * W.stream_length(blocks, net_info)
    if not (os.path.exists(path) and os.path.getsize(path) == want):
        tmp = path + ".%d.tmp" % os.getpid()
        W.write_darknet_weights(tmp, _params(model))
        os.replace(tmp, path)
    return path


def _net(model, dtype, **kw):
    return yolov3.Darknet(_cfg(model), device="cuda", dtype=dtype, **kw).load_weights(_weights_path(model)).eval()


def _frames(model, n, seed):
    dim = DIMS[model]
    frames = synth_frames(seed, n, dim, dim)
    frames[0] = resize_bilinear_u8(load_jpeg_bgr(SAMPLE_IMAGES[seed % len(SAMPLE_IMAGES)]), dim, dim)
    return frames


@pytest.mark.parametrize("model", ["yolov4-tiny", "yolov4"])
def test_float32_matches_restatement(model):
    net = _net(model, "float32")
    ref = R.Restatement(_cfg(model), net._params)
    frames = _frames(model, 2, 11)
    got = net.forward(R.frames_to_input(frames))
    want = ref.forward(R.frames_to_input(frames))
    np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=SCORE_ATOL)

    # inference() end to end on three sample images: the kept prediction rows agree with those the oracle's post-processing
    # keeps from the restatement's outputs, up to candidates the float32 forward deviation moves across a pixel, the
    # threshold or an IoU boundary (thresholds 0.2 / 0.3, one of the pairs the YOLOv3 golden lists use)
    dim = DIMS[model]
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES[:3]]
    resized = [resize_bilinear_u8(f, dim, dim) for f in images]
    res = yolov3.inference(net, images, device="cuda", prob_thresh=0.2, nms_iou_thresh=0.3, return_rows=True)
    rst = ref.forward(R.frames_to_input(resized))
    theirs = orc.postprocess(rst["bbox_xywh"].numpy(), rst["class_prob"].numpy(), rst["class_idx"].numpy(),
                             [f.shape for f in images], 0.2, 0.3, audit=True)
    kept = 0
    for f in range(len(images)):
        got_rows, want_rows = set(res[f][3].tolist()), set(theirs[f][3].tolist())
        union = got_rows | want_rows
        jac = len(got_rows & want_rows) / len(union) if union else 1.0
        kept += len(got_rows)
        print(model, "frame", f, "kept", len(got_rows), "restatement kept", len(want_rows), "jaccard %.3f" % jac)
        assert jac >= 0.9, (model, f, jac)
        g = {int(r): k for k, r in enumerate(res[f][3])}
        w = {int(r): k for k, r in enumerate(theirs[f][3])}
        same = sorted(set(g) & set(w))
        assert all(res[f][2][g[r]] == theirs[f][2][w[r]] for r in same), (model, f, "classes differ")
        np.testing.assert_allclose([res[f][1][g[r]] for r in same], [theirs[f][1][w[r]] for r in same], atol=SCORE_ATOL)
    assert kept > 0


def _teacher_forced(model, mode, batch, frames_checked):
    rnd, emulate = MODES[mode]["rnd"], MODES[mode]["emulate"]
    frames = _frames(model, batch, 21)
    net = _net(model, MODES[mode]["dtype"], keep_all=True, fuse=True)
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    report = net.plan_report()
    kernel_of = {}
    for r in report:
        kernel_of.setdefault(r["block"], []).append(r["kernel"])
    ref = R.Restatement(_cfg(model), net._params)
    blocks = ref.blocks
    rounds = ref.rounding_points()
    sel = list(frames_checked)
    x_net = rnd(R.frames_to_input([frames[j] for j in sel]))

    def hip(i):
        return x_net if i < 0 else net.block_output(i)[sel].cpu()

    def fused_away(i):
        return kernel_of.get(i, [""])[0].startswith("(fused")

    checked, heads = 0, []
    for i, blk in enumerate(blocks):
        kind = blk["type"]
        what = "%s %s block %d (%s, %s)" % (mode, model, i, kind, ",".join(kernel_of.get(i, ["-"])))
        if kind == "convolutional":
            if i + 1 < len(blocks) and fused_away(i + 1) and blocks[i + 1]["type"] == "convolutional":
                continue
            slack = None
            if fused_away(i) and blocks[i - 1]["type"] == "convolutional":
                mid = ref.conv(i - 1, hip(i - 2), emulate)
                x = rnd(mid)
                p2 = ref.params[ref.slot[i]]
                alpha2 = torch.from_numpy(p2["bn_gamma"] / np.sqrt(p2["bn_var"] + orc.BN_EPS))
                k = blk["size"]
                slack = _flip_slack(mid, rnd(torch.from_numpy(p2["weight"])), alpha2, blk["stride"],
                                    (k - 1) // 2 if "pad" in blk else 0, mode)
            elif i == 0 and kernel_of[0][0].startswith("conv_stem3x3"):
                # the VALU stem (a 3x3 stride-2 layer on the uint8 frames: yolov4-tiny) computes in float32 from the bytes
                # and float32 weights; only its output is stored in 16 bits
                y = ref.conv(0, R.frames_to_input([frames[j] for j in sel]))
                _close_bf16(hip(0), rnd(y), what, None, mode)
                checked += 1
                continue
            else:
                x = hip(i - 1)
            y = ref.conv(i, x, emulate)
            if i + 1 < len(blocks) and blocks[i + 1]["type"] == "yolo":
                heads.append((i + 1, y))
                continue
            if not rounds[i]:
                sc = i + 1
                _close_bf16(hip(sc), rnd(y + hip(sc + blocks[sc]["from"])), what + " + shortcut", slack, mode)
            else:
                _close_bf16(hip(i), rnd(y), what, slack, mode)
            checked += 1
        elif kind == "shortcut":
            if rounds[i - 1]:
                _close_bf16(hip(i), rnd(hip(i - 1) + hip(i + blk["from"])), what, None, mode)
                checked += 1
        elif kind == "maxpool":
            assert torch.equal(hip(i), orc.maxpool(hip(i - 1), blk["size"], blk["stride"])), what
            checked += 1
        elif kind == "upsample":
            assert torch.equal(hip(i), orc.upsample(hip(i - 1), blk["stride"])), what
            checked += 1
        elif kind == "route":
            assert torch.equal(hip(i), R.route({j: hip(j) for j in blk["layers"]}, blk)), what
            checked += 1
    bb, pr, ci = out["bbox_xywh"][sel].cpu(), out["class_prob"][sel].cpu(), out["class_idx"][sel].cpu()
    row = 0
    for yi, logits in heads:
        box, prob, idx = ref.decode(yi, logits)
        n = prob.shape[1]
        what = "%s %s head at block %d (%s)" % (mode, model, yi, ",".join(kernel_of.get(yi - 1, ["-"])))
        torch.testing.assert_close(bb[:, row:row + n], box, rtol=2e-4, atol=2e-5, msg=lambda m: what + " boxes: " + m)
        torch.testing.assert_close(pr[:, row:row + n], prob, rtol=5e-4, atol=2e-5, msg=lambda m: what + " scores: " + m)
        na = len(R.mask_of(blocks[yi]))
        top2 = torch.softmax(logits.reshape(logits.shape[0], na, -1, logits.shape[2], logits.shape[3])[:, :, 5:], dim=2)
        top2 = torch.topk(top2, 2, dim=2).values
        margin = (top2[:, :, 0] - top2[:, :, 1]).reshape(logits.shape[0], -1)
        assert int(((ci[:, row:row + n] != idx) & (margin > 1e-3)).sum()) == 0, what + ": arg-max flips on clear margins"
        row += n
        checked += 1
    assert row == pr.shape[1]
    return checked, kernel_of


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["yolov4-tiny", "yolov4"])
def test_16bit_every_block_teacher_forced_batch16(model, mode):
    checked, kernel_of = _teacher_forced(model, mode, 16, (0, 15))
    print(mode, model, "blocks checked", checked, sorted({k[0] for k in kernel_of.values()}))
    assert checked >= (30 if model == "yolov4-tiny" else 130)


def test_detect_in_frames_tiny_batch16_equals_inference():
    net = _net("yolov4-tiny", "bf16")
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES] * 2           # 18 frames: a full batch and a partial one
    streamed = list(yolov3.detect_in_frames(net, images, batch_size=16))
    assert len(streamed) == len(images)
    for f, img in enumerate(images):
        one = yolov3.inference(net, img, device="cuda")[0]
        for a, b in zip(streamed[f], one):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "frame %d" % f
