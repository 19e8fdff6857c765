"""tests/golden/cfg/attention.cfg on the GPU (-m gpu): squeeze-and-excite units, spatial attention, an [avgpool] with two readers,
attention outputs that feed a shortcut, a route slice and a mish conv, a [sam] whose `from` lies inside a concat buffer.

Block by block, teacher-forced (every block recomputed on the CPU from the product's own inputs) against tests/attention_restate.py:
convs and shortcuts at one storage ulp in bf16 / fp16 and at the float32 gates of tests/test_gpu_yolov4.py; the attention blocks
bit for bit in every dtype, since their statement (include/yolov3_hip.h) is exact.  At batch 1 and 16 with ``keep_all=True``; then
with the arena on: the same kernels by name, outputs ``torch.equal`` to the keep-all run, twice on one plan; then once through
``inference()`` and once through ``detect_in_frames``."""
import os

import numpy as np
import pytest
import torch

import yolov3

import attention_restate as AR
import attention_util as AU
import plan_interp as PI
import test_gpu_yolov4 as T4
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu

CFG = os.path.join(GOLDEN, "cfg", "attention.cfg")
DTYPE = {"float32": "float32", "bf16": "bf16", "fp16": "fp16"}
EMULATE = {"float32": None, "bf16": "bf16", "fp16": "f16"}
F32_GATE = dict(rtol=1e-4, atol=T4.BOX_ATOL)          # test_gpu_yolov4.test_float32_matches_restatement's, on boxes; scores: SCORE_ATOL
_case = {}


def case(batch):
    if batch not in _case:
        _case[batch] = PI.synth_case(CFG, 64, 64, batch=batch)
    return _case[batch]


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def _attention_expected(kind, dtype, prev, src):
    """the exact statement on the product's own inputs: (B, C, H, W) float32 tensors of storage values -> the same"""
    if kind == "avgpool":
        want = AU.avgpool_ordered_expected(_nhwc(prev), dtype)
    else:
        want = AU.product_expected(_nhwc(src), _nhwc(prev), dtype)
    return torch.from_numpy(np.ascontiguousarray(want)).permute(0, 3, 1, 2).contiguous()


def _teacher_forced(dtype, batch, sel):
    c = case(batch)
    net = yolov3.Darknet(CFG, device="cuda", dtype=dtype, keep_all=True).set_params(c["params"]).eval()
    out = net.forward_frames(c["frames"])
    torch.cuda.synchronize()
    kernel_of = {}
    for r in net.plan_report():
        kernel_of.setdefault(r["block"], []).append(r["kernel"])
    ref = AR.Restatement(CFG, c["params"])
    emulate = EMULATE[dtype]
    rnd = T4.MODES[dtype]["rnd"] if emulate else (lambda t: t)
    x_in = c["x"][sel]

    def hip(i):
        return net.block_output(i)[sel].cpu()

    def close(got, want, what):
        if emulate:
            T4._close_bf16(got, want, what, None, dtype)
        else:
            np.testing.assert_allclose(got.numpy(), want.numpy(), err_msg=what, **F32_GATE)

    checked, logits = 0, None
    for i, blk in enumerate(ref.blocks):
        kind = blk["type"]
        what = "%s batch %d block %d (%s, %s)" % (dtype, batch, i, kind, ",".join(kernel_of.get(i, ["-"])))
        if kind == "convolutional":
            if i == 0 and (not emulate or kernel_of[0][0].startswith("conv_stem3x3")):
                y = ref.conv(0, x_in)                       # the VALU stem computes in float32 from the bytes and float32 weights
            else:
                y = ref.conv(i, rnd(x_in) if i == 0 else hip(i - 1), emulate)
            if ref.blocks[i + 1]["type"] == "yolo":
                logits = y
                continue
            close(hip(i), rnd(y), what)
        elif kind == "shortcut":
            close(hip(i), rnd(hip(i - 1) + hip(i + blk["from"])), what)
        elif kind == "route":
            assert torch.equal(hip(i), torch.cat([hip(j) for j in blk["layers"]], dim=1)), what
        elif kind in AR.KINDS:
            assert kernel_of[i] == ["%s_%s" % (kind, AU.TAG[dtype])], what
            src = None if kind == "avgpool" else hip(ref.src_of(i))
            want = _attention_expected(kind, dtype, hip(i - 1), src)
            assert AU.same_bits(hip(i).numpy(), want.numpy()).all(), what
            # and the float64 restatement, at one storage ulp (float32: the gate)
            close(hip(i), rnd(AR.attention_block(blk, hip(i - 1), src, torch.float64)), what + " against float64")
        elif kind == "yolo":
            box, prob, _ = ref.decode(i, logits)
            what = "%s batch %d head (%s)" % (dtype, batch, ",".join(kernel_of.get(i - 1, ["-"])))
            np.testing.assert_allclose(out["bbox_xywh"][sel].cpu().numpy(), box.numpy(), err_msg=what, **F32_GATE)
            np.testing.assert_allclose(out["class_prob"][sel].cpu().numpy(), prob.numpy(), err_msg=what, atol=T4.SCORE_ATOL)
        else:
            raise AssertionError(what)
        checked += 1
    return net, out, kernel_of, checked


@pytest.mark.parametrize("batch", [1, 16])
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_every_block_teacher_forced_then_the_arena_run_and_the_entry_points(dtype, batch):
    sel = [0] if batch == 1 else [0, 15]
    keep, out, kernel_of, checked = _teacher_forced(dtype, batch, sel)
    assert checked == 24, checked                          # every block but the head conv, which the decode stands for
    c = case(batch)
    # the arena on: slots reused as soon as their last reader has run
    net = yolov3.Darknet(CFG, device="cuda", dtype=dtype, fuse=False).set_params(c["params"]).eval()
    for _ in range(2):
        got = net.forward_frames(c["frames"])
        torch.cuda.synchronize()
        names = {}
        for r in net.plan_report():
            names.setdefault(r["block"], []).append(r["kernel"])
        assert names == kernel_of
        for key in ("bbox_xywh", "class_prob", "class_idx"):
            assert torch.equal(got[key], out[key]), (dtype, batch, key)
    assert net._last_plan.desc["arena_bytes"] < keep._last_plan.desc["arena_bytes"]
    if batch != 16:
        return
    # float32 forward against the restatement end to end, at test_gpu_yolov4's gates
    fwd = net.forward(c["x"])                              # the float32 tensor entry point, in every dtype
    assert torch.isfinite(fwd["class_prob"]).all() and fwd["class_prob"].shape == out["class_prob"].shape
    if dtype == "float32":
        want = AR.Restatement(CFG, c["params"]).forward(c["x"])
        for got in (out, fwd):
            np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=T4.BOX_ATOL)
            np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=T4.SCORE_ATOL)
    # once through inference() and once through detect_in_frames: the same detections frame by frame
    frames = list(c["frames"])
    single = yolov3.inference(net, frames, device="cuda", prob_thresh=0.05)
    streamed = list(yolov3.detect_in_frames(net, frames, batch_size=16, prob_thresh=0.05))
    assert len(single) == len(streamed) == 16 and sum(len(d[1]) for d in single) > 0
    for f in range(16):
        for a, b in zip(streamed[f], single[f]):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "frame %d" % f
