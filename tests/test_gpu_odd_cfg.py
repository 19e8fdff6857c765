"""One hand-written cfg off the shipped networks' path through ``Darknet`` (-m gpu): tests/golden/cfg/odd.cfg.

The one-op plans of tests/test_gpu_footprint.py do not pass through ``Darknet._device_weights``' layout for the direct fallback,
through the plan's padded pixel strides for channel counts off the 16-byte chunk, or through ``forward_frames`` on a stem that is
not 3 channels x 3x3.  This network does: one input channel, a 5x5 stride-2 stem, a 3x3 block without ``pad=``, a route whose
second member starts at channel 20 (off the 8-channel grain: the plan copies it), a 7x7, and a linear 1x1 head.  Batch 2.

* float32: every block against the oracle, tolerances of tests/test_gpu_parity.py::test_mini_every_block_fp32.
* bf16 / fp16: every block teacher-forced at one storage ulp (tests/test_gpu_bf16.py ``_close_bf16``), the head through the
  decode as tests/test_gpu_bf16.py ``_teacher_forced`` checks its heads.
* ``forward_frames(frames)`` == ``forward(frames_to_input(frames))`` bit for bit in float32.
"""
import os

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

from golden_util import GOLDEN
from test_gpu_bf16 import MODES, _close_bf16

pytestmark = pytest.mark.gpu

CFG = os.path.join(GOLDEN, "cfg", "odd.cfg")
TAG = {"float32": "f32", "bf16": "bf16", "fp16": "f16"}
STEM, PAD0, C20_24, ROUTE, K7, HEAD = 0, 1, 2, 3, 4, 5
_cache = {}


def _params():
    if "params" not in _cache:
        blocks, net_info = parse_config(CFG)
        calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
        _cache["params"] = W.synth_params(blocks, net_info, seed=0, obj_bias=-2.0, calib=calib)
    return _cache["params"]


def _frames():
    """(2, 48, 64, 1) uint8"""
    return np.ascontiguousarray(synth_frames(31, 2, 48, 64)[..., 1:2])


def _reference_f32():
    """the oracle's float32 forward (float64 accumulation), computed once and left unchanged: (outputs, {block: tensor})"""
    if "ref" not in _cache:
        blocks = {}
        x = torch.from_numpy(orc.frames_to_input(list(_frames())))
        out = orc.OracleDarknet(CFG).set_params(_params()).forward(x, collect=blocks, accumulate="f64")
        _cache["ref"] = (out, blocks)
    return _cache["ref"]


def _net(dtype):
    return yolov3.Darknet(CFG, device="cuda", dtype=dtype, keep_all=True, fuse=True).set_params(_params()).eval()


def _kernels(net, dtype):
    kernel_of = {}
    for r in net.plan_report():
        kernel_of.setdefault(r["block"], []).append(r["kernel"])
    print("odd.cfg %s: %s" % (dtype, {b: ",".join(k) for b, k in sorted(kernel_of.items())}))
    direct = "conv_direct_" + TAG[dtype]
    assert kernel_of[STEM] == [direct] and kernel_of[K7] == [direct], kernel_of
    if dtype != "float32":
        assert kernel_of[C20_24] == [direct], kernel_of
    return kernel_of


def test_float32_every_block():
    frames = _frames()
    assert frames.shape == (2, 48, 64, 1) and frames.dtype == np.uint8
    x = torch.from_numpy(orc.frames_to_input(list(frames)))
    net = _net("float32")
    out = net.forward(x)
    torch.cuda.synchronize()
    kernel_of = _kernels(net, "float32")
    want_out, want = _reference_f32()
    shapes = {STEM: (2, 12, 24, 32), PAD0: (2, 20, 22, 30), C20_24: (2, 24, 22, 30), ROUTE: (2, 44, 22, 30), K7: (2, 40, 22, 30),
              HEAD: (2, 18, 22, 30)}
    for i, shape in shapes.items():
        got = net.block_output(i).cpu().numpy()
        assert got.shape == shape, (i, got.shape)
        np.testing.assert_allclose(got, want[i].numpy(), rtol=1e-4, atol=2e-5, err_msg="block %d (%s)" % (i, kernel_of.get(i)))
    np.testing.assert_allclose(out["bbox_xywh"].cpu().numpy(), want_out["bbox_xywh"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out["class_prob"].cpu().numpy(), want_out["class_prob"].numpy(), rtol=1e-4, atol=1e-6)
    assert torch.equal(out["class_idx"].cpu(), want_out["class_idx"])


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_16bit_every_block_teacher_forced(mode):
    rnd, emulate = MODES[mode]["rnd"], MODES[mode]["emulate"]
    frames = _frames()
    net = _net(MODES[mode]["dtype"])
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    kernel_of = _kernels(net, mode)
    ref = orc.OracleDarknet(CFG).set_params(net._params)
    blocks = ref.blocks
    # the stem is conv_direct on the bytes: byte / 255 in float32 times the 16-bit weights, no rounding of the input
    x_net = torch.from_numpy(orc.frames_to_input(list(frames)))

    def hip(i):
        return x_net if i < 0 else net.block_output(i).cpu()

    checked = 0
    for i, blk in enumerate(blocks):
        what = "%s odd.cfg block %d (%s, %s)" % (mode, i, blk["type"], ",".join(kernel_of.get(i, ["-"])))
        if blk["type"] == "convolutional":
            k = blk["size"]
            pad = (k - 1) // 2 if "pad" in blk else 0
            y = orc.conv_block(hip(i - 1), ref.params[ref._conv_slot[i]], blk["stride"], pad, blk["activation"] == "leaky",
                               round_weights=emulate)
            if i == HEAD:
                # float32 logits: through the decode, as tests/test_gpu_bf16.py _teacher_forced checks its heads
                yb = blocks[i + 1]
                mask = yb["mask"] if isinstance(yb["mask"], list) else [yb["mask"]]
                box, prob, idx = orc.yolo_decode(y, [yb["anchors"][m] for m in mask])
                box[:, :, 2] /= ref.net_info["width"]
                box[:, :, 3] /= ref.net_info["height"]
                torch.testing.assert_close(out["bbox_xywh"].cpu(), box, rtol=2e-4, atol=2e-5, msg=lambda m: what + " boxes: " + m)
                torch.testing.assert_close(out["class_prob"].cpu(), prob, rtol=5e-4, atol=2e-5, msg=lambda m: what + " scores: " + m)
                assert torch.equal(out["class_idx"].cpu(), idx), what
            else:
                _close_bf16(hip(i), rnd(y), what, None, mode)
        elif blk["type"] == "route":
            assert torch.equal(hip(i), torch.cat([hip(j) for j in blk["layers"]], dim=1)), what
        else:
            assert blk["type"] == "yolo", what
            continue
        checked += 1
    assert checked == len(blocks) - 1 == 6


def test_float32_frames_match_float_input_bit_for_bit():
    frames = _frames()
    net = _net("float32")
    a = net.forward(torch.from_numpy(orc.frames_to_input(list(frames))))
    blocks_a = [net.block_output(i) for i in range(HEAD + 1)]
    b = net.forward_frames(frames)
    torch.cuda.synchronize()
    assert net.plan_report()[0]["kernel"] == "conv_direct_f32"
    for i, t in enumerate(blocks_a):
        assert torch.equal(t, net.block_output(i)), "block %d" % i
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(a[k], b[k]), k
