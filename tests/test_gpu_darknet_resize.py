"""Darknet's float preprocessing on the GPU (-m gpu): ``y3_preprocess_darknet_f32`` against the numpy restatement
(tests/darknet_resize_restate.py) bit for bit, its memory footprint on a mixed batch, ``inference(preprocess="darknet")`` end to
end on tests/golden/cfg/mini.cfg against the restatement's tensor fed to ``forward``, and the default path call for call."""
import os

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.inference import Detector
from yolov3.preprocess import darknet_frames_device
from yolov3.synthdata import synth_frames

import darknet_resize_restate as R
import footprint_util as fu
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu

MINI = os.path.join(GOLDEN, "cfg", "mini.cfg")

# source (h, w) -> network (net_h, net_w)
KERNEL_CASES = [
    ((1, 9), (8, 8)),                  # one source row
    ((9, 1), (8, 8)),                  # one source column
    ((5, 7), (9, 13)),                 # enlarging, odd sizes
    ((37, 23), (16, 24)),              # reducing
    ((16, 24), (16, 24)),              # net-sized: a copy
    ((100, 301), (64, 96)),            # wide
    ((301, 100), (96, 64)),            # tall
    ((50, 41), (33, 70)),              # a width that is no multiple of 4: 4-byte stores and their tail
    ((23, 61), (31, 33)),              # the same with an odd pixel count (the last lane's quad is partial)
]


def _device_equals_restatement(frames, net_h, net_w, letterbox):
    got, shapes = darknet_frames_device(frames, net_h, net_w, "cuda", letterbox)
    torch.cuda.synchronize()
    assert shapes == [tuple(f.shape) for f in frames]
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(frames), 3, net_h, net_w) and got.is_contiguous()
    want = torch.from_numpy(R.network_input(frames, net_h, net_w, letterbox))
    got = got.cpu()
    for i in range(len(frames)):
        assert torch.equal(got[i], want[i]), "frame %d %s into %dx%d, letterbox %s: %d values differ, max |d| %.3g" % (
            i, frames[i].shape, net_h, net_w, letterbox, int((got[i] != want[i]).sum()), float((got[i] - want[i]).abs().max()))
    return got


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("shape,net", KERNEL_CASES)
def test_kernel_equals_the_restatement_bit_for_bit(shape, net, letterbox):
    frame = R.random_frame(*shape, seed=shape[0] * 1000 + shape[1])
    got = _device_equals_restatement([frame], *net, letterbox)
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    if letterbox and R.geometry(*shape, *net)[:2] != net:
        assert (got == 0.5).any()


def test_last_row_quirk_on_the_device():
    """a size pair whose last row's sy rounds below h - 1: that row is (1 - dy) * part[h - 2], nearly black"""
    h, H = next((a, b) for a in range(2, 64) for b in range(2, 200)
                if a != b and np.float32(b - 1) * (np.float32(a - 1) / np.float32(b - 1)) < np.float32(a - 1))
    frame = np.full((h, 12, 3), 255, np.uint8)
    got = _device_equals_restatement([frame], H, 12, False)
    assert float(got[0, :, H - 1].max()) < 1e-3 and float(got[0, :, H - 2].min()) > 0.99


def test_more_frames_than_one_launch_takes_and_a_striding_grid():
    """70 frames: 64 descriptors per launch, and 33 tiles of 1024 pixels against 32 workgroups per frame"""
    rng = np.random.default_rng(5)
    frames = [R.random_frame(int(rng.integers(2, 60)), int(rng.integers(2, 60)), 200 + i) for i in range(70)]
    _device_equals_restatement(frames, 160, 208, True)


BATCH = [(40, 100), (90, 60), (33, 70), (7, 5)]


MIXED_NETS = [(33, 70), (32, 48)]


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("net", MIXED_NETS)
def test_mixed_batch_in_one_launch_stays_inside_its_output(net, letterbox):
    """four frames of different sizes, one call; the output lies between guards filled with a byte pattern and is itself
    pre-filled with NaN: the guards must stay as they are and no NaN may be left"""
    _hip.require_gpu()
    dev = torch.device("cuda:0")
    frames = [R.random_frame(h, w, seed=10 * h + w) for h, w in BATCH]
    n = len(frames) * 3 * net[0] * net[1]
    out = fu.flat("network input", "out", "float32", n)
    lay = fu.Layout([out])
    raw = torch.empty(lay.total + fu.ALIGN, dtype=torch.uint8, device=dev)
    shift = -raw.data_ptr() % fu.ALIGN
    alloc = raw[shift:shift + lay.total]
    fu.fill(alloc, lay, {}, poisoned=True)
    srcs = [torch.from_numpy(f).to(dev) for f in frames]
    descs = (_hip.Y3DarknetFrame * len(frames))(*[_hip.Y3DarknetFrame(s.data_ptr(), s.shape[0], s.shape[1]) for s in srcs])
    torch.cuda.synchronize()
    before = alloc.clone()
    assert bool(torch.isnan(fu.read_slice(before, out, 0, torch.float32)).all())
    import kernel_census as census
    del census.LAUNCHED[:]
    census.logged(lambda: _hip.check(_hip.lib().y3_preprocess_darknet_f32(descs, len(frames), out.ptr(alloc.data_ptr()), net[0], net[1],
                                                                       1 if letterbox else 0, None)))
    torch.cuda.synchronize()
    census.assert_census("y3_preprocess_darknet_f32")
    msg = fu.footprint_violations(before, alloc, lay)
    assert msg is None, msg
    got = fu.read_slice(alloc, out, 0, torch.float32).reshape(len(frames), 3, net[0], net[1]).cpu()
    assert not bool(torch.isnan(got).any()), "%d values of the output were never written" % int(torch.isnan(got).sum())
    for i, f in enumerate(frames):
        single, _ = darknet_frames_device([f], net[0], net[1], dev, letterbox)
        assert torch.equal(got[i], single[0].cpu()), "frame %d differs from its single-frame result" % i
    assert torch.equal(got, torch.from_numpy(R.network_input(frames, net[0], net[1], letterbox)))


# ---- end to end on mini.cfg ------------------------------------------------------------------------------------------------------
E2E_SHAPES = [(40, 100), (90, 60), (64, 64)]
E2E_THRESH, E2E_IOU = 0.3, 0.45
_NETS = {}


def _mini(dtype):
    """synthetic parameters whose scores depend on the image (seed chosen with the CPU oracle: every frame below has
    candidates scoring 0.7 .. 0.95 in both modes and both dtypes, far from the threshold)"""
    if dtype not in _NETS:
        blocks, net_info = parse_config(MINI)
        params = W.synth_params(blocks, net_info, seed=3, obj_bias=-1.0)
        _NETS[dtype] = yolov3.Darknet(MINI, device="cuda", dtype=dtype).set_params(params).eval()
    return _NETS[dtype]


def _frames(shapes):
    return [synth_frames(70 + k, 1, h, w)[0] for k, (h, w) in enumerate(shapes)]


def _same(a, b):
    assert len(a) == len(b)
    for f, (fa, fb) in enumerate(zip(a, b)):
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            assert np.array_equal(np.asarray(x), np.asarray(y)), "frame %d" % f


@pytest.mark.parametrize("letterbox", [False, True])
@pytest.mark.parametrize("dtype", ["float32", "bf16"])
def test_inference_equals_forward_on_the_restatements_tensor(dtype, letterbox):
    net = _mini(dtype)
    frames = _frames(E2E_SHAPES)
    got = yolov3.inference(net, frames, device="cuda", prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU, return_rows=True,
                           preprocess="darknet", letterbox=letterbox, letterbox_fill=7)      # (the fill byte plays no part)
    x = torch.from_numpy(R.network_input(frames, 32, 48, letterbox))
    out = net.forward(x)
    batch, rows = out["class_prob"].shape
    det = Detector(batch, rows, torch.device("cuda", torch.cuda.current_device()))
    det.run(out, np.asarray(E2E_SHAPES, np.int32), float(np.float32(E2E_THRESH)), E2E_IOU, letterbox=(32, 48) if letterbox else None)
    want = det.fetch(return_rows=True)
    _same(got, want)
    for f, d in enumerate(got):
        assert len(d[1]) >= 1, "frame %d kept no box: the comparison would be empty" % f
    # the streaming entry point runs the same batches
    streamed = list(yolov3.detect_in_frames(net, frames, batch_size=2, prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU,
                                            preprocess="darknet", letterbox=letterbox))
    _same(streamed, [d[:3] for d in got])
    if dtype == "float32":
        # the mode changes the answer on frames that are resized: the default 8-bit resize samples elsewhere
        plain = yolov3.inference(net, frames[:1], device="cuda", prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU,
                                 return_rows=True, letterbox=letterbox)
        assert not (len(plain[0][1]) == len(got[0][1]) and np.array_equal(plain[0][1], got[0][1]))


def test_net_sized_frames_give_the_default_modes_detections():
    """float32: resize_image copies a net-sized frame, so the network sees byte / 255 either way"""
    net = _mini("float32")
    frames = _frames([(32, 48)] * 3)
    for letterbox in (False, True):
        a = yolov3.inference(net, frames, device="cuda", prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU, return_rows=True,
                             preprocess="darknet", letterbox=letterbox)
        b = yolov3.inference(net, frames, device="cuda", prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU, return_rows=True,
                             letterbox=letterbox)
        assert all(len(d[1]) >= 1 for d in b)
        _same(a, b)


# ---- the default path --------------------------------------------------------------------------------------------------------------
class _Spy(object):
    """the loaded library with every entry point that is looked up written down"""
    QUIET = ("y3_capabilities", "y3_last_error", "y3_device_count", "y3_abi_version")

    def __init__(self, real):
        self._real, self.seen = real, []

    def __getattr__(self, name):
        if name not in self.QUIET:
            self.seen.append(name)
        return getattr(self._real, name)


def test_default_mode_makes_todays_calls(monkeypatch):
    net = _mini("float32")
    frames = _frames([(40, 100), (40, 100)])          # (the default resize wants one frame size per batch)
    kw = dict(device="cuda", prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU)
    warm = [yolov3.inference(net, frames, **kw), yolov3.inference(net, frames, letterbox=True, **kw),
            yolov3.inference(net, frames, preprocess="darknet", **kw)]       # plans and detector buffers exist from here on
    spy = _Spy(_hip.lib())
    monkeypatch.setattr(_hip, "lib", lambda: spy)

    def calls(**more):
        del spy.seen[:]
        result = yolov3.inference(net, frames, **dict(kw, **more))
        return list(spy.seen), result

    tail = ["y3_plan_run", "y3_detect", "y3_pack_records"]
    seen, result = calls()
    assert seen == ["y3_resize_bilinear_u8"] * 2 + tail
    _same(result, warm[0])
    seen, _ = calls(preprocess=None, letterbox_fill=3)
    assert seen == ["y3_resize_bilinear_u8"] * 2 + tail
    seen, result = calls(letterbox=True)
    assert seen == ["y3_letterbox_u8", "y3_plan_run", "y3_detect_letterbox", "y3_pack_records"]
    _same(result, warm[1])
    del spy.seen[:]
    sized = _frames([(32, 48)] * 2)                    # (the streaming loop takes net-sized frames of a non-square network)
    streamed = list(yolov3.detect_in_frames(net, sized, batch_size=2, prob_thresh=E2E_THRESH, nms_iou_thresh=E2E_IOU))
    assert "y3_plan_run" in spy.seen and "y3_preprocess_darknet_f32" not in spy.seen
    _same(streamed, yolov3.inference(net, sized, **kw))
    # ... and the mode itself: one preprocessing launch for the batch, then the same forward and tail
    seen, result = calls(preprocess="darknet")
    assert seen == ["y3_preprocess_darknet_f32"] + tail
    _same(result, warm[2])
    seen, _ = calls(preprocess="darknet", letterbox=True)
    assert seen == ["y3_preprocess_darknet_f32", "y3_plan_run", "y3_detect_letterbox", "y3_pack_records"]
