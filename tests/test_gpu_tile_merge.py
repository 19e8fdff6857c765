"""The seam merge on the GPU (-m gpu): ``y3_merge_tiled`` through ctypes on every case of tests/tile_merge_cases.py at its
thresholds against the restatement of tests/tile_merge_restate.py, and ``inference(tile_overlap=..., tile_merge=...)`` end to end
on tests/golden/cfg/mini.cfg against the restatement applied to what the unmerged call returns.

Everything is integers plus one float64 division, so every comparison is equality.  Every output lies between a fill and a guard:
slots past a frame's new count must keep the fill, the elements behind the capacity and around the workspace their guard; the
inputs must come back unchanged; the launch log must show one launch, of the merge kernel."""
import ctypes
import json

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.inference import _MergeBuffers, get_detector  # noqa: F401  (the stage's buffers: this module needs the feature)

import tile_merge_cases as C
import tile_merge_restate as M
from detect_util import dev
from golden_util import MODELS
from test_gpu_tiles import NET_H, NET_W, _frame, _mini

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = {torch.int32: -858993460, torch.int64: -3689348814741910324, torch.float32: -7.5}     # 0xCC.. patterns and a score no case has


def _guarded(shape, dtype, d):
    """A buffer of ``shape`` holding FILL, with GUARD elements of ones after it: (the whole allocation, the buffer)."""
    n = int(np.prod(shape))
    whole = torch.full((n + GUARD,), FILL[dtype], dtype=dtype, device=d)
    whole[n:] = 1
    return whole, whole[:n].view(shape)


class _Run(object):
    """One case on the device: inputs, outputs between fill and guard, and a workspace between canaries."""

    def __init__(self, case):
        d = dev()
        self.case = case
        self.host_in = (case.count, case.box, case.prob, case.cls, case.row)
        self.inputs = [torch.from_numpy(a.copy()).to(d) for a in self.host_in]
        B, cap = case.batch, case.capacity
        shapes = (((B,), torch.int32), ((B, cap, 4), torch.int64), ((B, cap), torch.float32), ((B, cap), torch.int64),
                  ((B, cap), torch.int32), ((B, cap), torch.int32))
        self.wholes, self.outs = zip(*[_guarded(s, t, d) for s, t in shapes])
        self.ws_bytes = _hip.lib().y3_merge_tiled_workspace_bytes(B, cap)
        assert self.ws_bytes > 0 and self.ws_bytes % 256 == 0
        self.ws_whole = torch.full((256 + self.ws_bytes + 256,), 0xA5, dtype=torch.uint8, device=d)

    def call(self, thr, members=True):
        c = self.case
        with _hip.launch_log() as log:
            _hip.check(_hip.lib().y3_merge_tiled(
                *[t.data_ptr() for t in self.inputs], c.batch, c.capacity, c.tile_rows, ctypes.c_double(thr),
                self.ws_whole.data_ptr() + 256, self.ws_bytes, *[t.data_ptr() for t in self.outs[:5]],
                self.outs[5].data_ptr() if members else None, _hip.stream_ptr()))
        torch.cuda.synchronize()
        assert len(log.names) == 1 and "tile_merge_kernel" in log.names[0], log.names
        return [w.clone() for w in self.wholes]

    def check(self, thr, members=True):
        c = self.case
        for whole in self.wholes:
            assert bool((whole[-GUARD:] == 1).all()), "a write past an output's capacity"
        ws = self.ws_whole.cpu().numpy()
        assert (ws[:256] == 0xA5).all() and (ws[-256:] == 0xA5).all(), "a write outside the workspace"
        for t, a in zip(self.inputs, self.host_in):
            assert np.array_equal(t.cpu().numpy().view(np.uint8), a.view(np.uint8)), "an input was written"
        count, box, prob, cls, row, mem = (t.cpu().numpy() for t in self.outs)
        frames = []
        for b in range(c.batch):
            want = C.expected(c, b, thr)
            n = int(count[b])
            assert n == len(want[4]), (c.name, b, n, len(want[4]))
            got = (box[b, :n], prob[b, :n], cls[b, :n], row[b, :n]) + ((mem[b, :n],) if members else ())
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g, w), (c.name, b)
            assert got[1].tobytes() == want[1].tobytes()
            # slots past the count keep their fill
            assert (box[b, n:] == FILL[torch.int64]).all() and (cls[b, n:] == FILL[torch.int64]).all()
            assert (prob[b, n:] == np.float32(FILL[torch.float32])).all() and (row[b, n:] == FILL[torch.int32]).all()
            assert (mem[b, n if members else 0:] == FILL[torch.int32]).all()
            frames.append(got)
        return frames


CALLS = [(c, thr) for c in C.CASES for thr in c.thrs]


@pytest.mark.parametrize("case,thr", CALLS, ids=["%s @ %r" % (c.name, thr) for c, thr in CALLS])
def test_merge_tiled_equals_the_restatement(case, thr):
    run = _Run(case)
    first = run.call(thr)
    run.check(thr)
    second = run.call(thr)                                     # the same buffers again: the same bits everywhere
    for a, b in zip(first, second):
        assert a.dtype == b.dtype and np.array_equal(a.cpu().numpy().view(np.uint8), b.cpu().numpy().view(np.uint8))


@pytest.mark.parametrize("name", ["batch tile_rows 500", "batch tile_rows 1000"])
def test_each_frame_alone_gives_what_it_gives_in_the_batch(name):
    case = C.BY_NAME[name]
    run = _Run(case)
    run.call(0.5)
    together = run.check(0.5)
    assert [len(f[3]) for f in together][:2] == [0, 1] and 1 < len(together[2][3]) < 300
    for b in range(case.batch):
        alone = _Run(case.alone(b))
        alone.call(0.5)
        count, box, prob, cls, row, mem = (t.cpu().numpy() for t in alone.outs)
        n = int(count[0])
        for g, w in zip((box[0, :n], prob[0, :n], cls[0, :n], row[0, :n], mem[0, :n]), together[b]):
            assert np.array_equal(g, w)


def test_threshold_one_copies_the_input_and_members_may_be_null():
    case = C.BY_NAME["random 101"]
    run = _Run(case)
    run.call(1.0, members=False)
    got = run.check(1.0, members=False)[0]
    for g, w in zip(got, case.frame(0)):
        assert np.array_equal(g, w)
    run2 = _Run(case)
    run2.call(0.5, members=False)
    assert len(run2.check(0.5, members=False)[0][3]) < 600


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def _tile_rows(net):
    return int(net.forward_frames(np.zeros((1, NET_H, NET_W, 3), np.uint8))["class_prob"].shape[1])


def _restate(frame, tile_rows, t):
    tlbr, prob, cls, rows = (np.asarray(a) for a in frame)
    o = M.merge(tlbr.tolist(), prob.tolist(), cls.tolist(), rows.tolist(), tile_rows, t)
    idx = [rows.tolist().index(r) for r in o[3]]
    return np.array(o[0], np.int64).reshape(-1, 4), prob[idx], np.array(o[2], np.int64), np.array(o[3]), np.array(o[4], np.int32)


@pytest.mark.parametrize("overview", [True, False])
@pytest.mark.parametrize("iou", [0.3, 1.0])
def test_inference_with_tile_merge_equals_the_restatement_on_the_unmerged_call(overview, iou):
    net = _mini()
    tile_rows = _tile_rows(net)
    image = _frame(100, 150, seed=250)
    kw = dict(device="cuda", prob_thresh=0.02, nms_iou_thresh=iou, return_rows=True, tile_overlap=0.25, tile_overview=overview)
    yolov3.inference(net, image, **kw)                          # (whatever a first call of this shape launches once is behind us)
    with _hip.launch_log() as before:
        plain = yolov3.inference(net, image, **kw)
    assert len(plain) == 1 and len(plain[0]) == 4 and len(plain[0][1]) > 0
    n_tiles = 17 if overview else 16
    assert int(np.asarray(plain[0][3]).max()) < n_tiles * tile_rows
    for t in (0.5, 1.0):
        with _hip.launch_log() as log:
            got = yolov3.inference(net, image, tile_merge=t, **kw)
        assert len(got) == 1 and len(got[0]) == 4
        want = _restate(plain[0], tile_rows, t)
        print("overview %s, iou %s, merge %s: %d -> %d detections" % (overview, iou, t, len(plain[0][1]), len(want[1])))
        for g, w in zip(got[0], want[:4]):
            assert np.array_equal(np.asarray(g), w)
        assert np.asarray(got[0][1]).tobytes() == want[1].tobytes()
        for g, p in zip(got[0], plain[0]):
            assert np.asarray(g).dtype == np.asarray(p).dtype
        det = get_detector(1, n_tiles * tile_rows, net._torch_device())
        assert np.array_equal(det.members[0, :len(want[4])].cpu().numpy(), want[4])
        # the merged call launches what the plain call launches, and the merge kernel after the detection tail
        merge = [i for i, n in enumerate(log.names) if "tile_merge_kernel" in n]
        assert len(merge) == 1 and "detect_kernel" in log.names[merge[0] - 1]
        assert [n for n in log.names if "tile_merge_kernel" not in n] == before.names
        if t == 1.0:
            assert len(want[1]) == len(plain[0][1])
        elif iou == 1.0:
            assert len(want[1]) < len(plain[0][1]), "nothing was merged: nothing was compared"
    # tile_merge=None after a merged call: the unmerged list bit for bit, from the same launches as before
    with _hip.launch_log() as after:
        again = yolov3.inference(net, image, tile_merge=None, **kw)
    for a, b in zip(again[0], plain[0]):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert after.names == before.names and not any("tile_merge" in n for n in after.names)
    assert det.members is None


def test_command_line_writes_the_merged_detections(tmp_path):
    from PIL import Image

    from yolov3.__main__ import main
    net = _mini()
    weights = str(tmp_path / "mini.weights")
    W.write_darknet_weights(weights, W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-8.0, calib=None))
    loaded = yolov3.Darknet(MODELS["mini"], device="cuda", dtype="float32").load_weights(weights).eval()
    folder = tmp_path / "images"
    folder.mkdir()
    image = _frame(70, 100, 5)
    Image.fromarray(image[:, :, ::-1]).save(str(folder / "a.png"))
    dump = tmp_path / "det.json"
    assert main(["-c", MODELS["mini"], "-w", weights, "-I", str(folder), "-p", "0.02", "-i", "1.0", "--tile-overlap", "0.25",
                 "--tile-merge", "0.5", "--batch-size", "4", "--json", str(dump)]) == 0
    with open(str(dump)) as fh:
        coco = json.load(fh)
    kw = dict(device="cuda", prob_thresh=0.02, nms_iou_thresh=1.0, tile_overlap=0.25, tile_batch=4)
    tlbr, prob, cls = yolov3.inference(loaded, image, tile_merge=0.5, **kw)[0]
    assert 0 < len(prob) < len(yolov3.inference(loaded, image, **kw)[0][1])
    got = sorted((a["category_id"], a["score"], tuple(a["bbox"])) for a in coco["annotations"])
    want = sorted((int(c), float(p), (int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])))
                  for b, p, c in zip(tlbr.tolist(), prob.tolist(), cls.tolist()))
    assert got == want
