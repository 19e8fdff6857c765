"""Callers of the hot path: COCO export, id matching, box drawing, file
listing, command line.  CPU tests pin the host logic against vectors produced by the reference
(tests/golden/coco_export.json, tools/make_goldens.py g9); the GPU tests check that the batched
loops return exactly what per-frame ``inference()`` returns."""
import copy
import json
import os

import numpy as np
import pytest

import yolov3
from yolov3 import stream
from yolov3.__main__ import build_parser, main as cli_main
from yolov3.devtools import coco_util

from yolov3.synthdata import synth_frames

from golden_util import GOLDEN, MODELS, golden_weights_path, load_jpeg_bgr


def _coco_case():
    with open(os.path.join(GOLDEN, "coco_export.json")) as fh:
        g = json.load(fh)
    output = [[np.array(b, dtype=np.int64).reshape(-1, 4), np.array(p, dtype=np.uint32).view(np.float32),
               np.array(c, dtype=np.int64)] for b, p, c in g["inference_output"]]
    return g, output


def test_to_coco_matches_reference():
    g, output = _coco_case()
    got = yolov3.to_coco(g["image_filenames"], output, g["class_names"])
    assert got == g["to_coco"]
    json.dumps(got)   # plain Python numbers only


def test_match_ids_matches_reference():
    g, output = _coco_case()
    dataset = yolov3.to_coco(g["image_filenames"], output, g["class_names"])
    coco_util.match_ids(dataset, copy.deepcopy(g["reference_dataset"]))
    assert dataset == g["match_ids"]
    with pytest.raises(KeyError):
        bad = copy.deepcopy(g["reference_dataset"])
        bad["images"].append({"file_name": "missing.jpg", "id": 1, "height": 1, "width": 1})
        coco_util.match_ids(yolov3.to_coco(g["image_filenames"], output, g["class_names"]), bad)


def test_draw_boxes_outlines_and_clipping():
    img = np.zeros((40, 60, 3), dtype=np.uint8)
    boxes = np.array([[10, 8, 30, 20], [-5, -5, 70, 50]], dtype=np.int64)      # second one leaves the image
    out = yolov3.draw_boxes(img, boxes)
    assert out is img
    assert (img[8, 10:31] == (0, 255, 0)).all() and (img[20, 10:31] == (0, 255, 0)).all()
    assert (img[8:21, 10] == (0, 255, 0)).all() and (img[8:21, 30] == (0, 255, 0)).all()
    assert (img[14, 20] == 0).all()                                            # interior untouched
    # per-class colours + labels: no exception, label patch drawn inside the image
    img2 = np.zeros((64, 64, 3), dtype=np.uint8)
    yolov3.draw_boxes(img2, boxes[:1], class_prob=np.array([0.5]), class_idx=np.array([1]), class_names=["a", "b"])
    assert img2.any()
    assert len(set(stream.unique_colors(5))) == 5


def test_list_image_files_sorted_and_filtered(tmp_path):
    for name in ("b.jpg", "a.png", "notes.txt", "c.JPG"):
        (tmp_path / name).write_bytes(b"x")
    directory, names = stream.list_image_files(tmp_path)
    assert directory == str(tmp_path) and names == ["a.png", "b.jpg", "c.JPG"]
    directory, names = stream.list_image_files(tmp_path / "b.jpg")
    assert directory == str(tmp_path) and names == ["b.jpg"]


def test_cli_flags_mirror_the_reference():
    p = build_parser()
    a = p.parse_args(["-V", "v.mp4", "-c", "m.cfg", "-w", "m.weights", "-i", "0.4", "-p", "0.2", "-n", "names.txt",
                      "-o", "out", "--show-fps", "-v"])
    assert a.iou_thresh == 0.4 and a.prob_thresh == 0.2 and a.device == "cuda" and a.show_fps and a.verbose
    assert p.parse_args(["-C", "-c", "m.cfg", "-w", "w"]).cam == 0           # bare -C: device 0
    with pytest.raises(SystemExit):
        p.parse_args(["-c", "m.cfg", "-w", "w"])                              # an input source is required
    with pytest.raises(SystemExit):
        p.parse_args(["-I", "a", "-V", "b", "-c", "m.cfg", "-w", "w"])        # ... and exactly one
    with pytest.raises(SystemExit):
        cli_main(["-I", "a", "-c", "m.cfg", "-w", "w", "-d", "cpu"])          # no CPU path: refused loudly


def test_video_and_camera_need_opencv_and_say_so(tmp_path):
    if stream._cv2() is not None:
        pytest.skip("OpenCV present")
    clip = tmp_path / "clip.mp4"
    clip.write_bytes(b"\x00\x00\x00\x18ftypmp42" + b"\x00" * 64)
    with pytest.raises(ValueError, match="OpenCV"):         # an .mp4 needs a codec library; .avi (MJPEG) / .y4m do not
        list(stream._video_frames(str(clip)))
    with pytest.raises(RuntimeError, match="OpenCV"):
        stream.detect_in_cam(None)


# ------------------------------------------------------------------- the frame loop's own bookkeeping, on a recording pipeline
# detect_in_frames with yolov3.pipeline.Pipeline replaced by a stub that records what it is asked to do and whose ``results``
# return the ids of the frames it was given (a frame's id is its byte [0, 0, 0]), so the generator's grouping, draining, buffer
# rotation and clean-up run without a GPU.  The same cases on the real pipeline: tests/test_gpu_frame_loop.py.
class _FakeNet(object):
    def __init__(self, height=4, width=6):
        self.net_info = {"height": height, "width": width}
        self.device, self.dtype = "cuda", "float32"

    def _torch_device(self):
        return None


def _frame(i, h=4, w=6):
    f = np.zeros((h, w, 3), dtype=np.uint8)
    f[0, 0, 0] = i
    return f


@pytest.fixture
def loop(monkeypatch):
    """Patches the frame loop onto the recording stub.  ``loop.made``: the stubs built, in order; ``loop.staged``: weak
    references to the device batches the (patched) device path returned."""
    import types
    import weakref
    import torch
    from yolov3 import _hip, pipeline

    rec = types.SimpleNamespace(made=[], staged=[])

    class StubPipeline(object):
        def __init__(self, net, batch, height=None, width=None, in_flight=3, kmax=512, label_capacity=None):
            self.batch, self.height, self.width, self.in_flight = batch, height, width, in_flight
            self.max_open = self.nbuf = 2 * in_flight
            self.busy = False
            self._n = 0
            self.log = []             # ("submit", ticket, ids, path, pinned buffer) / ("results", ticket) / ("synchronize",)
            self._host = {}
            self._given = {}
            rec.made.append(self)

        def host_frames(self, j):
            assert 0 <= j < self.nbuf
            if j not in self._host:
                self._host[j] = torch.zeros((self.batch, self.height, self.width, 3), dtype=torch.uint8)
            return self._host[j]

        def upload_done(self, j, wait=True):
            self.log.append(("upload_done", j))
            return True

        def next_slot(self):
            return None, self._n % self.max_open

        def submit(self, frames, orig_hw=None, n_frames=None, letterbox=False):
            assert self.busy, "a pipeline is used by the generator that marked it busy"
            assert tuple(frames.shape) == (self.batch, self.height, self.width, 3)
            buf = [j for j, h in self._host.items() if h is frames]
            path = "pinned" if buf else ("device" if orig_hw is not None else "whole")
            ids = [int(f[0, 0, 0]) for f in frames[:n_frames]]
            self._given[self._n] = ids
            self.log.append(("submit", self._n, ids, path, buf[0] if buf else None))
            self._n += 1
            return self._n - 1

        def results(self, ticket):
            assert self._n - self.max_open <= ticket < self._n, "ticket {} is not open".format(ticket)
            self.log.append(("results", ticket))
            return list(self._given[ticket])

        def synchronize(self):
            self.log.append(("synchronize",))

        def events(self, *kinds):
            return [e for e in self.log if e[0] in kinds]

    def frames_on_device(frames, height, width, dev, stream, resize, letterbox, letterbox_fill):
        same = letterbox or all(tuple(f.shape[:2]) == (height, width) for f in frames)
        h, w = (height, width) if same else (width, height)          # preprocess.reference_dsize
        out = torch.zeros((len(frames), h, w, 3), dtype=torch.uint8)
        for i, f in enumerate(frames):
            out[i, 0, 0, 0] = int(f[0, 0, 0])
        rec.staged.append(weakref.ref(out))
        return out, [tuple(f.shape) for f in frames]

    monkeypatch.setattr(pipeline, "Pipeline", StubPipeline)
    monkeypatch.setattr(_hip, "require_gpu", lambda: None)
    monkeypatch.setattr(stream, "_frames_on_device", frames_on_device)
    return rec


def test_frame_loop_groups_frames_and_flushes_before_a_whole_batch(loop):
    """Single frames are grouped into batches of ``batch_size``; a pending group is flushed (short) before a whole
    (B, H, W, 3) item, which is submitted as it is when it fills the pipeline and staged when it is a short last batch."""
    net = _FakeNet()
    items = [_frame(0), _frame(1), _frame(2), np.stack([_frame(3), _frame(4)]), _frame(5), _frame(6),
             np.stack([_frame(7)])]
    assert list(stream.detect_in_frames(net, iter(items), batch_size=2, in_flight=3)) == list(range(8))
    pipe, = loop.made
    assert (pipe.batch, pipe.height, pipe.width, pipe.in_flight) == (2, 4, 6, 3)
    assert [e[1:] for e in pipe.events("submit")] == [(0, [0, 1], "pinned", 0), (1, [2], "pinned", 1), (2, [3, 4], "whole", None),
                                                      (3, [5, 6], "pinned", 2), (4, [7], "pinned", 3)]
    assert loop.staged == []


def test_frame_loop_refuses_a_batch_larger_than_its_pipeline(loop):
    net = _FakeNet()
    items = [_frame(0), _frame(1), np.stack([_frame(2), _frame(3), _frame(4)])]
    gen = stream.detect_in_frames(net, items, batch_size=2, in_flight=1)
    with pytest.raises(ValueError, match="a batch of 3 frames after the pipeline was sized for 2"):
        list(gen)
    pipe, = loop.made
    assert [e[2] for e in pipe.events("submit")] == [[0, 1]]
    assert not pipe.busy and len(pipe.events("synchronize")) == 1


def test_frame_loop_drains_the_oldest_ticket_first_and_all_at_the_end(loop):
    """With ``max_open`` tickets open the oldest one's results are taken before the next submit (which reuses its buffers);
    what is open at the end of the iterable is drained in order."""
    net = _FakeNet()
    assert list(stream.detect_in_frames(net, [_frame(i) for i in range(5)], batch_size=1, in_flight=1)) == list(range(5))
    pipe, = loop.made
    assert pipe.max_open == 2
    assert [e[:2] for e in pipe.events("submit", "results", "synchronize")] == [
        ("submit", 0), ("submit", 1), ("results", 0), ("submit", 2), ("results", 1), ("submit", 3), ("results", 2), ("submit", 4),
        ("results", 3), ("results", 4), ("synchronize",)]
    assert not pipe.busy


def _abandon(how, net):
    """One generator over 8 one-frame batches at ``in_flight=1``, left in the way ``how`` names."""
    import gc

    def source():
        for i in range(8):
            if how == "iterable raises" and i == 2:
                raise KeyError("decoder")
            yield _frame(i)

    gen = stream.detect_in_frames(net, source(), batch_size=1, in_flight=1)
    if how == "exhausted":
        assert list(gen) == list(range(8))
    elif how == "iterable raises":
        with pytest.raises(KeyError):
            list(gen)
    else:
        assert next(gen) == 0                                  # tickets 0 and 1 were submitted; 1 is still open
        if how == "close":
            gen.close()
        elif how == "throw":
            with pytest.raises(ZeroDivisionError):
                gen.throw(ZeroDivisionError("consumer"))
        elif how == "dropped":
            del gen
            gc.collect()


@pytest.mark.parametrize("how", ["exhausted", "close", "iterable raises", "throw", "dropped"])
def test_frame_loop_leaves_its_pipeline_idle_on_every_exit_path(loop, how):
    """However the generator ends, it synchronises its pipeline once and clears ``busy``; the next call gets the same
    pipeline from the cache."""
    net = _FakeNet()
    _abandon(how, net)
    pipe, = loop.made
    assert not pipe.busy and len(pipe.events("synchronize")) == 1 and pipe.log[-1] == ("synchronize",)
    assert list(net._pipelines.values()) == [pipe]
    before = pipe._n
    assert list(stream.detect_in_frames(net, [_frame(9), _frame(10)], batch_size=1, in_flight=1)) == [9, 10]
    assert loop.made == [pipe] and pipe._n == before + 2 and not pipe.busy and len(pipe.events("synchronize")) == 2


def test_a_busy_cached_pipeline_is_not_handed_out_twice(loop):
    net = _FakeNet()
    a = stream.detect_in_frames(net, [_frame(i) for i in range(4)], batch_size=1, in_flight=1)
    b = stream.detect_in_frames(net, [_frame(i) for i in range(10, 14)], batch_size=1, in_flight=1)
    assert next(a) == 0 and next(b) == 10
    first, second = loop.made
    assert first is not second and first.busy and second.busy
    assert list(net._pipelines.values()) == [first]             # the cache keeps the pipeline it had
    assert [next(a), next(b), next(a), next(b)] == [1, 11, 2, 12]
    assert list(a) == [3] and list(b) == [13]
    assert [e[2] for e in first.events("submit")] == [[0], [1], [2], [3]]
    assert [e[2] for e in second.events("submit")] == [[10], [11], [12], [13]]
    assert not first.busy and not second.busy and list(net._pipelines.values()) == [first]
    assert list(stream.detect_in_frames(net, [_frame(20)], batch_size=1, in_flight=1)) == [20]
    assert loop.made == [first, second] and first._n == 5
    # another cache key (batch size, in_flight) is another pipeline
    assert list(stream.detect_in_frames(net, [_frame(21)], batch_size=1, in_flight=2)) == [21]
    assert len(loop.made) == 3 and len(net._pipelines) == 2


def test_pinned_buffers_rotate_by_the_calls_own_count_not_by_ticket(loop):
    """Batches alternate between the pinned path and the device path.  The pinned batches take the pinned buffers 0, 1, 2, ...
    in turn, so that the one refilled is always the one whose upload is oldest and all ``nbuf`` are in use -- indexed by ticket
    they would take every other buffer here and wait for an upload two batches back instead of four.  The count starts again
    with every call; the tickets go on."""
    net = _FakeNet()

    def mixed(first):
        return [_frame(first + i) if i % 2 == 0 else _frame(first + i, 5, 7) for i in range(10)]

    for call, first in enumerate((0, 100)):
        assert list(stream.detect_in_frames(net, mixed(first), batch_size=1, in_flight=1, letterbox=True)) == list(range(first, first + 10))
        pipe, = loop.made
        submits = pipe.events("submit")[10 * call:]
        assert [e[1] for e in submits] == list(range(10 * call, 10 * call + 10))
        assert [e[3] for e in submits] == ["pinned", "device"] * 5
        assert [e[4] for e in submits if e[3] == "pinned"] == [0, 1, 0, 1, 0]       # nbuf = 2
        waits = [e[1] for e in pipe.events("upload_done")][5 * call:]
        assert waits == [0, 1, 0, 1, 0]                          # asked before each refill, for that buffer


def test_device_frames_stay_alive_while_their_ticket_is_open(loop):
    """The batch the device path made is referenced by nothing on the host once it is submitted, except by the generator:
    until the ticket's slot comes round again its memory must not go back to the allocator under the forward that reads it."""
    import gc
    net = _FakeNet()
    gen = stream.detect_in_frames(net, [_frame(i, 5, 7) for i in range(6)], batch_size=1, in_flight=1, letterbox=True)
    assert next(gen) == 0                                       # tickets 0 and 1 submitted
    gc.collect()
    assert len(loop.staged) == 2 and all(ref() is not None for ref in loop.staged)
    assert next(gen) == 1                                       # ticket 2 took the slot of ticket 0
    gc.collect()
    assert len(loop.staged) == 3 and loop.staged[0]() is None and loop.staged[1]() is not None and loop.staged[2]() is not None
    assert list(gen) == [2, 3, 4, 5]


def test_stretched_frames_of_a_network_that_is_not_square_get_a_pipeline_of_their_size(loop):
    """``inference()`` runs the frames it stretches at ``preprocess.reference_dsize`` -- width x height, the reference's
    ``cv2.resize`` quirk -- and net-sized ones at height x width: the loop keeps one pipeline per size and the order of the
    results; letterboxed frames are net-sized."""
    net = _FakeNet(4, 6)
    items = [_frame(0), _frame(1, 5, 7), _frame(2, 9, 3), _frame(3)]
    assert list(stream.detect_in_frames(net, items, batch_size=1, in_flight=1)) == [0, 1, 2, 3]
    own, turned = loop.made
    assert (own.height, own.width) == (4, 6) and (turned.height, turned.width) == (6, 4)
    assert [e[2:4] for e in own.events("submit")] == [([0], "pinned"), ([3], "pinned")]
    assert [e[2:4] for e in turned.events("submit")] == [([1], "device"), ([2], "device")]
    assert all(not p.busy and len(p.events("synchronize")) == 1 for p in loop.made) and len(net._pipelines) == 2
    assert list(stream.detect_in_frames(net, items, batch_size=1, in_flight=1, letterbox=True)) == [0, 1, 2, 3]
    assert len(loop.made) == 2 and len(own.events("submit")) == 6


def test_resize_false_refuses_the_first_frame_of_another_size(loop):
    """``resize=False``: the loop runs at the network's size only.  The first frame (or whole batch) of another size is a
    ValueError that names both sizes and where such frames do run; nothing of that frame's batch reaches the pipeline."""
    net = _FakeNet()
    with pytest.raises(ValueError, match=r"5 x 7.*4 x 6.*inference\(resize=False\)"):
        list(stream.detect_in_frames(net, [_frame(0, 5, 7)], batch_size=2, resize=False))
    assert loop.made == [] and loop.staged == []
    frames = [_frame(0), _frame(1), _frame(2), _frame(3, 5, 7), _frame(4)]
    gen = stream.detect_in_frames(net, frames, batch_size=2, in_flight=1, resize=False)
    with pytest.raises(ValueError, match=r"5 x 7.*4 x 6.*inference\(resize=False\)"):
        list(gen)
    pipe, = loop.made
    assert [e[2] for e in pipe.events("submit")] == [[0, 1]] and loop.staged == []      # frame 2 waited for its group
    assert not pipe.busy and len(pipe.events("synchronize")) == 1
    with pytest.raises(ValueError, match=r"5 x 7.*4 x 6.*inference\(resize=False\)"):
        list(stream.detect_in_frames(net, [np.stack([_frame(0, 5, 7)] * 2)], batch_size=2, in_flight=1, resize=False))
    assert list(stream.detect_in_frames(net, [_frame(5), _frame(6)], batch_size=2, in_flight=1, resize=False)) == [5, 6]


# ---------------------------------------------------------------------------------------------- GPU
IMAGES = ["000000000785.jpg", "000000017627.jpg", "000000024919.jpg", "000000035279.jpg", "000000037777.jpg"]


def _net(dtype="float32"):
    net = yolov3.Darknet(MODELS["yolov3-tiny"], device="cuda", dtype=dtype)
    net.load_weights(golden_weights_path("yolov3-tiny"))
    return net.eval()


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
def test_batched_frame_loop_equals_per_frame_inference():
    names = sorted(n for n in os.listdir(os.path.join(GOLDEN, "images")) if n.endswith(".jpg"))
    frames = [load_jpeg_bgr(n) for n in names]          # different sizes: resized on the GPU per frame
    net = _net()
    want = [yolov3.inference(net, f, prob_thresh=0.2, nms_iou_thresh=0.3)[0] for f in frames]
    for batch_size, in_flight in ((4, 2), (2, 3), (16, 1), (1, 2)):
        got = list(yolov3.detect_in_frames(net, iter(frames), batch_size=batch_size, prob_thresh=0.2,
                                           nms_iou_thresh=0.3, in_flight=in_flight))
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert _same(g, w), (batch_size, in_flight)
    assert list(yolov3.detect_in_frames(net, [], batch_size=4)) == []


@pytest.mark.gpu
def test_video_loop_over_a_frame_directory_and_cli(tmp_path):
    img_dir = os.path.join(GOLDEN, "images")
    net = _net()
    collected = []
    results = yolov3.detect_in_video(net, img_dir, prob_thresh=0.2, frames=collected, batch_size=4)
    names_sorted = stream.list_image_files(img_dir)[1]
    assert len(results) == len(names_sorted) == len(collected)
    first = yolov3.inference(net, load_jpeg_bgr(names_sorted[0]), prob_thresh=0.2)[0]
    assert _same(results[0], first)
    assert collected[0].shape == load_jpeg_bgr(names_sorted[0]).shape

    out_json, out_dir = tmp_path / "det.json", tmp_path / "frames"
    rc = cli_main(["-I", img_dir, "-c", MODELS["yolov3-tiny"], "-w", golden_weights_path("yolov3-tiny"), "-p", "0.2",
                   "--dtype", "float32", "-b", "4", "--json", str(out_json), "-o", str(out_dir)])
    assert rc == 0
    with open(out_json) as fh:
        ds = json.load(fh)
    assert [im["file_name"] for im in ds["images"]] == names_sorted
    assert len(ds["annotations"]) == sum(len(r[1]) for r in results)
    assert len(os.listdir(out_dir)) == len(names_sorted)


def _check_dump(dump, d, n_frames):
    """The arrays `bench.py --dump-outputs` wrote: the detections of one batch, as the JSON line lists them.  Returns the
    number of detections."""
    arrays = {name: np.load(os.path.join(dump, name + ".npy")) for name in d["dump_outputs"]["arrays"]}
    assert {name: list(a.shape) for name, a in arrays.items()} == d["dump_outputs"]["arrays"]
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    counts = arrays["count_per_frame"]
    assert counts.shape == (n_frames,) and counts.sum() == len(arrays["frame"]) and "sample_index" not in arrays
    assert (np.diff(arrays["frame"]) >= 0).all() and (np.bincount(arrays["frame"].astype(int), minlength=n_frames) == counts).all()
    n = int(counts.sum())
    assert arrays["boxes_tlbr"].shape == (n, 4) and arrays["scores"].shape == arrays["classes"].shape == (n,)
    assert ((arrays["scores"] >= 0.05) & (arrays["scores"] <= 1)).all() and (arrays["classes"] == np.round(arrays["classes"])).all()
    return n


@pytest.mark.gpu
def test_bench_plain_run_prints_only_the_headline(tmp_path):
    """A plain `bench.py` run (no --full) sets up, warms up, times, dumps and prints: the headline keys, none of the
    sections that take runs of their own (CPU baseline, per-kernel passes, other configurations, agreement)."""
    import subprocess
    import sys
    from golden_util import ROOT
    dump = str(tmp_path / "dump")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "yolov3-tiny", "--dim", "416",
                           "--batch", "2", "--steps", "3", "--warmup", "1", "--repeats", "5", "--dump-outputs", dump],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "dtype", "config"):
        assert key in d, key
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["repeats"]["windows"] == 5 and d["repeats"]["ms_per_step_min"] <= d["ms_per_step"] <= d["repeats"]["ms_per_step_max"]
    for key in ("roofline", "kernels", "resident", "other_configs", "detection_regimes", "latency", "bf16_agreement", "f16_agreement"):
        assert key not in d, key
    assert d["cpu_baseline"] is None and "cpu_baseline_s" not in d["phases_s"]
    _check_dump(dump, d, 2)


@pytest.mark.gpu
def test_bench_prints_one_contract_json_line(tmp_path):
    """bench.py --full's output contract (one JSON line with the driver's keys plus roofline / cpu_baseline objects), on a
    small workload so the test stays short."""
    import subprocess
    import sys
    from golden_util import ROOT
    dump = str(tmp_path / "dump")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--model", "yolov3-tiny", "--dim", "416",
                           "--batch", "2", "--steps", "3", "--warmup", "1", "--cpu-budget", "4", "--repeats", "5",
                           "--dump-outputs", dump],
                          capture_output=True, text=True, timeout=900)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["value"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and "traffic" in r
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]
    assert c["cpu_model"] and c["batch1"]["fps"] > 0 and c["batch16"]["fps"] > 0
    # the headline is the PCIe-inclusive rate of the package's own loop; measured in the same run: the resident rate, the
    # other BASELINE configurations, bf16 detection agreement
    assert "pinned host memory" in d["config"]["workload"] and d["config"]["timed_loop"] == "yolov3.pipeline.Pipeline.submit"
    assert d["use_graph"] is False
    assert d["resident"]["value"] > 0
    assert {o["workload"] for o in d["other_configs"]} == {"yolov3-tiny 416x416 batch=8 float32", "yolov3-spp 608x608 batch=16 bf16",
                                                           "yolov3 608x608 batch=16 fp16", "yolov3 608x608 batch=16 bf16",
                                                           "yolov3 608x608 batch=16 float32"}
    for o in d["other_configs"]:
        assert o["value"] > 0 and abs(o["roofline"]["frac"] - o["roofline"]["achieved"] / o["roofline"]["peak"]) < 1e-3
    # the headline workload at the reference test's thresholds and in a heavy regime (more candidates, all kept
    # boxes still inside the records)
    regimes = d["detection_regimes"]
    assert [(g["prob_thresh"], g["nms_iou_thresh"]) for g in regimes] == [(0.2, 0.3), (0.05, 0.3)]
    assert all(g["value"] > 0 and g["candidates_per_frame"] >= g["kept_per_frame"] for g in regimes)
    assert regimes[1]["candidates_per_frame"] > regimes[0]["candidates_per_frame"] and regimes[1]["kept_per_frame"] <= regimes[1]["kmax"]
    agree = d["bf16_agreement"]["thr_0.05_iou_0.3"]
    assert len(agree["keep_set_jaccard"]) == 3 and min(agree["keep_set_jaccard"]) > 0.4
    assert agree["score_abs_diff"]["median"] < 0.01
    # round 5: the fp16 storage mode beside it (same kernels on the f16 MFMA): far closer to the reference's float32 lists
    f16 = d["f16_agreement"]
    assert min(f16["thr_0.05_iou_0.3"]["keep_set_jaccard"]) > 0.85 and f16["thr_0.05_iou_0.3"]["score_abs_diff"]["median"] < 1e-3
    assert f16["bench_regime"]["thr_0.05_iou_0.3"]["keep_set_jaccard"] > 0.9
    # R timed windows, the median is the value; the CPU baseline ran in a pinned child before any GPU call; phases
    assert d["repeats"]["windows"] == 5 and d["repeats"]["ms_per_step_min"] <= d["ms_per_step"] <= d["repeats"]["ms_per_step_max"]
    assert "child process" in c["process"] and len(c["pinned_cpus"]) == c["cores"] and len(c["loadavg_before"]) == 3
    assert d["phases_s"]["total_s"] > 0 and "cpu_baseline_s" in d["phases_s"]
    assert d["per_rank"]["placement"][0]["cpus"] >= 1
    # --dump-outputs: the detections of the last timed step, as Pipeline.results returned them
    _check_dump(dump, d, 2)


@pytest.mark.gpu
def test_bench_resident_variant_runs(tmp_path):
    """`bench.py --resident` (frames already in HBM, records left there: kernel A/B runs): runs and says in
    config.workload that it is not the headline configuration.  By default --steps is the number of timed steps (one
    window); --dump-outputs reads the last step's detections from the device."""
    import subprocess
    import sys
    from golden_util import ROOT
    dump = str(tmp_path / "dump")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "yolov3-tiny", "--dim", "416",
                           "--batch", "2", "--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--resident",
                           "--obj-bias", "-5", "--dump-outputs", dump],
                          capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stderr[-2000:]
    d = json.loads([l for l in proc.stdout.splitlines() if l.startswith("{")][0])
    assert d["value"] > 0 and "NOT the headline" in d["config"]["workload"] and "resident" not in d
    assert d["steps"] == 5 and d["repeats"]["windows"] == 1
    assert _check_dump(dump, d, 2) > 0           # objectness bias -5: a few hundred candidates per frame


@pytest.mark.gpu
def test_bench_under_torchrun_runs_the_rccl_plumbing():
    """One rank under torchrun with Y3_BENCH_FORCE_DIST=1: process-group init on RCCL, barriers, the per-step
    all-gather of detection records issued from three streams, the max all-reduce and the teardown all execute on a
    real GPU (multi-rank correctness of the sharding / gather itself is covered by the gloo test on CPU)."""
    import subprocess
    import sys
    from golden_util import ROOT
    env = dict(os.environ, Y3_BENCH_FORCE_DIST="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    proc = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                           "--master-addr", "127.0.0.1", "--master-port", "29533", os.path.join(ROOT, "bench.py"),
                           "--gpus", "1", "--model", "yolov3-tiny", "--dim", "416", "--batch", "4", "--steps", "6",
                           "--warmup", "3", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, env=env)
    assert proc.returncode == 0, (proc.stdout[-1500:], proc.stderr[-1500:])
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and "all_gather_into_tensor" in d["config"]["collective"]
    assert d["config"]["collective"].startswith("1 x ") and d["config"]["ranks_seen_by_collective"] == 1


@pytest.mark.gpu
def test_bench_refuses_more_gpus_than_visible_on_the_gpu_box():
    """`python bench.py --gpus N` (no torchrun) with fewer than N GPUs: non-zero exit and a clear message, never a
    silent one-rank run."""
    import subprocess
    import sys
    import torch
    from golden_util import ROOT
    want = torch.cuda.device_count() + 1
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(want), "--steps", "1", "--warmup", "0"],
                          capture_output=True, text=True, timeout=300, env=env)
    assert proc.returncode != 0
    assert "%d GPUs requested, %d visible" % (want, want - 1) in proc.stderr
    assert not [l for l in proc.stdout.splitlines() if l.startswith("{")]


def test_video_io_without_opencv(tmp_path):
    """Motion-JPEG AVI and YUV4MPEG2, the two containers readable without a codec library (yolov3/videoio.py): what
    the writer produces the reader returns frame for frame (AVI: exactly the JPEG decode of every frame; y4m: YCbCr
    4:2:0 round trip of smooth frames within a few grey levels), frame rates survive, other files are refused."""
    import io
    from PIL import Image
    from yolov3 import videoio
    yy, xx = np.mgrid[0:46, 0:62]
    frames = [np.stack([(xx * 3 + i * 7) % 256, (yy * 5) % 256, (xx + yy + i) % 256], axis=-1).astype(np.uint8) for i in range(5)]
    avi = str(tmp_path / "clip.avi")
    videoio.write_avi_mjpeg(avi, frames, fps=30, quality=95)
    fps, got = videoio.open_video(avi)
    got = list(got)
    assert fps == 30 and len(got) == 5
    for src, g in zip(frames, got):
        buf = io.BytesIO()
        Image.fromarray(src[:, :, ::-1]).save(buf, format="JPEG", quality=95)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))[:, :, ::-1]
        assert g.shape == src.shape and np.array_equal(g, want)
    ys, xs = np.mgrid[0:40, 0:60]
    smooth = [np.stack([np.full((40, 60), 40 + 10 * i), (xs * 2 + 30) % 200, (ys * 3 + 20) % 200],
                       axis=-1).astype(np.uint8) for i in range(3)]
    y4m = str(tmp_path / "clip.y4m")
    videoio.write_video(y4m, smooth, fps=24)
    fps, got = videoio.open_video(y4m)
    got = list(got)
    assert fps == 24 and len(got) == 3
    for src, g in zip(smooth, got):
        assert g.shape == src.shape and np.abs(g.astype(int) - src.astype(int)).mean() < 4
    grey = np.full((8, 8, 3), 128, np.uint8)          # a grey frame survives YCbCr exactly to +-1
    videoio.write_y4m(y4m, [grey], 25)
    assert np.abs(list(videoio.open_video(y4m)[1])[0].astype(int) - 128).max() <= 1
    bad = tmp_path / "clip.mp4"
    bad.write_bytes(b"\x00\x00\x00\x18ftypmp42" + b"\x00" * 64)
    with pytest.raises(ValueError):
        videoio.open_video(str(bad))
    assert stream.video_fps(avi) == 30


@pytest.mark.gpu
def test_cli_video_file_round_trip(tmp_path):
    """`yolov3 --video clip.avi -o out.avi` without OpenCV: detections equal running the decoded frames through
    detect_in_frames, and the annotated output video has as many frames as the input."""
    from yolov3 import videoio
    from yolov3.__main__ import main as cli_main
    frames = [f for f in synth_frames(11, 5, 208, 256)]
    clip = str(tmp_path / "in.avi")
    videoio.write_avi_mjpeg(clip, frames, fps=12)
    decoded = list(videoio.open_video(clip)[1])
    net = _net()
    want = list(stream.detect_in_frames(net, decoded, batch_size=2, prob_thresh=0.2))
    out = str(tmp_path / "out.avi")
    out_json = str(tmp_path / "out.json")
    rc = cli_main(["-V", clip, "-c", MODELS["yolov3-tiny"], "-w", golden_weights_path("yolov3-tiny"), "-p", "0.2",
                   "--dtype", "float32", "-b", "2", "-o", out, "--json", out_json])
    assert rc == 0
    fps, annotated = videoio.open_video(out)
    assert fps == 12 and len(list(annotated)) == 5
    with open(out_json) as fh:
        ds = json.load(fh)
    assert len(ds["images"]) == 5 and len(ds["annotations"]) == sum(len(r[1]) for r in want)


@pytest.mark.gpu
def test_bench_self_launch_on_a_real_gpu():
    """`python bench.py --gpus N` as the driver calls it, with the one GPU this box has (Y3_BENCH_FORCE_LAUNCH=1): the parent
    counts devices without touching the GPU, starts the torchrun child job under its watchdog, the rank initialises RCCL, verifies
    the ranks with a real all-gather, runs the pipelined steps with one all-gather per step, and the parent relays exactly one
    JSON line (it arrives tee'd through torchrun's per-rank prefix: a 10-KiB line must survive that)."""
    import subprocess
    import sys
    from golden_util import ROOT
    env = dict(os.environ, Y3_BENCH_FORCE_LAUNCH="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "yolov3-tiny", "--dim", "416",
                           "--batch", "4", "--steps", "8", "--warmup", "3", "--no-cpu-baseline", "--launch-timeout", "400"],
                          capture_output=True, text=True, timeout=600, env=env)
    assert proc.returncode == 0, (proc.stdout[-1500:], proc.stderr[-2500:])
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["config"]["ranks_seen_by_collective"] == 1
    assert "all_gather_into_tensor" in d["config"]["collective"] and len(d["per_rank"]["ms_per_step_by_rank"]) == 1
