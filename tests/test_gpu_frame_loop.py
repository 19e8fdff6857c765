"""The frame loop users call (yolov3/stream.py: ``detect_in_frames`` on the ``Pipeline`` it caches on the network) across
calls, input forms and shared plans: the state that survives from one call to the next -- the cached pipeline and its ``busy``
flag, tickets that keep counting, pinned buffers, device frames kept per ticket slot, the compute streams every pipeline of a
device shares, compiled plans shared by key.  The reference of every case is per-frame ``inference()`` with the same arguments
on the same frames as numpy arrays (itself pinned to the oracle and the goldens: test_gpu_parity.py), compared with
``np.array_equal``.  The generator's own bookkeeping runs on a recording stub in test_callers.py, without a GPU.

Most cases run tests/golden/cfg/mini.cfg, a 32 x 48 network: small, and not square, so that the frames ``inference()`` stretches
enter the network 48 x 32 (``preprocess.reference_dsize``) and the loop needs a second pipeline for them.  Need an MI355X: -m gpu."""
import gc

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import pipeline as pipeline_module
from yolov3 import weights as W
from yolov3.pipeline import Pipeline
from yolov3.synthdata import synth_frames

from golden_util import MODELS

pytestmark = pytest.mark.gpu

NET_H, NET_W = 32, 48
# three calls that differ in everything a cached pipeline is told anew: threshold, IoU threshold, suppression rule
SETTINGS = (dict(prob_thresh=0.05, nms_iou_thresh=0.3), dict(prob_thresh=0.1, nms_iou_thresh=0.45, nms_kind="greedynms"),
            dict(prob_thresh=0.02, nms_iou_thresh=0.2, nms_kind="diounms", beta_nms=0.8))


def _mini():
    """mini.cfg with procedural weights; objectness bias -8 leaves from a few to a few dozen of the 360 rows per frame at the
    thresholds above (counted on the CPU oracle)."""
    net = yolov3.Darknet(MODELS["mini"], device="cuda", dtype="float32").eval()
    return net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-8.0, calib=None))


def _tiny():
    """yolov3-tiny at 416 in bf16: with ``in_flight > 1`` its pipeline plans take the throughput-tile option."""
    net = yolov3.Darknet(MODELS["yolov3-tiny"], device="cuda", dtype="bf16").eval()
    return net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-5.0, calib=W.load_calibration("yolov3-tiny")))


def _other_sized(seed, n):
    """n frames that are not net-sized, of two sizes in turn (one of them odd and narrower than it is tall)."""
    a, b = synth_frames(seed, n, 40, 56), synth_frames(seed + 1, n, 61, 27)
    return [a[i] if i % 2 == 0 else b[i] for i in range(n)]


def _reference(net, frames, **kw):
    want = [yolov3.inference(net, np.asarray(f), **kw)[0] for f in frames]
    assert sum(len(w[1]) for w in want) > 0, "the reference kept no detection: nothing would be compared"
    return want


def _check(got, want, note=None):
    assert len(got) == len(want), (len(got), len(want), note)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w) == 3
        for x, y in zip(g, w):
            assert np.array_equal(x, y), (i, note)
    assert sum(len(g[1]) for g in got) > 0


def _idle(pipe):
    return (not pipe.busy) and all(s.query() for s in pipe.streams + [pipe.copy_stream])


# ---------------------------------------------------------------------------------------------- reuse across calls
@pytest.mark.parametrize("model", ["mini", "yolov3-tiny-bf16"])
def test_one_pipeline_serves_call_after_call(model):
    """Three calls on one network with one cache key and different thresholds, IoU thresholds and suppression rules: each
    equals its own reference, on one cached pipeline that is idle between the calls and whose tickets go on counting."""
    if model == "mini":
        net, frames, batch, in_flight = _mini(), list(synth_frames(21, 7, NET_H, NET_W)), 3, 2
    else:
        net, frames, batch, in_flight = _tiny(), list(synth_frames(21, 8, 416, 416)), 4, 3
    n_batches = -(-len(frames) // batch)
    pipe = None
    for call, kw in enumerate(SETTINGS):
        want = _reference(net, frames, **kw)
        got = list(yolov3.detect_in_frames(net, iter(frames), batch_size=batch, in_flight=in_flight, **kw))
        _check(got, want, kw)
        cached = list(net._pipelines.values())
        assert len(cached) == 1 and (pipe is None or cached[0] is pipe)
        pipe = cached[0]
        assert not pipe.busy and pipe._n == (call + 1) * n_batches
    assert pipe.batch == batch and pipe.in_flight == in_flight


# ---------------------------------------------------------------------------------------------- abandonment
def _held_up(pipe):
    """~0.1 s of work queued on the pipeline's first stream: a generator that left without synchronising would leave it there."""
    with torch.cuda.stream(pipe.streams[0]):
        torch.cuda._sleep(200_000_000)


@pytest.mark.parametrize("in_flight", [1, 3])
@pytest.mark.parametrize("how", ["close", "iterable raises", "throw", "dropped"])
def test_an_abandoned_generator_leaves_the_pipeline_idle(how, in_flight):
    """A generator left half way -- closed with tickets open, ended by its frame iterable, by an exception thrown in by the
    consumer, or dropped and collected -- leaves the cached pipeline not busy and nothing queued on any of its streams (work
    is provably queued when it leaves: ``_held_up``), and the next full call equals the reference."""
    net = _mini()
    frames = list(synth_frames(33, 16, NET_H, NET_W))
    kw = dict(prob_thresh=0.05, nms_iou_thresh=0.3)
    want = _reference(net, frames, **kw)

    def source():
        for i, f in enumerate(frames):
            if how == "iterable raises" and i == 4:          # after the second batch
                _held_up(list(net._pipelines.values())[0])
                raise KeyError("decoder")
            yield f

    gen = yolov3.detect_in_frames(net, source(), batch_size=2, in_flight=in_flight, **kw)
    if how == "iterable raises":
        with pytest.raises(KeyError):
            next(gen)
        pipe = list(net._pipelines.values())[0]
        assert pipe._n == 2
    else:
        _check([next(gen)], want[:1])
        pipe = list(net._pipelines.values())[0]
        assert pipe.busy and pipe._n == pipe.max_open          # one ticket taken (in part), the others still open
        _held_up(pipe)
        if how == "close":
            gen.close()
        elif how == "throw":
            with pytest.raises(ZeroDivisionError):
                gen.throw(ZeroDivisionError("consumer"))
        else:
            del gen
            gc.collect()
    assert _idle(pipe), "busy = {}, streams idle = {}".format(pipe.busy, [s.query() for s in pipe.streams + [pipe.copy_stream]])
    before = pipe._n
    _check(list(yolov3.detect_in_frames(net, frames, batch_size=2, in_flight=in_flight, **kw)), want)
    assert list(net._pipelines.values()) == [pipe] and pipe._n == before + 8 and _idle(pipe)


# ---------------------------------------------------------------------------------------------- two generators, one network
@pytest.mark.parametrize("in_flight", [1, 3])
def test_two_generators_interleaved_on_one_network(monkeypatch, in_flight):
    """Two generators open on one network at once, different frames and thresholds, ``next()`` in turn.  The second builds a
    pipeline of its own while the cached one is busy; both ask for the same plan slots, and plan slot k of both runs on the
    same stream object (the invariant stated at ``pipeline._STREAMS``).  Both equal their references; afterwards the cache
    holds the one pipeline it had, idle."""
    made = []

    class Recorded(Pipeline):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(pipeline_module, "Pipeline", Recorded)
    net = _mini()
    frames_a, frames_b = list(synth_frames(41, 14, NET_H, NET_W)), list(synth_frames(42, 14, NET_H, NET_W))
    kw_a, kw_b = SETTINGS[0], SETTINGS[1]
    want_a, want_b = _reference(net, frames_a, **kw_a), _reference(net, frames_b, **kw_b)
    a = yolov3.detect_in_frames(net, iter(frames_a), batch_size=2, in_flight=in_flight, **kw_a)
    b = yolov3.detect_in_frames(net, iter(frames_b), batch_size=2, in_flight=in_flight, **kw_b)
    got_a, got_b = [next(a)], [next(b)]
    assert len(made) == 2 and made[0] is not made[1] and made[0].busy and made[1].busy
    assert list(net._pipelines.values()) == [made[0]]
    assert len(made[0].streams) == len(made[1].streams) == in_flight
    for k in range(in_flight):
        assert made[0].plans[k] is made[1].plans[k]            # the same arena and output buffers ...
        assert made[0].streams[k] is made[1].streams[k]        # ... ordered by the one stream that runs them
    assert made[0].copy_stream is made[1].copy_stream
    for _ in range(13):
        got_a.append(next(a))
        got_b.append(next(b))
    assert list(a) == [] and list(b) == []
    _check(got_a, want_a, "a")
    _check(got_b, want_b, "b")
    assert len(made) == 2 and list(net._pipelines.values()) == [made[0]] and _idle(made[0]) and _idle(made[1])


# ---------------------------------------------------------------------------------------------- input forms
def _as_form(frame, form):
    if form == "numpy":
        return np.ascontiguousarray(frame)
    t = torch.from_numpy(np.ascontiguousarray(frame))
    return {"cpu": t, "pinned": t.pin_memory(), "cuda": t.cuda()}[form]


FRAME_CASES = [(form, size, letterbox) for form in ("numpy", "cpu", "cuda")
               for size, letterbox in (("net", False), ("other", False), ("other", True))]


@pytest.mark.parametrize("form,size,letterbox", FRAME_CASES, ids=["{}-{}{}".format(f, s, "-letterbox" if l else "") for f, s, l in FRAME_CASES])
def test_frame_forms(form, size, letterbox):
    """Frames as numpy arrays, host tensors and device tensors, net-sized or not, stretched or letterboxed: what the numpy
    frames give through ``inference()``.  (Net-sized device frames used to end in ``f.numpy()``: a TypeError.)"""
    net = _mini()
    frames = list(synth_frames(51, 7, NET_H, NET_W)) if size == "net" else _other_sized(52, 7)
    kw = dict(prob_thresh=0.05, nms_iou_thresh=0.3, letterbox=letterbox)
    want = _reference(net, frames, **kw)
    given = [_as_form(f, form) for f in frames]
    _check(list(yolov3.detect_in_frames(net, iter(given), batch_size=3, in_flight=3, **kw)), want)
    assert all(_idle(p) for p in net._pipelines.values())
    # not square, so the stretched frames ran on a pipeline of their own size
    sizes = {(p.height, p.width) for p in net._pipelines.values()}
    assert sizes == ({(NET_W, NET_H)} if size == "other" and not letterbox else {(NET_H, NET_W)})


@pytest.mark.parametrize("length", ["full", "short last batch"])
@pytest.mark.parametrize("form", ["numpy", "pinned", "cuda"])
def test_whole_batch_forms(form, length):
    """Whole (B, H, W, 3) batches as a numpy array, a pinned tensor and a device tensor; every batch full, or the last one
    short.  The device batches are made on the fly and dropped by the caller as soon as they are handed over.  (A short
    device batch used to end in ``f.numpy()``.)"""
    net = _mini()
    n = 12 if length == "full" else 10
    frames = synth_frames(53, n, NET_H, NET_W)
    kw = dict(prob_thresh=0.05, nms_iou_thresh=0.3)
    want = _reference(net, list(frames), **kw)

    def batches():
        for i in range(0, n, 4):
            yield _as_form(frames[i:i + 4], form)

    _check(list(yolov3.detect_in_frames(net, batches(), batch_size=4, in_flight=1, **kw)), want)
    pipe, = net._pipelines.values()
    assert pipe.batch == 4 and pipe._n == 3 and _idle(pipe)


def test_device_frames_on_yolov3_tiny_bf16():
    """Net-sized device frames and a short last device batch through the three-stream pipeline with its throughput tiles."""
    net = _tiny()
    frames = synth_frames(54, 8, 416, 416)
    kw = dict(prob_thresh=0.1, nms_iou_thresh=0.3)
    want = _reference(net, list(frames), **kw)
    singles = (torch.from_numpy(f).cuda() for f in frames)
    _check(list(yolov3.detect_in_frames(net, singles, batch_size=3, in_flight=3, **kw)), want, "frames")
    whole = (torch.from_numpy(frames[i:i + 3]).cuda() for i in range(0, 8, 3))
    _check(list(yolov3.detect_in_frames(net, whole, batch_size=3, in_flight=3, **kw)), want, "whole batches")
    pipe, = net._pipelines.values()
    assert pipe._n == 6 and _idle(pipe)


# ---------------------------------------------------------------------------------------------- mixed stream
@pytest.mark.parametrize("letterbox", [True, False], ids=["letterbox", "stretch"])
@pytest.mark.parametrize("in_flight", [1, 3])
def test_mixed_stream_reuses_every_slot_on_both_paths(in_flight, letterbox):
    """Batches alternate between the pinned path (net-sized frames) and the device path (other sizes), and the alternation
    turns round with every ``max_open`` batches, so that over ``4 * max_open + 1`` batches every ticket slot takes both
    paths twice, every pinned buffer is refilled and every kept device batch is replaced.  Letterboxed, all of it runs on one
    pipeline; stretched, the device batches of this network that is not square run on a second one, and the results still
    come in frame order."""
    net = _mini()
    max_open = 2 * in_flight
    n_batches = 4 * max_open + 1
    own, other = synth_frames(61, 2 * n_batches, NET_H, NET_W), _other_sized(62, 2 * n_batches)
    frames, pinned = [], 0
    for b in range(n_batches):
        on_pinned_path = (b + b // max_open) % 2 == 0
        pinned += on_pinned_path
        frames += [own[2 * b], own[2 * b + 1]] if on_pinned_path else [other[2 * b], other[2 * b + 1]]
    kw = dict(prob_thresh=0.05, nms_iou_thresh=0.3, letterbox=letterbox)
    want = _reference(net, frames, **kw)
    _check(list(yolov3.detect_in_frames(net, iter(frames), batch_size=2, in_flight=in_flight, **kw)), want)
    pipes = {(p.height, p.width): p for p in net._pipelines.values()}
    assert all(_idle(p) for p in pipes.values())
    if letterbox:
        assert list(pipes) == [(NET_H, NET_W)] and pipes[NET_H, NET_W]._n == n_batches
    else:
        assert sorted(pipes) == sorted([(NET_H, NET_W), (NET_W, NET_H)])
        assert pipes[NET_H, NET_W]._n == pinned and pipes[NET_W, NET_H]._n == n_batches - pinned
    assert pipes[NET_H, NET_W]._uploads == pinned > pipes[NET_H, NET_W].nbuf


# ---------------------------------------------------------------------------------------------- resize=False
def test_resize_false_takes_net_sized_frames_only():
    net = _mini()
    frames = list(synth_frames(71, 5, NET_H, NET_W))
    kw = dict(prob_thresh=0.05, nms_iou_thresh=0.3, resize=False)
    want = _reference(net, frames, **kw)
    _check(list(yolov3.detect_in_frames(net, iter(frames), batch_size=2, in_flight=2, **kw)), want)
    pipe, = net._pipelines.values()
    for bad in (synth_frames(72, 1, 40, 56)[0], torch.from_numpy(synth_frames(72, 1, 40, 56)[0]).cuda(), synth_frames(72, 2, 40, 56)):
        before = pipe._n
        gen = yolov3.detect_in_frames(net, frames[:3] + [bad], batch_size=2, in_flight=2, **kw)
        with pytest.raises(ValueError, match=r"40 x 56.*32 x 48.*inference\(resize=False\)"):
            list(gen)
        assert pipe._n == before + 1 and _idle(pipe)          # the first batch went in; the third frame waited for its group
    assert list(net._pipelines.values()) == [pipe]
    # ... and inference(resize=False) does run such a frame, at its own size
    assert len(yolov3.inference(net, synth_frames(72, 1, 40, 56)[0], prob_thresh=0.05, resize=False)[0]) == 3
    _check(list(yolov3.detect_in_frames(net, iter(frames), batch_size=2, in_flight=2, **kw)), want)


# ---------------------------------------------------------------------------------------------- plans are not inference()'s
def _span(t):
    return t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()


def _disjoint(a, b):
    return a[1] <= b[0] or b[1] <= a[0]


@pytest.mark.parametrize("pipeline_first", [False, True], ids=["inference-first", "pipeline-first"])
@pytest.mark.parametrize("in_flight", [1, 3])
def test_pipeline_plans_are_not_the_plan_of_inference(in_flight, pipeline_first):
    """``inference()`` / ``forward_frames()`` run the plan ``net._get_plan(b, h, w, "u8")`` on the caller's current stream.
    No plan of a ``Pipeline(net, b, in_flight=n)`` with default options is that object, and their arenas and output buffers
    share no byte, whichever was compiled first.  (With n = 1 the pipeline used to ask for the very same key; with n > 1 only
    the throughput-tile option it adds kept them apart.)"""
    net = _mini()
    batch = 2
    if pipeline_first:
        pipe = Pipeline(net, batch, in_flight=in_flight)
        base = net._get_plan(batch, NET_H, NET_W, "u8")
    else:
        base = net._get_plan(batch, NET_H, NET_W, "u8")
        pipe = Pipeline(net, batch, in_flight=in_flight)
    assert pipe.options is None or in_flight > 1
    assert len(pipe.plans) == in_flight and len({id(p) for p in pipe.plans}) == in_flight
    plans = [base] + list(pipe.plans)
    for i, p in enumerate(plans):
        for q in plans[i + 1:]:
            assert p is not q and p.handle.value != q.handle.value
            for name in ("arena", "bbox", "prob", "cls"):
                assert _disjoint(_span(getattr(p, name)), _span(getattr(q, name))), name
    # what forward_frames() runs by default is still `base`, and the pipeline's forwards still run the pipeline's plans
    frames = synth_frames(81, batch, NET_H, NET_W)
    net.forward_frames(frames, fresh=False)
    assert net._last_plan is base
    pipe.results(pipe.submit(frames))
    assert net._last_plan is pipe.plans[0]


def test_inference_inside_the_frame_loop():
    """``inference()`` on another frame at every step of a loop over ``detect_in_frames(batch_size=1, in_flight=1)`` -- the same
    batch size on the caller's stream while the generator is suspended with batches in flight: both sequences equal their
    references.  (What rules the race out is the test above; no timing is provoked here.)"""
    net = _mini()
    frames_a, frames_b = list(synth_frames(91, 9, NET_H, NET_W)), list(synth_frames(92, 9, NET_H, NET_W))
    kw_a, kw_b = SETTINGS[0], SETTINGS[1]
    want_a, want_b = _reference(net, frames_a, **kw_a), _reference(net, frames_b, **kw_b)
    got_a, got_b = [], []
    for i, result in enumerate(yolov3.detect_in_frames(net, iter(frames_a), batch_size=1, in_flight=1, **kw_a)):
        got_a.append(result)
        got_b.append(yolov3.inference(net, frames_b[i], **kw_b)[0])
    _check(got_a, want_a, "loop")
    _check(got_b, want_b, "inference")
