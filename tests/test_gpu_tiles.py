"""Tiled inference on the GPU (-m gpu): ``y3_tiles_u8`` against numpy's crop plus pad, ``y3_detect_tiled`` against the
restatement of tests/tiles_restate.py on planted tensors, and ``inference(tile_overlap=...)`` end to end on
tests/golden/cfg/mini.cfg against the restatement applied to the same tiles' forward outputs.

Both sides of a tail case receive the same float32 numbers; the scale is one float32 product (-ffp-contract=off), everything
after the truncation is integer or float64: every comparison is equality.  Scores are all different except where a case is
about a tie, and tie cases stay at 16 candidates or fewer, where numpy's argsort is stable.  The cutter's ``d_dst`` lies between
canaries, and every output of the tail has a guard behind its ``tiles * rows`` capacity."""
import ctypes

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip, tiles
from yolov3 import weights as W
from yolov3.inference import Detector, cut_tiles_device
from yolov3.preprocess import resize_bilinear_u8

import tiles_restate as R
from detect_util import F, assert_canonical_order, assert_equals_oracle, dev
from golden_util import MODELS

pytestmark = pytest.mark.gpu

CANARY, PAD = 0xA5, 512


# ---- the cutter ------------------------------------------------------------------------------------------------------------------
def _cut(frames, cuts, net_h, net_w, fill, launches):
    """``y3_tiles_u8`` on ``cuts`` = [(frame index, y0, x0), ...] into a buffer between canaries; checked against crop plus pad."""
    d = dev()
    srcs = [torch.from_numpy(f).to(d) for f in frames]
    nbytes = len(cuts) * net_h * net_w * 3
    buf = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8, device=d)
    descs = (_hip.Y3Tile * len(cuts))(*[_hip.Y3Tile(srcs[i].data_ptr(), frames[i].shape[0], frames[i].shape[1], y0, x0)
                                         for i, y0, x0 in cuts])
    with _hip.launch_log() as log:
        _hip.check(_hip.lib().y3_tiles_u8(descs, len(cuts), buf.data_ptr() + PAD, net_h, net_w, fill, _hip.stream_ptr()))
    torch.cuda.synchronize()
    assert len(log.names) == launches and len(log.symbols) == 1 and "letterbox_u8_kernel" in log.symbols[0], log.names
    host = buf.cpu().numpy()
    assert (host[:PAD] == CANARY).all() and (host[PAD + nbytes:] == CANARY).all(), "a write outside d_dst"
    got = host[PAD:PAD + nbytes].reshape(len(cuts), net_h, net_w, 3)
    for k, (i, y0, x0) in enumerate(cuts):
        want = R.crop_pad(frames[i], y0, x0, net_h, net_w, fill)
        assert np.array_equal(got[k], want), "tile %d (frame %d at %d, %d): %d bytes differ" % (
            k, i, y0, x0, int((got[k] != want).sum()))
    return got


def test_cut_a_frame_smaller_than_the_network_in_both_axes():
    got = _cut([R.arange_frame(20, 30)], [(0, 0, 0)], 32, 64, 7, 1)
    assert (got[0, 20:] == 7).all() and (got[0, :, 30:] == 7).all()


def test_cut_a_frame_one_pixel_larger_than_the_network():
    grid = tiles.tile_grid(33, 65, 32, 64, 0.25)
    assert grid == [(0, 0), (0, 1), (1, 0), (1, 1)]
    _cut([R.arange_frame(33, 65)], [(0, y0, x0) for y0, x0 in grid], 32, 64, 7, 1)


def test_cut_at_origins_whose_byte_offsets_are_no_multiple_of_16():
    # row pitch 300 bytes; (3, 5) starts at byte 915, (1, 1) at 303, (49, 99) is the last pixel: one pixel and fill
    _cut([R.arange_frame(50, 100)], [(0, 3, 5), (0, 1, 1), (0, 0, 37), (0, 49, 99), (0, 20, 36)], 32, 64, 0, 1)


def test_cut_into_a_33_by_35_canvas_takes_the_byte_stores():
    assert (33 * 35 * 3) % 16 != 0
    _cut([R.arange_frame(70, 80)], [(0, 0, 0), (0, 37, 45), (0, 60, 70), (0, 11, 13)], 33, 35, 255, 1)


def test_cut_into_a_32_by_64_canvas_takes_the_16_byte_stores():
    assert (32 * 64 * 3) % 16 == 0
    got = cut_tiles_device(torch.from_numpy(R.arange_frame(90, 200)).to(dev()), 32, 64, tiles.tile_grid(90, 200, 32, 64, 0.5), fill=3)
    want = tiles.cut_tiles_u8(R.arange_frame(90, 200), 32, 64, tiles.tile_grid(90, 200, 32, 64, 0.5), fill=3)
    assert np.array_equal(got.cpu().numpy(), want)
    _cut([R.arange_frame(90, 200)], [(0, y0, x0) for y0, x0 in tiles.tile_grid(90, 200, 32, 64, 0.5)], 32, 64, 3, 1)


def test_cut_33_tiles_in_one_call_takes_two_launches():
    cuts = [(0, (7 * k) % 100, (13 * k) % 200) for k in range(33)]
    _cut([R.arange_frame(100, 200)], cuts, 32, 64, 128, 2)


def test_cut_tiles_of_two_frames_of_different_sizes_in_one_call():
    frames = [R.arange_frame(40, 150), R.arange_frame(97, 31, start=100)]
    _cut(frames, [(0, 0, 0), (1, 0, 0), (0, 8, 86), (1, 65, 0), (1, 96, 30), (0, 39, 149)], 32, 64, 77, 1)


# ---- the tail ----------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _guarded(shape, dtype, d):
    """A zeroed buffer of ``shape`` with GUARD elements of ones after it: (the whole allocation, the buffer)."""
    n = int(np.prod(shape))
    whole = torch.zeros(n + GUARD, dtype=dtype, device=d)
    whole[n:] = 1
    return whole, whole[:n].view(shape)


def tiled_detect(box, prob, cls, batch, n_tiles, geom, prob_thresh, iou):
    """``y3_detect_tiled`` through ctypes with buffers of its own.  box (batch * n_tiles, rows, 4) etc.; geom: batch * n_tiles
    tuples.  -> per frame (tlbr, prob, cls, combined rows), and the raw output tensors."""
    lib = _hip.lib()
    d = dev()
    rows = prob.shape[1]
    assert prob.shape[0] == batch * n_tiles == len(geom)
    cap = n_tiles * rows
    tb, tp, tc = torch.from_numpy(box).to(d), torch.from_numpy(prob).to(d), torch.from_numpy(cls).to(d)
    garr = np.array([tuple(g) for g in geom], dtype=np.dtype([("sx", "<f4"), ("sy", "<f4"), ("ox", "<i4"), ("oy", "<i4")]))
    assert garr.itemsize == 16
    tg = torch.from_numpy(garr.view(np.uint8).copy()).to(d)
    nbytes = lib.y3_detect_tiled_workspace_bytes(batch, n_tiles, rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    wc, count = _guarded((batch,), torch.int32, d)
    wt, tlbr = _guarded((batch, cap, 4), torch.int64, d)
    wp, dprob = _guarded((batch, cap), torch.float32, d)
    wk, dcls = _guarded((batch, cap), torch.int64, d)
    wr, drow = _guarded((batch, cap), torch.int32, d)
    with _hip.launch_log() as log:
        _hip.check(lib.y3_detect_tiled(tb.data_ptr(), tp.data_ptr(), tc.data_ptr(), batch, n_tiles, rows, tg.data_ptr(),
                                       ctypes.c_float(float(F(prob_thresh))), ctypes.c_double(iou), ws.data_ptr(), nbytes,
                                       count.data_ptr(), tlbr.data_ptr(), dprob.data_ptr(), dcls.data_ptr(), drow.data_ptr(),
                                       _hip.stream_ptr()))
    torch.cuda.synchronize()
    assert len(log.names) == 1 and "detect_kernel" in log.names[0] and "Lb0ELi0E" in log.names[0], log.names
    for whole in (wc, wt, wp, wk, wr):
        assert bool((whole[-GUARD:] == 1).all()), "a write past the outputs' capacity"
    n = count.cpu().numpy()
    frames = [(tlbr[f, :n[f]].cpu().numpy(), dprob[f, :n[f]].cpu().numpy(), dcls[f, :n[f]].cpu().numpy(),
               drow[f, :n[f]].cpu().numpy().astype(np.int64)) for f in range(batch)]
    return frames, (count, tlbr, dprob, dcls, drow)


def _against_restatement(box, prob, cls, batch, n_tiles, geom, prob_thresh, iou):
    got, _ = tiled_detect(box, prob, cls, batch, n_tiles, geom, prob_thresh, iou)
    counts = []
    for f in range(batch):
        s = slice(f * n_tiles, (f + 1) * n_tiles)
        want, n_cand = R.tiled_postprocess(box[s], prob[s], cls[s], geom[s], F(prob_thresh), iou)
        print("frame %d: %d candidates, kept %d (restatement %d)" % (f, n_cand, len(got[f][3]), len(want[3])))
        assert_equals_oracle(got[f], want)          # the same rows; box, score bits and class at each; canonical order
        assert_canonical_order(got[f][1], got[f][2], got[f][3])
        assert len(got[f][3]) <= n_cand <= n_tiles * prob.shape[1]
        counts.append((n_cand, len(got[f][3])))
    return got, counts


def test_one_tile_equals_y3_detect_bit_for_bit():
    batch, rows = 2, 3000
    box, prob, cls = R.random_outputs(3, batch, rows, 5)
    hw = np.array([[480, 640], [1080, 1921]], np.int32)
    geom = [(float(w), float(h), 0, 0) for h, w in hw.tolist()]
    _, tiled = tiled_detect(box, prob, cls, batch, 1, geom, 0.6, 0.3)
    lib, d = _hip.lib(), dev()
    tb, tp, tc = torch.from_numpy(box).to(d), torch.from_numpy(prob).to(d), torch.from_numpy(cls).to(d)
    nbytes = lib.y3_detect_workspace_bytes(batch, rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    plain = (torch.zeros(batch, dtype=torch.int32, device=d), torch.zeros((batch, rows, 4), dtype=torch.int64, device=d),
             torch.zeros((batch, rows), dtype=torch.float32, device=d), torch.zeros((batch, rows), dtype=torch.int64, device=d),
             torch.zeros((batch, rows), dtype=torch.int32, device=d))
    _hip.check(lib.y3_detect(tb.data_ptr(), tp.data_ptr(), tc.data_ptr(), batch, rows, torch.from_numpy(hw).to(d).data_ptr(),
                             ctypes.c_float(float(F(0.6))), ctypes.c_double(0.3), ws.data_ptr(), nbytes,
                             *[t.data_ptr() for t in plain], _hip.stream_ptr()))
    torch.cuda.synchronize()
    assert int(plain[0].min()) > 100
    for a, b in zip(tiled, plain):
        assert torch.equal(a, b)                    # slots past a frame's count are written by neither: both were zeroed


def _seen_twice():
    """The object at frame (56, 20), 10 x 10, in the tiles at x0 = 0 (row 2) and x0 = 48 (row 4); the tile at x0 = 96 is empty."""
    box = np.zeros((3, 5, 4), F)
    prob = np.zeros((3, 5), F)
    cls = np.full((3, 5), 3, np.int64)
    box[0, 2] = [56 / 64, 20 / 64, 10 / 64, 10 / 64]
    box[1, 4] = [8 / 64, 20 / 64, 10 / 64, 10 / 64]
    geom = [(64.0, 64.0, 0, 0), (64.0, 64.0, 48, 0), (64.0, 64.0, 96, 0)]
    return box, prob, cls, geom


def test_an_object_in_two_overlapping_tiles_survives_once_with_the_higher_score():
    box, prob, cls, geom = _seen_twice()
    prob[0, 2], prob[1, 4] = 0.8, 0.9
    got, counts = _against_restatement(box, prob, cls, 1, 3, geom, 0.5, 0.3)
    assert counts == [(2, 1)]
    assert got[0][3].tolist() == [9] and got[0][0].tolist() == [[51, 15, 61, 25]] and got[0][1].tolist() == [F(0.9)]


def test_an_exact_tie_goes_to_the_higher_combined_row():
    box, prob, cls, geom = _seen_twice()
    prob[0, 2] = prob[1, 4] = 0.75
    got, counts = _against_restatement(box, prob, cls, 1, 3, geom, 0.5, 0.3)
    assert counts == [(2, 1)] and got[0][3].tolist() == [9]
    # a third copy, from the last tile's first row: combined row 10 is the highest of the three and wins
    box[2, 0], prob[2, 0] = [-40 / 64, 20 / 64, 10 / 64, 10 / 64], 0.75              # the same object from x0 = 96
    got, counts = _against_restatement(box, prob, cls, 1, 3, geom, 0.5, 0.3)
    assert counts == [(3, 1)] and got[0][3].tolist() == [10]


def test_negative_and_fractional_centres_are_truncated_before_the_offset():
    # products -0.75, 2.5, -3.25, 63.5, -1.0 and 0.999..: toward zero, then + 10 / + 7; sizes 0: corners = centre
    vals = [-0.75, 2.5, -3.25, 63.5, -1.0, 0.99]
    box = np.zeros((1, len(vals), 4), F)
    box[0, :, 0] = np.array(vals, F) / F(64)
    box[0, :, 1] = np.array(vals[::-1], F) / F(64)
    prob = R.unique_scores(np.random.default_rng(0), (1, len(vals))) * F(0.4) + F(0.5)
    cls = np.arange(len(vals), dtype=np.int64)[None]                          # one class each: nothing is suppressed
    got, counts = _against_restatement(box, prob, cls, 1, 1, [(64.0, 64.0, 10, 7)], 0.5, 0.3)
    assert counts == [(len(vals), len(vals))]
    by_row = got[0][0][np.argsort(got[0][3])]
    trunc = [0, 2, -3, 63, -1, 0]
    assert by_row[:, 0].tolist() == [10 + t for t in trunc] and by_row[:, 1].tolist() == [7 + t for t in trunc[::-1]]
    assert np.array_equal(by_row[:, :2], by_row[:, 2:])
    assert by_row[0, 0] != int(np.floor(-0.75 + 10))                           # adding first would have given 9


def test_nine_tiles_of_1000_rows():
    """Tile borders fall inside a 1024-thread chunk and inside a wave (1000 = 15 * 64 + 40), and 9000 rows are more than one
    8192-row compaction pass."""
    box, prob, cls = R.random_outputs(11, 9, 1000, 4)
    got, counts = _against_restatement(box, prob, cls, 1, 9, R.grid_geom(3, 3, 64, 48), 0.8, 0.3)
    assert 1000 < counts[0][0] < 4096 and 50 < counts[0][1] < counts[0][0]
    t = got[0][3] // 1000
    assert sorted(set(t.tolist())) == list(range(9))                          # every tile keeps something
    assert (got[0][3] >= 8192).any()


def test_more_than_4096_candidates_take_the_global_memory_sort():
    box, prob, cls = R.random_outputs(12, 9, 1000, 12, size=0.5)
    got, counts = _against_restatement(box, prob, cls, 1, 9, R.grid_geom(3, 3, 64, 56), 0.4, 0.3)
    assert counts[0][0] > 4096 and counts[0][1] > 100


def test_two_frames_with_different_geometry():
    box, prob, cls = R.random_outputs(13, 2 * 4, 300, 3)
    geom = R.grid_geom(2, 2, 64, 40) + [(32.0, 48.0, 5, 0), (32.0, 48.0, 21, 0), (32.0, 48.0, 5, 30), (90.0, 70.0, 0, 0)]
    got, counts = _against_restatement(box, prob, cls, 2, 4, geom, 0.7, 0.3)
    assert all(c[0] > 100 and c[1] > 10 for c in counts)
    # each frame alone gives what it gives inside the batch
    for f in range(2):
        s = slice(4 * f, 4 * f + 4)
        alone, _ = tiled_detect(box[s], prob[s], cls[s], 1, 4, geom[s], 0.7, 0.3)
        for a, b in zip(alone[0], got[f]):
            assert np.array_equal(a, b)


def test_overview_geometry_mixed_with_plain_tiles():
    # a 100 x 150 frame: 2 x 3 tiles of 64 x 64 cut 1:1, and the whole frame stretched
    grid = tiles.tile_grid(100, 150, 64, 64, 0.25)
    geom = R.plain_geom(64, 64, grid) + [(150.0, 100.0, 0, 0)]
    assert len(geom) == 7
    box, prob, cls = R.random_outputs(14, 7, 200, 3)
    # the first 20 rows of the overview repeat what tile 4 = (36, 43) sees, in the overview's own relative coordinates
    y0, x0 = grid[4]
    box[6, :20, 0] = (box[4, :20, 0] * F(64) + F(x0)) / F(150)
    box[6, :20, 1] = (box[4, :20, 1] * F(64) + F(y0)) / F(100)
    box[6, :20, 2] = box[4, :20, 2] * F(64) / F(150)
    box[6, :20, 3] = box[4, :20, 3] * F(64) / F(100)
    cls[6, :20] = cls[4, :20]
    got, counts = _against_restatement(box, prob, cls, 1, 7, geom, 0.6, 0.3)
    assert counts[0][0] > 300 and (got[0][3] >= 6 * 200).any() and (got[0][3] < 200).any()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
NET_H, NET_W = 32, 48
_NET = []


def _mini():
    """tests/golden/cfg/mini.cfg (a 32 x 48 network, 360 rows) in float32 with the repository's procedural weights."""
    if not _NET:
        net = yolov3.Darknet(MODELS["mini"], device="cuda", dtype="float32").eval()
        _NET.append(net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-8.0, calib=None)))
    return _NET[0]


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def _restated_inference(net, image, overlap, overview, fill, tile_batch, prob_thresh, iou):
    """The tiles of ``image`` from numpy (crop plus pad; the overview by the host resize), run through ``forward_frames`` in the
    chunks ``inference()`` uses, and the restated tail on their outputs."""
    h, w = image.shape[:2]
    grid = [(y0, x0) for y0 in R_axis(h, NET_H, overlap) for x0 in R_axis(w, NET_W, overlap)]
    stack = [R.crop_pad(image, y0, x0, NET_H, NET_W, fill) for y0, x0 in grid]
    geom = R.plain_geom(NET_H, NET_W, grid)
    if overview:
        stack.append(resize_bilinear_u8(image, NET_H, NET_W))
        geom.append((float(w), float(h), 0, 0))
    stack = np.stack(stack)
    outs = [net.forward_frames(stack[i:i + tile_batch]) for i in range(0, len(stack), tile_batch)]
    fwd = {k: torch.cat([o[k] for o in outs]).cpu().numpy() for k in outs[0]}
    want, n_cand = R.tiled_postprocess(fwd["bbox_xywh"], fwd["class_prob"], fwd["class_idx"], geom, F(prob_thresh), iou)
    return want, n_cand, len(stack)


def R_axis(length, net, f):
    """The issue's per-axis rule, restated: one origin when the axis fits, else evenly spread origins from 0 to length - net."""
    ov = int(f * net)
    if length <= net:
        return [0]
    step = net - ov
    n = (length - ov + step - 1) // step
    return [(i * (length - net)) // (n - 1) for i in range(n)]


# (a net-sized frame with its overview would be the same tile twice: every candidate an exact tie, past what argsort keeps stable)
@pytest.mark.parametrize("shape,overview,tile_batch", [
    ((100, 150), True, 16), ((100, 150), True, 4), ((100, 150), False, 5), ((64, 64), True, 16), ((64, 64), False, 4),
    ((32, 48), False, 16), ((20, 30), True, 16), ((33, 49), True, 3)])
def test_inference_tiled_equals_the_restatement_on_the_same_tiles(shape, overview, tile_batch):
    net = _mini()
    image = _frame(*shape, seed=sum(shape))
    thr, iou = 0.02, 0.3
    got = yolov3.inference(net, image, device="cuda", prob_thresh=thr, nms_iou_thresh=iou, return_rows=True, tile_overlap=0.25,
                           tile_overview=overview, tile_fill=99, tile_batch=tile_batch)
    want, n_cand, n_tiles = _restated_inference(net, image, 0.25, overview, 99, tile_batch, thr, iou)
    print("%s: %d tiles, %d candidates, kept %d" % (shape, n_tiles, n_cand, len(want[3])))
    assert len(got) == 1 and len(got[0]) == 4
    assert n_cand > 0 and len(want[3]) > 0, "no candidates: nothing would be compared"
    assert_equals_oracle(tuple(np.asarray(a) for a in got[0]), want)
    if shape == (100, 150):
        assert n_tiles == (16 + 1 if overview else 16)          # 4 x 4 windows of 32 x 48, a quarter shared


def test_tile_overlap_none_is_the_plain_call():
    net = _mini()
    frames = [_frame(100, 150, 1), _frame(100, 150, 2), _frame(32, 48, 3)]
    for image in frames:
        a = yolov3.inference(net, image, device="cuda", prob_thresh=0.02, return_rows=True)
        yolov3.inference(net, image, device="cuda", prob_thresh=0.02, tile_overlap=0.25)           # a tiled call in between
        b = yolov3.inference(net, image, device="cuda", prob_thresh=0.02, return_rows=True, tile_overlap=None)
        assert len(a[0][1]) > 0
        for x, y in zip(a[0], b[0]):
            assert np.array_equal(np.asarray(x), np.asarray(y))


def test_command_line_tiles_every_image(tmp_path):
    """``--tile-overlap`` loops ``inference()`` over the images: the JSON holds what the call returns for each."""
    import json

    from PIL import Image

    from yolov3.__main__ import main
    net = _mini()
    weights = str(tmp_path / "mini.weights")
    W.write_darknet_weights(weights, W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-8.0, calib=None))
    loaded = yolov3.Darknet(MODELS["mini"], device="cuda", dtype="float32").load_weights(weights).eval()
    folder = tmp_path / "images"
    folder.mkdir()
    images = {"a.png": _frame(70, 100, 5), "b.png": _frame(32, 48, 6)}
    for name, im in images.items():
        Image.fromarray(im[:, :, ::-1]).save(str(folder / name))
    dump = tmp_path / "det.json"
    assert main(["-c", MODELS["mini"], "-w", weights, "-I", str(folder), "-p", "0.02", "--tile-overlap", "0.25", "--no-tile-overview",
                 "--batch-size", "4", "--json", str(dump)]) == 0
    with open(str(dump)) as fh:
        coco = json.load(fh)
    ids = {im["file_name"]: im["id"] for im in coco["images"]}
    assert sorted(ids) == sorted(images)
    for name, im in images.items():
        tlbr, prob, cls = yolov3.inference(loaded, im, device="cuda", prob_thresh=0.02, tile_overlap=0.25, tile_overview=False,
                                           tile_batch=4)[0]
        assert len(prob) > 0
        got = sorted((a["category_id"], a["score"], tuple(a["bbox"])) for a in coco["annotations"] if a["image_id"] == ids[name])
        want = sorted((int(c), float(p), (int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])))
                      for b, p, c in zip(tlbr.tolist(), prob.tolist(), cls.tolist()))
        assert got == want, name


def test_run_tiled_on_a_detector_of_its_own():
    box, prob, cls = R.random_outputs(15, 4, 100, 3)
    geom = R.grid_geom(2, 2, 64, 48)
    det = Detector(1, 400, dev())
    det.run_tiled({"bbox_xywh": torch.from_numpy(box).cuda(), "class_prob": torch.from_numpy(prob).cuda(),
                   "class_idx": torch.from_numpy(cls).cuda()}, geom, 4, float(F(0.5)), 0.3)
    got = det.fetch(return_rows=True)[0]
    want, n_cand = R.tiled_postprocess(box, prob, cls, geom, F(0.5), 0.3)
    assert n_cand > 50
    assert_equals_oracle((got[0], got[1], got[2], np.asarray(got[3], np.int64)), want)
    with pytest.raises(ValueError):
        det.run_tiled({"bbox_xywh": torch.from_numpy(box).cuda(), "class_prob": torch.from_numpy(prob).cuda(),
                       "class_idx": torch.from_numpy(cls).cuda()}, geom, 3, 0.5, 0.3)
