"""Parity tests proper: the HIP path (through the C ABI) against the golden vectors generated from
the reference and against the CPU oracle on the same seeded inputs.  Need an MI355X: -m gpu."""
import json
import os

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import weights as W
from yolov3.preprocess import resize_bilinear_u8
from yolov3.synthdata import synth_frames

from golden_util import (GOLDEN, MODELS, MODEL_DIMS, compare_detections, golden_params, golden_weights_path,
                         load_jpeg_bgr, sha)

pytestmark = pytest.mark.gpu

# float32 parity bars (BASELINE.json north_star: box coords and scores within 1e-3 fp32)
BOX_ATOL = 1e-3
SCORE_ATOL = 1e-3


def _net(model, dtype="float32", **kw):
    net = yolov3.Darknet(MODELS[model], device="cuda", dtype=dtype, **kw)
    if model == "mini":
        net.set_params(golden_params("mini"))
    else:
        net.load_weights(golden_weights_path(model))
    return net.eval()


def test_library_reports_gfx950():
    from yolov3 import _hip
    assert _hip.lib().y3_device_count() >= 1


def test_cxywh_to_tlbr_known_answer():
    xywh = np.array([[5, 8, 10, 13, 10000], [100, 200, 30, 17, 19000]], dtype=np.int64)
    want = np.array([[0, 2, 10, 14, 10000], [85, 192, 115, 208, 19000]])
    assert (yolov3.cxywh_to_tlbr(xywh) == want).all()
    neg = np.array([[-3, 4, 5, 7]], dtype=np.int64)
    assert (yolov3.cxywh_to_tlbr(neg) == orc.cxywh_to_tlbr(neg)).all()


def test_mini_every_block_fp32():
    g = np.load(os.path.join(GOLDEN, "mini_blocks.npz"))
    net = _net("mini", keep_all=True)
    out = net.forward(torch.from_numpy(g["input"]))
    worst = {}
    for i, blk in enumerate(net.blocks):
        key = "block_%d" % i
        if key not in g.files or blk["type"] == "yolo":
            continue
        try:
            got = net.block_output(i).cpu().numpy()
        except ValueError:
            continue  # fused away (conv feeding a shortcut)
        err = np.abs(got - g[key]).max()
        worst[i] = float(err)
        np.testing.assert_allclose(got, g[key], rtol=1e-4, atol=2e-5, err_msg="%s (%s)" % (key, blk["type"]))
    assert len(worst) >= 20
    np.testing.assert_allclose(out["bbox_xywh"].cpu().numpy(), g["bbox_xywh"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(out["class_prob"].cpu().numpy(), g["class_prob"], rtol=1e-4, atol=1e-6)
    assert out["class_idx"].dtype == torch.int64
    assert (out["class_idx"].cpu().numpy() == g["class_idx"]).mean() > 0.999


def test_mini_u8_frames_match_f32_input():
    g = np.load(os.path.join(GOLDEN, "mini_blocks.npz"))
    net = _net("mini")
    a = net.forward(torch.from_numpy(g["input"]))
    b = net.forward_frames(g["frames"])
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(a[k], b[k]), k


def test_mini_bf16_close_to_fp32():
    g = np.load(os.path.join(GOLDEN, "mini_blocks.npz"))
    net = _net("mini", dtype="bf16")
    out = net.forward(torch.from_numpy(g["input"]))
    dp = np.abs(out["class_prob"].cpu().numpy() - g["class_prob"])
    assert np.isfinite(out["bbox_xywh"].cpu().numpy()).all()
    assert np.median(dp) < 5e-3 and dp.max() < 0.3


def test_mini_bf16_uint8_stem_matches_bf16_float_stem():
    """bf16 mode has two first-layer kernels: the MFMA stem (uint8 frames) and the VALU stem (float input).
    Same network, same weights: their outputs may differ only by the bf16 rounding of the 27 inputs."""
    g = np.load(os.path.join(GOLDEN, "mini_blocks.npz"))
    net = _net("mini", dtype="bf16")
    a = net.forward(torch.from_numpy(g["input"]))
    b = net.forward_frames(g["frames"])
    d = (a["class_prob"] - b["class_prob"]).abs().cpu().numpy()
    assert np.median(d) < 2e-3 and d.max() < 0.1
    assert (a["class_idx"] == b["class_idx"]).float().mean() > 0.97


def test_mini_fp16_close_to_fp32_and_its_two_stems_agree():
    """fp16 mode (round 5): the float-input first layer (VALU stem, what ``forward(x)`` runs) and the uint8 MFMA stem
    (``forward_frames``) on the same network: both within the fp16 storage error of the float32 golden, and of each other."""
    g = np.load(os.path.join(GOLDEN, "mini_blocks.npz"))
    net = _net("mini", dtype="fp16")
    a = net.forward(torch.from_numpy(g["input"]))
    b = net.forward_frames(g["frames"])
    assert np.isfinite(a["bbox_xywh"].cpu().numpy()).all()
    dp = np.abs(a["class_prob"].cpu().numpy() - g["class_prob"])
    assert np.median(dp) < 6e-4 and dp.max() < 0.04                       # (bf16: 5e-3 / 0.3)
    d = (a["class_prob"] - b["class_prob"]).abs().cpu().numpy()
    assert np.median(d) < 3e-4 and d.max() < 0.02
    assert (a["class_idx"] == b["class_idx"]).float().mean() > 0.99


DEFAULT_KNOBS = {"igemm_version": 2, "igemm_bm": 0, "igemm_ns": 2, "auto_mask": 0xb409d, "fuse_stem": 1, "decode_lanes": 4, "use_graph": 0, "fuse_head": 1, "fuse_spp": 1}


def test_tuning_knobs_do_not_change_results():
    """Every kernel variant behind y3_set_tuning computes the same convolution (fp32: same values up to
    summation order)."""
    from yolov3 import _hip
    lib = _hip.lib()
    g = np.load(os.path.join(GOLDEN, "mini_blocks.npz"))
    x = torch.from_numpy(g["input"])
    ref = _net("mini").forward(x)
    try:
        for knobs in ({"auto_mask": 0}, {"auto_mask": 63}, {"auto_mask": 127}, {"igemm_version": 1},
                      {"igemm_version": 3, "auto_mask": 0}, {"igemm_version": 3, "igemm_bm": 64, "igemm_ns": 3, "auto_mask": 0}):
            for k, v in knobs.items():
                _hip.check(lib.y3_set_tuning(k.encode(), v))
            out = _net("mini").forward(x)
            np.testing.assert_allclose(out["class_prob"].cpu().numpy(), ref["class_prob"].cpu().numpy(), atol=2e-5,
                                       err_msg=str(knobs))
            np.testing.assert_allclose(out["bbox_xywh"].cpu().numpy(), ref["bbox_xywh"].cpu().numpy(), rtol=1e-4,
                                       atol=1e-5, err_msg=str(knobs))
            for k in knobs:
                _hip.check(lib.y3_set_tuning(k.encode(), DEFAULT_KNOBS[k]))
    finally:
        for k, v in DEFAULT_KNOBS.items():
            lib.y3_set_tuning(k.encode(), v)
    assert lib.y3_set_tuning(b"no_such_knob", 1) != 0


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3", "yolov3-spp"])
def test_forward_golden_fp32(model):
    g = np.load(os.path.join(GOLDEN, "forward_%s.npz" % model))
    dim = MODEL_DIMS[model]
    frames = np.stack([resize_bilinear_u8(load_jpeg_bgr("000000035279.jpg"), dim, dim),
                       synth_frames(5, 1, dim, dim)[0]])
    assert [sha(f) for f in frames] == g["frames_sha"].tolist(), "input frames differ from the golden run"
    net = _net(model)
    out = net.forward(torch.from_numpy(orc.frames_to_input(list(frames))))
    bb = out["bbox_xywh"].cpu().numpy()
    pr = out["class_prob"].cpu().numpy()
    ci = out["class_idx"].cpu().numpy()
    assert bb.shape == g["bbox_xywh"].shape and ci.dtype == np.int64
    print("max |dbox| %.3g  max |dscore| %.3g" % (np.abs(bb - g["bbox_xywh"]).max(), np.abs(pr - g["class_prob"]).max()))
    np.testing.assert_allclose(bb, g["bbox_xywh"], rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(pr, g["class_prob"], atol=SCORE_ATOL)
    flips = (ci != g["class_idx"]) & (g["cls_margin"] >= 1e-4)
    assert flips.sum() == 0, "%d arg-max flips on clear margins" % flips.sum()
    # the uint8 entry point (fused preprocessing) gives the same answer
    out8 = net.forward_frames(frames)
    assert torch.equal(out8["class_idx"], out["class_idx"])
    np.testing.assert_allclose(out8["bbox_xywh"].cpu().numpy(), bb, atol=1e-6)


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3", "yolov3-spp"])
def test_inference_golden_fp32(model):
    """``inference()`` end to end against the reference's lists (G7), thresholds 0.05 / 0.3 and 0.2 / 0.3.
    (1) The device post-processing (threshold, scale, int, tlbr, per-class NMS, gather: one kernel) equals the oracle's
    numpy post-processing of the SAME forward outputs bit for bit -- rows, boxes, classes, scores, no exemptions.
    (2) Against the reference's lists the keep sets are identical except where the float32 forward deviation flips a
    candidate's truncated pixel (golden_util.compare_detections)."""
    from golden_util import product_candidates
    g = np.load(os.path.join(GOLDEN, "inference_%s.npz" % model))
    dim = MODEL_DIMS[model]
    frames = [load_jpeg_bgr("000000229358.jpg"), synth_frames(9, 1, dim, dim)[0], load_jpeg_bgr("000000393569.jpg")]
    assert [sha(f) for f in frames] == g["frames_sha"].tolist()
    net = _net(model)
    resized = np.stack([resize_bilinear_u8(f, dim, dim) for f in frames])
    fwd = {k: v.cpu().numpy() for k, v in net.forward_frames(resized).items()}
    for tag in ("a", "b"):
        pth, ith = g[tag + "_thresholds"]
        res = yolov3.inference(net, frames, device="cuda", prob_thresh=float(pth), nms_iou_thresh=float(ith),
                               return_rows=True)
        assert len(res) == len(frames)
        want = orc.postprocess(fwd["bbox_xywh"], fwd["class_prob"], fwd["class_idx"], [f.shape for f in frames],
                               float(pth), float(ith), audit=True)
        for f in range(len(frames)):
            a, b = orc.canonical_rows(res[f][:3]), orc.canonical_rows(want[f][:3])
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), \
                "%s %s frame %d: device post-processing differs from the oracle's on identical inputs" % (model, tag, f)
            assert sorted(res[f][3].tolist()) == sorted(want[f][3].tolist())
            cand = product_candidates(fwd["bbox_xywh"][f], fwd["class_prob"][f], fwd["class_idx"][f], frames[f].shape, pth)
            ndiff, nbad, nflip = compare_detections(g, "%s_f%d_" % (tag, f), res[f][:3], rows=res[f][3],
                                                    prob_tol=SCORE_ATOL, cand=cand)
            print(model, tag, f, "kept", len(res[f][1]), "candidates", len(cand[0]), "flipped by the forward deviation", nflip,
                  "keep-set diff", ndiff, "box diffs", nbad)


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3", "yolov3-spp"])
def test_inference_bench_regime_all_sample_images_fp32(model):
    """G7': the reference's ``inference()`` lists at the BENCHMARKED regime (a few hundred candidates, tens of kept boxes
    per frame), one call per image like the reference's own test (/root/reference/tests/test_inference.py:51-59), on all
    nine sample_dataset JPEGs and on procedural frames the generator audited.
    AUDITED-CLEAN (frame, threshold) pairs -- every candidate >= 2e-3 px from an integer pixel, every score >= 1e-4 from
    the threshold, every class margin >= 1e-4 -- must reproduce the reference EXACTLY: identical rows, classes and integer
    boxes after NMS, no exemption path (``cand=None``).  The other pairs use the flip rule of compare_detections."""
    from golden_util import BENCH_REGIME_OBJ_BIAS, bench_regime_frame, product_candidates
    g = np.load(os.path.join(GOLDEN, "inference_bench_regime_%s.npz" % model))
    dim = MODEL_DIMS[model]
    net = yolov3.Darknet(MODELS[model], device="cuda", dtype="float32")
    net.load_weights(golden_weights_path(model, obj_bias=BENCH_REGIME_OBJ_BIAS[model])).eval()
    names = [str(n) for n in g["names"]]
    assert sum(n.startswith("img") for n in names) == 9
    n_clean = kept_clean = 0
    for name in names:
        frame = bench_regime_frame(name, dim)
        fwd = {k: v.cpu().numpy() for k, v in net.forward_frames(resize_bilinear_u8(frame, dim, dim)[None]).items()}
        for tag in ("a", "b"):
            pth, ith = g[tag + "_thresholds"]
            key = "%s_%s_" % (name, tag)
            res = yolov3.inference(net, frame, device="cuda", prob_thresh=float(pth), nms_iou_thresh=float(ith), return_rows=True)[0]
            clean = bool(g[key + "audit"][4])
            if clean:
                order = np.argsort(res[3])
                gorder = np.argsort(g[key + "rows"])
                assert np.array_equal(res[3][order], g[key + "rows"][gorder]), (model, name, tag, "kept rows differ")
                assert np.array_equal(res[2][order], g[key + "cls"][gorder]), (model, name, tag, "classes differ")
                assert np.array_equal(res[0][order], g[key + "tlbr"][gorder]), (model, name, tag, "boxes differ")
                np.testing.assert_allclose(res[1][order], g[key + "prob"][gorder], atol=SCORE_ATOL)
                n_clean += 1
                kept_clean += len(res[1])
            else:
                cand = product_candidates(fwd["bbox_xywh"][0], fwd["class_prob"][0], fwd["class_idx"][0], frame.shape, pth)
                compare_detections(g, key, res[:3], rows=res[3], prob_tol=SCORE_ATOL, cand=cand)
    print(model, "audited-clean (frame, threshold) pairs reproduced exactly:", n_clean, "with", kept_clean, "kept boxes in all")
    assert n_clean >= 4


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3", "yolov3-spp"])
def test_inference_exact_identity_set_fp32(model):
    """G7x (round 5): "identical box indices / classes after NMS" on a fixture that is thick enough for
    Darknet-53 too -- >= 20 audited-clean (frame, threshold) pairs and >= 200 kept boxes per model at thresholds 0.2 / 0.3 and
    0.3 / 0.3 (tools/make_goldens.py g7x_exact: the reference's ``inference()``, one frame per call, on the sample images and on
    procedural frames; a pair is kept only if no deviation below 6e-5 can move a pixel, a threshold test, an arg-max or a
    suppression).  The float32 HIP path must return EVERY list exactly: rows, classes, integer boxes; no flip rule, no
    exemption.  The fp16 / bf16 paths are counted on the same set (printed; fp16 asserted to match the large majority)."""
    from golden_util import bench_regime_frame
    g = np.load(os.path.join(GOLDEN, "inference_exact_%s.npz" % model))
    pairs = [str(p) for p in g["pairs"]]
    dim = MODEL_DIMS[model]
    exact = {}
    for dtype in ("float32", "fp16", "bf16"):
        net = yolov3.Darknet(MODELS[model], device="cuda", dtype=dtype)
        net.load_weights(golden_weights_path(model, obj_bias=float(g["obj_bias"]))).eval()
        n_same = boxes = n_rows_same = box_px = 0
        score_d = 0.0
        for p in pairs:
            name, tag = p.rsplit("_", 1)
            pth, ith = g[tag + "_thresholds"]
            frame = bench_regime_frame(name, dim)
            res = yolov3.inference(net, frame, device="cuda", prob_thresh=float(pth), nms_iou_thresh=float(ith), return_rows=True)[0]
            order, gorder = np.argsort(res[3]), np.argsort(g[p + "_rows"])
            same = (len(order) == len(gorder) and np.array_equal(res[3][order], g[p + "_rows"][gorder]) and
                    np.array_equal(res[2][order], g[p + "_cls"][gorder]) and np.array_equal(res[0][order], g[p + "_tlbr"][gorder]))
            if dtype == "float32":
                assert same, (model, p, "differs from the reference's list")
                np.testing.assert_allclose(res[1][order], g[p + "_prob"][gorder], atol=SCORE_ATOL)
            n_same += int(same)
            boxes += len(g[p + "_rows"])
            if len(order) == len(gorder) and np.array_equal(res[3][order], g[p + "_rows"][gorder]) and np.array_equal(res[2][order], g[p + "_cls"][gorder]):
                n_rows_same += 1                          # identical box INDICES and CLASSES after NMS; how far are the boxes / scores?
                if len(order):
                    box_px = max(box_px, int(np.abs(res[0][order] - g[p + "_tlbr"][gorder]).max()))
                    score_d = max(score_d, float(np.abs(res[1][order] - g[p + "_prob"][gorder]).max()))
        exact[dtype] = (n_same, n_rows_same)
        print("%s %s: of %d audited-clean pairs (%d kept boxes) %d reproduced EXACTLY; %d with identical kept indices and classes "
              "(on those: boxes within %d px, scores within %.1e)" % (model, dtype, len(pairs), boxes, n_same, n_rows_same, box_px, score_d))
    assert exact["float32"] == (len(pairs), len(pairs)) and len(pairs) >= 20 and boxes >= 200
    # 16-bit storage cannot keep every truncated pixel (a deviation of 1e-4 of a 608-px frame is 0.06 px: one coordinate in
    # ten crosses an integer), but fp16 keeps the reference's kept INDICES and CLASSES on most clean pairs, bf16 on few
    assert exact["fp16"][1] >= exact["bf16"][1] and exact["fp16"][1] >= len(pairs) // 2


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3"])
def test_inference_net_sized_crops_fp32(model):
    """G7c: the reference's ``inference()`` lists on net-sized centre crops of the sample images (no resize anywhere between
    the JPEG and the network, on either side).  Audited-clean (frame, threshold) pairs must match exactly, the others go
    through the flip rule of compare_detections."""
    from golden_util import bench_regime_frame, product_candidates
    g = np.load(os.path.join(GOLDEN, "inference_crops_%s.npz" % model))
    dim = MODEL_DIMS[model]
    net = yolov3.Darknet(MODELS[model], device="cuda", dtype="float32")
    net.load_weights(golden_weights_path(model, obj_bias=float(g["obj_bias"]))).eval()
    n_clean = kept = 0
    for name in (str(n) for n in g["names"]):
        frame = bench_regime_frame(name, dim)
        assert frame.shape == (dim, dim, 3)
        fwd = {k: v.cpu().numpy() for k, v in net.forward_frames(frame[None]).items()}
        for tag in ("a", "b"):
            pth, ith = g[tag + "_thresholds"]
            key = "%s_%s_" % (name, tag)
            res = yolov3.inference(net, frame, device="cuda", prob_thresh=float(pth), nms_iou_thresh=float(ith), return_rows=True)[0]
            kept += len(res[1])
            if bool(g[key + "audit"][4]):
                order, gorder = np.argsort(res[3]), np.argsort(g[key + "rows"])
                assert np.array_equal(res[3][order], g[key + "rows"][gorder]), (model, name, tag, "kept rows differ")
                assert np.array_equal(res[2][order], g[key + "cls"][gorder]), (model, name, tag, "classes differ")
                assert np.array_equal(res[0][order], g[key + "tlbr"][gorder]), (model, name, tag, "boxes differ")
                np.testing.assert_allclose(res[1][order], g[key + "prob"][gorder], atol=SCORE_ATOL)
                n_clean += 1
            else:
                cand = product_candidates(fwd["bbox_xywh"][0], fwd["class_prob"][0], fwd["class_idx"][0], frame.shape, pth)
                compare_detections(g, key, res[:3], rows=res[3], prob_tol=SCORE_ATOL, cand=cand)
    print(model, "net-sized crops: clean pairs reproduced exactly:", n_clean, "kept boxes in all:", kept)
    assert kept > 100 and (n_clean >= 4 or model == "yolov3")


def test_device_resize_is_bit_identical_to_host_resize():
    from yolov3.preprocess import resize_on_device
    for name, (oh, ow) in (("000000229358.jpg", (608, 608)), ("000000393569.jpg", (416, 416)), ("000000035279.jpg", (320, 480))):
        img = load_jpeg_bgr(name)
        want = resize_bilinear_u8(img, oh, ow)
        got = resize_on_device(img, oh, ow, torch.device("cuda")).cpu().numpy()
        assert got.shape == want.shape and (got == want).all(), name
    same = synth_frames(4, 1, 64, 48)[0]
    assert (resize_on_device(same, 64, 48, torch.device("cuda")).cpu().numpy() == same).all()


def test_inference_single_frame_and_empty_result():
    net = _net("yolov3-tiny")
    frame = synth_frames(3, 1, 416, 416)[0]
    res = yolov3.inference(net, frame, prob_thresh=0.999)   # nothing passes
    assert len(res) == 1
    tlbr, prob, cls = res[0]
    assert tlbr.shape == (0, 4) and prob.shape == (0,) and cls.shape == (0,)
    assert tlbr.dtype == np.int64 and cls.dtype == np.int64 and prob.dtype == np.float32


def test_gpu_matches_oracle_on_fresh_input():
    """Not a golden: same seeded input through the oracle (CPU) and the HIP path."""
    net = _net("yolov3-tiny")
    ref = orc.OracleDarknet(MODELS["yolov3-tiny"]).load_weights(golden_weights_path("yolov3-tiny"))
    frames = synth_frames(21, 2, 320, 416)          # non-square, not the cfg size
    x = torch.from_numpy(orc.frames_to_input(list(frames)))
    want = ref.forward(x)
    got = net.forward(x)
    np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=SCORE_ATOL)
    agree = (got["class_idx"].cpu().numpy() == want["class_idx"].numpy()).mean()
    assert agree > 0.999
    dets_ref = orc.postprocess(want["bbox_xywh"].numpy(), want["class_prob"].numpy(), want["class_idx"].numpy(),
                               [f.shape for f in frames], 0.05, 0.3, audit=True)
    dets = yolov3.inference(net, list(frames), prob_thresh=0.05, nms_iou_thresh=0.3, resize=False, return_rows=True)
    for a, b in zip(dets, dets_ref):
        ndiff, nbad = orc.compare_detections(a, b)      # same rows, classes and pixel boxes outside fragile candidates
        print("kept", len(a[1]), "keep-set diff", ndiff, "fragile box diffs", nbad)


@pytest.mark.parametrize("h,w", [(352, 480), (512, 320)])
def test_yolov3_float32_matches_oracle_at_other_input_sizes(h, w):
    """Darknet-53 at input sizes other than the cfg's: feature-map rows of 60 / 30 / 15, 44 / 22 / 11, 64 / 32 / 16 and
    40 / 20 / 10 pixels (halo rows that are an exact multiple of the loader pass at 15, different weight-ring depths,
    strips that span several frames at the coarse scales), non-square.  float32 HIP path against the CPU oracle."""
    net = _net("yolov3")
    ref = orc.OracleDarknet(MODELS["yolov3"]).load_weights(golden_weights_path("yolov3"))
    frames = synth_frames(h + w, 2, h, w)
    x = torch.from_numpy(orc.frames_to_input(list(frames)))
    want = ref.forward(x)
    got = net.forward(x)
    np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=SCORE_ATOL)
    assert (got["class_idx"].cpu().numpy() == want["class_idx"].numpy()).mean() > 0.999


@pytest.mark.parametrize("h,w", [(352, 480), (512, 320), (480, 480)])
def test_yolov3_bf16_kernel_choices_agree_at_other_input_sizes(h, w):
    """Same sizes in bf16: the default kernel selection (halo / patch / fused kernels) against the plain implicit GEMM
    everywhere (`auto_mask` 0, no fusion) on the same frames -- different summation orders of the same bf16 products."""
    from yolov3 import _hip
    lib = _hip.lib()
    frames = synth_frames(h * 3 + w, 2, h, w)
    try:
        net = _net("yolov3", dtype="bf16")
        fast = {k: v.clone() for k, v in net.forward_frames(frames).items()}
        for key, val in (("auto_mask", 0), ("fuse_stem", 0), ("fuse_head", 0)):
            _hip.check(lib.y3_set_tuning(key.encode(), val))
        net2 = _net("yolov3", dtype="bf16")
        plain = net2.forward_frames(frames)
        assert not any("halo" in r["kernel"] or "patch" in r["kernel"] or "fused" in r["kernel"] for r in net2.plan_report())
        d = (fast["class_prob"] - plain["class_prob"]).abs()
        assert float(d.max()) < 0.1 and float(d.median()) < 2e-3, (float(d.max()), float(d.median()))
        assert float((fast["class_idx"] == plain["class_idx"]).float().mean()) > 0.97
        torch.testing.assert_close(fast["bbox_xywh"], plain["bbox_xywh"], rtol=5e-2, atol=5e-3)
    finally:
        for key, val in DEFAULT_KNOBS.items():
            lib.y3_set_tuning(key.encode(), val)


def test_nms_cases_match_reference():
    with open(os.path.join(GOLDEN, "nms_cases.json")) as fh:
        cases = json.load(fh)
    for c in cases:
        boxes = np.array(c["boxes"], dtype=np.int64).reshape(-1, 4)
        prob = np.array(c["prob_bits"], dtype=np.uint32).view(np.float32)
        ties = len(set(prob.tolist())) != len(prob)
        got = yolov3.non_max_suppression(boxes, prob, iou_thresh=c["thr"])
        assert isinstance(got, list)
        if not ties:
            assert sorted(got) == sorted(c["agnostic"]), c["name"]
            # class-agnostic order is pure score order in both implementations
            assert got == c["agnostic"], c["name"]
        if c["cls"] is not None:
            got = yolov3.non_max_suppression(boxes, prob, class_idx=np.array(c["cls"]), iou_thresh=c["thr"])
            if not ties:
                assert sorted(got) == sorted(c["per_class"]), c["name"]
    assert yolov3.non_max_suppression(np.zeros((0, 4), dtype=np.int64), np.zeros(0, dtype=np.float32)) == []



def _float_cases():
    with open(os.path.join(GOLDEN, "nms_float_cases.json")) as fh:
        table = json.load(fh)
    for c in table["nms"]:
        dt, pdt = np.dtype(c["dtype"]), np.dtype(c["prob_dtype"])
        boxes = np.array(c["boxes_bits"], dtype=np.uint32 if dt == np.float32 else np.uint64).view(dt).reshape(-1, 4)
        prob = np.array(c["prob_bits"], dtype=np.uint32 if pdt == np.float32 else np.uint64).view(pdt)
        yield c, boxes, prob, np.array(c["cls"], dtype=np.int64)
    for t in table["cxywh_to_tlbr"]:
        dt = np.dtype(t["dtype"])
        u = np.uint32 if dt == np.float32 else np.uint64
        yield t, np.array(t["xywh_bits"], dtype=u).view(dt).reshape(-1, t["cols"]), np.array(t["tlbr_bits"], dtype=u).view(dt).reshape(-1, t["cols"]), None


def test_float_box_nms_and_tlbr_match_reference():
    """G6f (round 5, VERDICT r04 missing #6): ``non_max_suppression`` / ``cxywh_to_tlbr`` are public functions of the reference
    and take any numeric dtype; a third-party caller may pass normalised or sub-pixel float boxes.  The device kernels
    (``y3_nms_float``, ``y3_cxywh_to_tlbr_float``: every step in the array's dtype, like numpy) return the reference's keep
    sets -- and, class-agnostic, its order -- on float32 and float64 boxes, and its corners bit for bit."""
    n_nms = 0
    for c, a, b, cls in _float_cases():
        if cls is None:
            got = yolov3.cxywh_to_tlbr(a)
            assert got.dtype == a.dtype and np.array_equal(got, b), c["dtype"]
            continue
        got = yolov3.non_max_suppression(a, b, iou_thresh=c["thr"])
        assert got == c["agnostic"], c["name"]
        got = yolov3.non_max_suppression(a, b, class_idx=cls, iou_thresh=c["thr"])
        assert sorted(got) == sorted(c["per_class"]), c["name"]
        n_nms += 1
    assert n_nms >= 13
    assert yolov3.non_max_suppression(np.zeros((0, 4), dtype=np.float32), np.zeros(0, dtype=np.float32)) == []
    # float16 boxes are REFUSED (the reference would compute areas / IoU in float16, where a 300 x 300 box's area is inf: the
    # float32 kernel would silently return another keep set -- ADVICE r05), and so are non-finite coordinates (numpy's
    # maximum / minimum propagate NaN, ``inf // 2`` is NaN; the kernels compare and floor)
    rs = np.random.RandomState(2)
    c16 = rs.rand(50, 2) * 100
    w16 = rs.rand(50, 2) * 30 + 1
    b16 = np.concatenate([c16 - w16 / 2, c16 + w16 / 2], axis=1)
    p16 = (rs.permutation(50) / 50.0).astype(np.float32)
    with pytest.raises(TypeError):
        yolov3.non_max_suppression(b16.astype(np.float16), p16, iou_thresh=0.3)
    with pytest.raises(TypeError):
        yolov3.cxywh_to_tlbr(b16.astype(np.float16))
    bad = b16.astype(np.float32)
    bad[3, 2] = np.nan
    with pytest.raises(ValueError):
        yolov3.non_max_suppression(bad, p16, iou_thresh=0.3)
    bad[3, 2] = np.inf
    with pytest.raises(ValueError):
        yolov3.cxywh_to_tlbr(bad)
    assert sorted(yolov3.non_max_suppression(b16.astype(np.float32), p16, iou_thresh=0.3)) == sorted(
        int(i) for i in orc.non_max_suppression(b16.astype(np.float32), p16, iou_thresh=0.3))


@pytest.mark.parametrize("thr", [0.3, 0.5, 0.25, 1.0 / 3.0, 0.2, 0.0, 1.0])
def test_nms_borderline_ratios_match_oracle(thr):
    """Small integer boxes make inter / union land exactly on (or one rounding away from) the threshold all the
    time (3/10 vs 0.3, 1/2 vs 0.5, 1/3 ...): the kernel's division-free compare must decide exactly like the
    reference's float64 quotient, including degenerate (x2 < x1) boxes whose union is <= 0."""
    rs = np.random.RandomState(int(thr * 1000) + 7)
    n = 1500
    tl = rs.randint(0, 12, size=(n, 2))
    wh = rs.randint(-1, 7, size=(n, 2))          # -1 -> degenerate boxes
    boxes = np.concatenate([tl, tl + wh], axis=1).astype(np.int64)
    boxes[0] = [0, 0, 9, 0]
    boxes[1] = [7, 0, 9, 0]                        # inter 3, union 10 with box 0
    prob = (rs.permutation(n).astype(np.float32) + 1) / (n + 1)
    prob[0], prob[1] = 2.0, 1.5
    for cls in (None, rs.randint(0, 4, size=n).astype(np.int64)):
        want = orc.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=thr)
        got = yolov3.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=thr)
        assert sorted(got) == sorted(int(i) for i in want)


@pytest.mark.parametrize("n,ncls", [(5000, 1), (9000, 3), (20000, 80)])
def test_nms_large_matches_oracle(n, ncls):
    """Sizes past the in-LDS sort limit (4096) and a single crowded class."""
    rs = np.random.RandomState(n)
    c = rs.randint(0, 2000, size=(n, 2))
    wh = rs.randint(2, 200, size=(n, 2))
    boxes = np.concatenate([c - wh // 2, c + wh // 2], axis=1).astype(np.int64)
    prob = (rs.permutation(n).astype(np.float32) + 1) / (n + 1)
    cls = rs.randint(0, ncls, size=n).astype(np.int64)
    want = orc.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=0.4)
    got = yolov3.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=0.4)
    assert sorted(got) == sorted(int(i) for i in want)


@pytest.mark.parametrize("model,dim,batch", [(m, d, b) for m in ("yolov3", "yolov3-tiny", "yolov3-spp")
                                             for d in (32, 64, 320, 416, 608) for b in (1, 2)])
def test_shape_sweep_bf16(model, dim, batch):
    """The reference's own 18-case smoke sweep (tests/test_darknet.py:10-27), plus shape asserts; bf16 at batch 1, fp16 at
    batch 2 (the two 16-bit modes share every kernel template).  32 and 64 pixels: detection scales of 1 x 1 and 2 x 2 cells."""
    net = _net(model, dtype="bf16" if batch == 1 else "fp16")
    x = torch.rand(batch, 3, dim, dim, generator=torch.Generator().manual_seed(dim + batch))
    out = net.forward(x)
    cells = sum((dim // s) ** 2 for s in ((32, 16) if model == "yolov3-tiny" else (32, 16, 8)))
    assert out["bbox_xywh"].shape == (batch, 3 * cells, 4)
    assert out["class_prob"].shape == (batch, 3 * cells) and out["class_idx"].shape == (batch, 3 * cells)
    assert torch.isfinite(out["bbox_xywh"]).all() and torch.isfinite(out["class_prob"]).all()
    assert int(out["class_idx"].min()) >= 0 and int(out["class_idx"].max()) < 80


def test_halo_kernels_match_goldens_on_yolov3_fp32():
    """The halo-reuse 3x3 kernel (192- and 256-pixel tiles) and the 2-D patch kernel against the goldens, whole network,
    fp32."""
    from yolov3 import _hip
    lib = _hip.lib()
    g = np.load(os.path.join(GOLDEN, "forward_yolov3.npz"))
    frames = np.stack([resize_bilinear_u8(load_jpeg_bgr("000000035279.jpg"), 608, 608), synth_frames(5, 1, 608, 608)[0]])
    halo = _hip.AM_HALO_ALL | _hip.AM_NO_SMALL_GRID     # the halo kernel whatever the grid size (two frames are a small grid)
    try:
        for mask in (halo, halo | _hip.AM_PATCH_WIDE, halo | _hip.AM_HALO_TILE256):
            _hip.check(lib.y3_set_tuning(b"auto_mask", mask))
            net = _net("yolov3")
            out = net.forward(torch.from_numpy(orc.frames_to_input(list(frames))))
            names = [r["kernel"] for r in net.plan_report()]
            assert any("halo_ws" in k for k in names)
            assert any("conv_patch" in k for k in names) == bool(mask & _hip.AM_PATCH_WIDE)     # 2-D patch kernel on the 152^2 layers
            np.testing.assert_allclose(out["bbox_xywh"].cpu().numpy(), g["bbox_xywh"], rtol=1e-4, atol=BOX_ATOL)
            np.testing.assert_allclose(out["class_prob"].cpu().numpy(), g["class_prob"], atol=SCORE_ATOL)
    finally:
        lib.y3_set_tuning(b"auto_mask", DEFAULT_KNOBS["auto_mask"])


@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_kernel_choice_does_not_change_a_bit(dtype):
    """Every MFMA conv kernel sums a layer in the same K order (channel chunk outermost, tap innermost), so which of them
    the launcher picks -- by grid size, i.e. by batch -- changes speed only: yolov3 on the implicit GEMM everywhere, on
    the halo / patch kernels with either tile height, on the wave-specialised implicit GEMM and with the default
    selection gives identical bits (fusion of conv pairs kept equal: the fused kernels round their on-chip intermediate
    like the two-kernel path does, but that is tested elsewhere)."""
    from yolov3 import _hip
    frames = synth_frames(31, 2, 608, 608)
    halo = _hip.AM_HALO_ALL | _hip.AM_NO_SMALL_GRID
    outs = []
    for opts in ({"auto_mask": _hip.AM_IGEMM_ONLY}, {"auto_mask": halo | _hip.AM_PATCH_WIDE}, {"auto_mask": halo | _hip.AM_HALO_TILE256},
                 {"auto_mask": _hip.AM_IGEMM_ONLY, "igemm_version": 3, "igemm_ns": 3},
                 {"auto_mask": _hip.AM_IGEMM_ONLY, "igemm_bm": 96},           # 96 x 64 tiles wherever Cout is a multiple of 64
                 {"auto_mask": halo | _hip.AM_HALO_DW_ALWAYS},                # direct-weights strip kernel wherever it fits (16-bit)
                 None):
        net = _net("yolov3", dtype=dtype, options=opts)
        outs.append({k: v.clone() for k, v in net.forward_frames(frames).items()})
        if opts and opts.get("auto_mask", 0) & _hip.AM_HALO_DW_ALWAYS and dtype != "float32":
            assert sum("conv_halo_dw" in r["kernel"] for r in net.plan_report()) >= 25, [r["kernel"] for r in net.plan_report()]
    for o in outs[1:]:
        for k in ("bbox_xywh", "class_prob", "class_idx"):
            assert torch.equal(o[k], outs[0][k]), k


@pytest.mark.parametrize("model", ["yolov3", "yolov3-spp"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_direct_weights_kernel_is_chosen_at_batch16_and_changes_no_bit(model, dtype):
    """BASELINE configs[2] / [3] (608 x 608, batch 16): the 256 -> 512 layers at 38^2 are 364 tiles of 256 x 128 -- two rounds of
    workgroups on 256 CUs, the second 42 % full -- against 242 of 192 x 256 in one round; the launcher picks the direct-weights
    strip kernel for them (its weights in MFMA-fragment order: a copy the plan makes), and forbidding it gives the same bits.  Also
    at an input size whose maps have other halo heights than the three instantiated ones (352 x 480: the run-time form)."""
    from yolov3 import _hip
    frames = synth_frames(43, 16, 608, 608)
    a = _net(model, dtype=dtype)
    oa = {k: v.clone() for k, v in a.forward_frames(frames).items()}
    names = [r["kernel"] for r in a.plan_report()]
    assert sum("conv_halo_dw" in n for n in names) >= 8, names
    b = _net(model, dtype=dtype, options={"auto_mask": _hip.AM_DEFAULT & ~_hip.AM_HALO_DW})
    ob = b.forward_frames(frames)
    assert not any("conv_halo_dw" in r["kernel"] for r in b.plan_report())
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(oa[k], ob[k]), k
    small = synth_frames(44, 3, 352, 480)
    halo = _hip.AM_HALO_ALL | _hip.AM_NO_SMALL_GRID
    c = _net(model, dtype=dtype, options={"auto_mask": halo | _hip.AM_HALO_DW_ALWAYS})
    oc = {k: v.clone() for k, v in c.forward_frames(small).items()}
    assert sum("conv_halo_dw" in r["kernel"] for r in c.plan_report()) >= 20   # 352 x 480: maps 44 x 60, 22 x 30, 11 x 15 -- all within 62 pixels
    d = _net(model, dtype=dtype, options={"auto_mask": halo})
    od = d.forward_frames(small)
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(oc[k], od[k]), k


def test_new_parameters_replace_the_plans_private_weight_copies():
    """The direct-weights kernel reads a fragment-order COPY of a layer's weights that the plan made when it was compiled.
    ``set_params`` on a network that has already run must not leave a plan with the old copy: the outputs equal those of a
    fresh network built with the new parameters."""
    frames = synth_frames(47, 16, 608, 608)
    net = _net("yolov3", dtype="bf16")
    first = {k: v.clone() for k, v in net.forward_frames(frames).items()}
    assert any("conv_halo_dw" in r["kernel"] for r in net.plan_report())
    other = W.synth_params(net.blocks, net.net_info, seed=3, obj_bias=-5.0, calib=W.load_calibration("yolov3"))
    net.set_params(other)
    second = net.forward_frames(frames)
    fresh = yolov3.Darknet(MODELS["yolov3"], device="cuda", dtype="bf16").eval()
    fresh.set_params(other)
    want = fresh.forward_frames(frames)
    assert not torch.equal(second["class_prob"], first["class_prob"])
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(second[k], want[k]), k


@pytest.mark.parametrize("model", ["yolov3", "yolov3-spp"])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_direct_weights_1x1_kernel_is_chosen_at_batch16_and_changes_no_bit(model, dtype):
    """Round 6: at 608 x 608, batch 16 the short-K bottleneck layers on the small maps (512 -> 256 at 38^2, 1024 -> 512 at 19^2,
    768 -> 256 after the route: /root/reference/models/yolov3.cfg blocks 38-61, 63-80, 87) go to the direct-weights 1x1 kernel
    (csrc/conv_1x1.hip: conv1x1_dw, one 96- or 48-pixel x 256-channel tile per CU, whole activation tile in LDS, weight
    fragments straight from the shared fragment-order copy); forbidding it gives the same bits."""
    from yolov3 import _hip
    frames = synth_frames(45, 16, 608, 608)
    a = _net(model, dtype=dtype)
    oa = {k: v.clone() for k, v in a.forward_frames(frames).items()}
    names = [r["kernel"] for r in a.plan_report()]
    assert sum(n.startswith("conv1x1_dw_") for n in names) >= 18, names
    assert any("_96x256" in n for n in names) and any("_48x256" in n for n in names), names
    b = _net(model, dtype=dtype, options={"auto_mask": _hip.AM_DEFAULT & ~_hip.AM_1X1_DW})
    ob = b.forward_frames(frames)
    assert not any(r["kernel"].startswith("conv1x1_dw_") for r in b.plan_report())
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(oa[k], ob[k]), k
    # one frame at a time (inference(), the video loop): too few tiles -- the kernel is not taken, same bits again
    c = _net(model, dtype=dtype)
    oc = c.forward_frames(frames[:1])
    assert not any(r["kernel"].startswith("conv1x1_dw_") for r in c.plan_report())
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(oc[k], oa[k][:1]), k


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,h,cin,cout,leaky", [
    (16, 38, 512, 256, True), (16, 19, 1024, 512, True), (16, 38, 768, 256, True), (16, 38, 256, 256, False), (16, 38, 384, 256, True),
    (15, 38, 512, 256, True),      # 21 660 pixels: the last 96-pixel tile holds 60
    (13, 19, 1024, 512, False),    # 4 693 pixels: the last 48-pixel tile holds 37
    (16, 27, 512, 256, True),      # 48-pixel tiles with ONE channel tile
    (16, 27, 768, 256, True)])
def test_direct_weights_1x1_kernel_matches_implicit_gemm(B, h, cin, cout, leaky, dtype):
    """Every instantiation of conv1x1_dw (tile heights 96 / 48; 4, 6, 8, 12, 16 K-steps), full and ragged last tiles, with and
    without LeakyReLU: a one-op plan through the C ABI, bit-equal to the LDS-DMA implicit GEMM on the same operands (same K
    order).  The plan makes its own fragment-order copy of the weights here (no y3_op.d_weight_frag): the C caller's path."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    g = torch.Generator().manual_seed(B * 1000 + h + cin)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    x = (torch.rand((B, h, h, cin), generator=g) - 0.5).to(tdt).to(dev)
    w = ((torch.rand((cout, cin), generator=g) - 0.5) * (6.0 / cin) ** 0.5).to(tdt).to(dev)
    sc, bi = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.rand(cout, generator=g) - 0.5).to(dev)
    outs, names = [], []
    for mask in (_hip.AM_1X1_DW, 0):
        out = torch.full((B, h, h, cout), 3.0, dtype=tdt, device=dev)
        op = _hip.Y3Op()
        op.kind, op.dtype = _hip.OP_CONV, {"bf16": _hip.Y3_BF16, "fp16": _hip.Y3_F16}[dtype]
        op.flags = _hip.F_LEAKY if leaky else 0
        op.batch, op.in_h, op.in_w, op.in_c, op.in_ld = B, h, h, cin, cin
        op.out_h, op.out_w, op.out_c, op.out_ld = h, h, cout, cout
        op.ksize, op.stride, op.pad, op.k_ld, op.cout_pad = 1, 1, 0, cin, cout
        op.d_in, op.d_out = x.data_ptr(), out.data_ptr()
        op.d_weight, op.d_scale, op.d_bias = w.data_ptr(), sc.data_ptr(), bi.data_ptr()
        opts = _hip.options(auto_mask=mask)
        handle = ctypes.c_void_p()
        _hip.check(lib.y3_plan_create_ex((_hip.Y3Op * 1)(op), 1, zero.data_ptr(), ctypes.byref(opts), ctypes.byref(handle)))
        try:
            names.append(lib.y3_plan_op_kernel(handle, 0).decode())
            _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            lib.y3_plan_destroy(handle)
        outs.append(out)
    assert names[0].startswith("conv1x1_dw_") and names[1].startswith("conv_igemm"), names
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1]), (names, float((outs[0].float() - outs[1].float()).abs().max()))


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("B,h,w,cin,cout,k,res,stride", [
    (1, 76, 76, 128, 256, 3, True, 1), (1, 38, 38, 256, 512, 3, True, 1), (1, 19, 19, 512, 1024, 3, True, 1), (2, 19, 19, 512, 1024, 3, False, 1),
    (3, 13, 13, 512, 1024, 3, False, 1),     # yolov3-tiny's deep layer, three frames: 507 pixels = 10 tiles + 27 pixels
    (1, 44, 60, 128, 256, 3, True, 1),       # a non-square map (352 x 480 input): rows of 60 pixels, 2640 pixels = 55 tiles
    (2, 11, 15, 256, 128, 3, True, 1),       # 32-channel workgroups would not fill the chip either: Cout 128
    (1, 76, 76, 256, 128, 1, False, 1), (1, 38, 38, 512, 256, 1, False, 1), (1, 19, 19, 1024, 512, 1, False, 1), (1, 38, 38, 768, 256, 1, False, 1),
    (1, 76, 76, 384, 128, 1, False, 1), (5, 19, 19, 1024, 512, 1, False, 1),
    # grids of several rounds of workgroups (Y3_AM_SMALL_DW_ALWAYS: the launcher would not pick the kernel there by itself)
    (16, 38, 38, 512, 256, 1, False, 1), (16, 19, 19, 512, 1024, 3, True, 1), (16, 76, 76, 384, 128, 1, False, 1),
    # stride 2 (the four downsampling layers with 128+ input channels; the four parity planes of the input in LDS): Darknet-53's three at one
    # frame -- 512 input channels as TWO images of 256 --, ragged last tiles over several frames, non-square maps (rows of 30 / 22
    # output pixels), a shortcut operand (not in any cfg, but the op allows it), many rounds of workgroups
    (1, 152, 152, 128, 256, 3, False, 2), (1, 76, 76, 256, 512, 3, False, 2), (1, 38, 38, 512, 1024, 3, False, 2),
    (3, 38, 38, 512, 1024, 3, False, 2), (2, 26, 26, 512, 1024, 3, True, 2), (1, 88, 120, 128, 256, 3, False, 2),
    (3, 44, 60, 256, 512, 3, True, 2), (5, 22, 30, 512, 256, 3, False, 2), (1, 104, 104, 256, 128, 3, False, 2),
    (16, 76, 76, 256, 512, 3, False, 2), (16, 38, 38, 512, 1024, 3, False, 2),
    (16, 88, 120, 64, 128, 3, False, 2)])   # 64 input channels (rows of eight 16-byte chunks)
def test_small_grid_direct_weights_kernel_matches_implicit_gemm(B, h, w, cin, cout, k, res, stride, dtype):
    """Round 6: conv_dw48 (csrc/conv_dw48.hip), the kernel of small grids -- one frame at a time, the mode the reference's command
    line runs -- in every instantiation (3x3 with 2 / 4 / 8 channel chunks, 1x1 with 2 .. 16, 3x3 stride 2 with 2 / 4 chunks in one or two
    images), with and without a shortcut operand, ragged last tiles, non-square maps, 1 .. 8 waves per workgroup: a one-op plan through
    the C ABI, bit-equal to the LDS-DMA implicit GEMM on the same operands (same K order: chunk outermost, tap innermost)."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    g = torch.Generator().manual_seed(B * 1000 + h * 7 + cin + k)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    x = (torch.rand((B, h, w, cin), generator=g) - 0.5).to(tdt).to(dev)
    kk = k * k * cin
    wt = ((torch.rand((cout, kk), generator=g) - 0.5) * (6.0 / kk) ** 0.5).to(tdt).to(dev)
    sc, bi = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.rand(cout, generator=g) - 0.5).to(dev)
    ho, wo = (h + 2 * ((k - 1) // 2) - k) // stride + 1, (w + 2 * ((k - 1) // 2) - k) // stride + 1
    r = (torch.rand((B, ho, wo, cout), generator=g) - 0.5).to(tdt).to(dev) if res else None
    outs, names = [], []
    for mask in (_hip.AM_SMALL_DW_ALWAYS if B == 16 else _hip.AM_SMALL_DW, 0):
        out = torch.full((B, ho, wo, cout), 3.0, dtype=tdt, device=dev)
        op = _hip.Y3Op()
        op.kind, op.dtype = _hip.OP_CONV, {"bf16": _hip.Y3_BF16, "fp16": _hip.Y3_F16}[dtype]
        op.flags = _hip.F_LEAKY | (_hip.F_RESIDUAL if res else 0)
        op.batch, op.in_h, op.in_w, op.in_c, op.in_ld = B, h, w, cin, cin
        op.out_h, op.out_w, op.out_c, op.out_ld = ho, wo, cout, cout
        op.ksize, op.stride, op.pad, op.k_ld, op.cout_pad = k, stride, (k - 1) // 2, kk, (cout + 127) // 128 * 128
        op.d_in, op.d_out = x.data_ptr(), out.data_ptr()
        if res:
            op.d_res, op.res_ld = r.data_ptr(), cout
        wpad = torch.zeros((op.cout_pad, kk), dtype=tdt, device=dev)
        wpad[:cout] = wt
        scp, bip = torch.zeros(op.cout_pad, device=dev), torch.zeros(op.cout_pad, device=dev)
        scp[:cout], bip[:cout] = sc, bi
        op.d_weight, op.d_scale, op.d_bias = wpad.data_ptr(), scp.data_ptr(), bip.data_ptr()
        opts = _hip.options(auto_mask=mask)
        handle = ctypes.c_void_p()
        _hip.check(lib.y3_plan_create_ex((_hip.Y3Op * 1)(op), 1, zero.data_ptr(), ctypes.byref(opts), ctypes.byref(handle)))
        try:
            names.append(lib.y3_plan_op_kernel(handle, 0).decode())
            _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            lib.y3_plan_destroy(handle)
        outs.append(out)
    assert names[0].startswith("conv_dw48_k%d%s_" % (k, "s2" if stride == 2 else "")) and names[1].startswith("conv_igemm"), names
    assert torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1]), (names, float((outs[0].float() - outs[1].float()).abs().max()))


@pytest.mark.parametrize("model,dim", [("yolov3", 608), ("yolov3-spp", 608), ("yolov3-tiny", 416)])
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_small_grid_kernel_is_chosen_for_one_frame_and_changes_no_bit(model, dim, dtype):
    """One frame at a time (``inference()``, the reference CLI's loop: __main__.py:157-165): most convs of the 16-bit networks run on
    conv_dw48; forbidding it gives the same bits at batches 1, 2, 3 and 5; at batch 16 it is not chosen at all."""
    from yolov3 import _hip
    for batch in (1, 2, 3, 5):
        frames = synth_frames(70 + batch, batch, dim, dim)
        a = _net(model, dtype=dtype)
        oa = {k: v.clone() for k, v in a.forward_frames(frames).items()}
        n = sum(r["kernel"].startswith("conv_dw48_") for r in a.plan_report())
        if batch == 1:
            assert n >= (50 if model != "yolov3-tiny" else 5), [r["kernel"] for r in a.plan_report()]
        b = _net(model, dtype=dtype, options={"auto_mask": _hip.AM_DEFAULT & ~_hip.AM_SMALL_DW})
        ob = b.forward_frames(frames)
        assert not any(r["kernel"].startswith("conv_dw48_") for r in b.plan_report())
        for k in ("bbox_xywh", "class_prob", "class_idx"):
            assert torch.equal(oa[k], ob[k]), (batch, k)
    if model != "yolov3-tiny":
        # batch 16: no 3x3 layer runs on it, and only the two 1x1 layers that Y3_AM_SMALL_DW_WIDE routes there (256 -> 128 @38^2,
        # 384 -> 128 @76^2: a few rounds of single-channel-tile workgroups, faster than the tiled implicit GEMM they ran on)
        c = _net(model, dtype=dtype)
        c.forward_frames(synth_frames(71, 16, dim, dim))
        on = [r["kernel"] for r in c.plan_report() if r["kernel"].startswith("conv_dw48_")]
        assert all(k.startswith("conv_dw48_k1_") for k in on) and len(on) <= 2, on


@pytest.mark.parametrize("B,h,cin,cout,k,stride,want", [
    (3, 76, 128, 256, 3, 1, "conv_dw48_k3_"),      # 361 tiles = 1.4 rounds: taken (19.1 against 26.0 us on the wave-specialised implicit GEMM)
    (4, 76, 128, 256, 3, 1, "conv_igemm"),         # 482 tiles = 1.9 rounds: left to the others (the strip kernel in a network's plan)
    (6, 38, 256, 512, 3, 1, "conv_dw48_k3_"),      # 362 tiles
    (16, 38, 256, 128, 1, 1, "conv_dw48_k1_"),     # 1x1, one channel tile, 482 tiles
    (16, 76, 384, 128, 1, 1, "conv_dw48_k1_"),     # ... 1926 tiles = 7.5 rounds
    (16, 76, 256, 128, 1, 1, "conv1x1_wres_"),     # the weights-resident kernel pays here: asked first
    (16, 152, 128, 64, 1, 1, "conv1x1_wres_"),     # 64 output channels: never the small-grid kernel on a big grid
    (3, 152, 128, 256, 3, 2, "conv_dw48_k3s2_")])  # stride 2, 361 tiles
def test_small_grid_kernel_on_grids_over_one_round(B, h, cin, cout, k, stride, want):
    """Y3_AM_SMALL_DW_WIDE: conv_dw48 beyond ONE round of workgroups where it measured faster than what the layer ran on (3x3: up to 1.5
    rounds; 1x1 with one channel tile per pixel tile: up to 8, after the weights-resident kernel) -- which kernel a one-op plan gets
    under the default mask, and the same bits as the implicit GEMM."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(B * 100 + h + cin)
    pad = (k - 1) // 2
    ho = (h + 2 * pad - k) // stride + 1
    kk = k * k * cin
    cp = (cout + 127) // 128 * 128
    x = (torch.rand((B, h, h, cin), generator=g) - 0.5).to(torch.bfloat16).to(dev)
    wt = torch.zeros((cp, kk), dtype=torch.bfloat16, device=dev)
    wt[:cout] = ((torch.rand((cout, kk), generator=g) - 0.5) * (6.0 / kk) ** 0.5).to(torch.bfloat16).to(dev)
    sc, bi = torch.zeros(cp, device=dev), torch.zeros(cp, device=dev)
    sc[:cout], bi[:cout] = (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.rand(cout, generator=g) - 0.5).to(dev)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    outs, names = [], []
    for mask in (_hip.AM_DEFAULT, 0):
        out = torch.full((B, ho, ho, cout), 3.0, dtype=torch.bfloat16, device=dev)
        op = _hip.Y3Op()
        op.kind, op.dtype, op.flags = _hip.OP_CONV, _hip.Y3_BF16, _hip.F_LEAKY
        op.batch, op.in_h, op.in_w, op.in_c, op.in_ld = B, h, h, cin, cin
        op.out_h, op.out_w, op.out_c, op.out_ld = ho, ho, cout, cout
        op.ksize, op.stride, op.pad, op.k_ld, op.cout_pad = k, stride, pad, kk, cp
        op.d_in, op.d_out = x.data_ptr(), out.data_ptr()
        op.d_weight, op.d_scale, op.d_bias = wt.data_ptr(), sc.data_ptr(), bi.data_ptr()
        opts = _hip.options(auto_mask=mask)
        handle = ctypes.c_void_p()
        _hip.check(lib.y3_plan_create_ex((_hip.Y3Op * 1)(op), 1, zero.data_ptr(), ctypes.byref(opts), ctypes.byref(handle)))
        try:
            names.append(lib.y3_plan_op_kernel(handle, 0).decode())
            _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            lib.y3_plan_destroy(handle)
        outs.append(out)
    if want == "conv_igemm":                               # (under the default mask a strip kernel or an implicit GEMM: not conv_dw48)
        assert not names[0].startswith("conv_dw48_"), names
    else:
        assert names[0].startswith(want), names
    assert names[1].startswith("conv_igemm") and torch.isfinite(outs[1].float()).all()
    assert torch.equal(outs[0], outs[1]), (names, float((outs[0].float() - outs[1].float()).abs().max()))


@pytest.mark.parametrize("h,cin,cout", [(38, 256, 512), (19, 512, 1024), (62, 128, 256), (76, 128, 256), (94, 256, 256)])
def test_direct_weights_kernel_beside_a_copy_kernel(h, cin, cout):
    """Regression (round 5): the direct-weights kernel loads its weights with inline-asm global loads, one K-step ahead.  The
    loads of the step AFTER the last one are still in flight at the end of the K loop and nobody reads their data, so the
    compiler took their destination registers for the epilogue's pointer arithmetic; alone the loads always landed first, beside
    the upload's copy kernel (memory contention) some landed late, overwrote an address, and the process ended with
    HSA_STATUS_ERROR_MEMORY_APERTURE_VIOLATION (first seen on the six-pass instantiation: 76^2 maps).  The final wait now keeps
    those registers allocated.  Every instantiation at its widest map, back to back beside that copy kernel: same bits as alone."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    B = 16
    g = torch.Generator().manual_seed(h)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    x = (torch.rand((B, h, h, cin), generator=g) - 0.5).to(torch.bfloat16).to(dev)
    k_ld = 9 * cin
    w = ((torch.rand((cout, k_ld), generator=g) - 0.5) * 0.05).to(torch.bfloat16).to(dev)
    sc, bi = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    out = torch.zeros((B, h, h, cout), dtype=torch.bfloat16, device=dev)
    op = _hip.Y3Op()
    op.kind, op.dtype, op.flags = _hip.OP_CONV, _hip.Y3_BF16, _hip.F_LEAKY
    op.batch, op.in_h, op.in_w, op.in_c, op.in_ld = B, h, h, cin, cin
    op.out_h, op.out_w, op.out_c, op.out_ld, op.res_ld = h, h, cout, cout, cout
    op.ksize, op.stride, op.pad, op.k_ld, op.cout_pad = 3, 1, 1, k_ld, cout
    op.d_in, op.d_out = x.data_ptr(), out.data_ptr()
    op.d_weight, op.d_scale, op.d_bias = w.data_ptr(), sc.data_ptr(), bi.data_ptr()
    opts = _hip.options()
    opts.auto_mask = _hip.AM_HALO_ALL | _hip.AM_HALO_DW_ALWAYS | _hip.AM_NO_SMALL_GRID
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex((_hip.Y3Op * 1)(op), 1, zero.data_ptr(), ctypes.byref(opts), ctypes.byref(handle)))
    try:
        assert lib.y3_plan_op_kernel(handle, 0).decode().startswith("conv_halo_dw_")
        _hip.check(lib.y3_plan_run(handle, None, None))
        torch.cuda.synchronize()
        alone = out.clone()
        host = torch.zeros(16 * 608 * 608 * 3, dtype=torch.uint8).pin_memory()
        dst = torch.zeros(16 * 608 * 608 * 3, dtype=torch.uint8, device=dev)
        cs, st = torch.cuda.Stream(), torch.cuda.Stream()
        for i in range(20):
            _hip.check(lib.y3_copy_bytes(host.data_ptr(), dst.data_ptr(), host.numel(), 8, _hip.stream_ptr(cs)))
            for j in range(6):
                _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr(st)))
            if i % 5 == 4:
                torch.cuda.synchronize()
                assert torch.equal(out, alone), i
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)


@pytest.mark.parametrize("dtype", ["float32"])
def test_96x64_tiles_are_chosen_for_yolov3_tiny_batch8_and_change_no_bit(dtype):
    """BASELINE configs[1] (yolov3-tiny 416 batch 8): the two big layers (13^2 512 -> 1024, 26^2 384 -> 256) are 352 / 344 tiles of
    128 x 32 on 256 CUs; the launcher picks 96 x 64 tiles (240 / 228, one round) for them -- and forbidding that choice
    (igemm_bm = 128) gives the same bits."""
    frames = synth_frames(41, 8, 416, 416)
    a = _net("yolov3-tiny", dtype=dtype)
    oa = {k: v.clone() for k, v in a.forward_frames(frames).items()}
    names = [r["kernel"] for r in a.plan_report()]
    assert sum("96x64" in n for n in names) >= 2, names
    b = _net("yolov3-tiny", dtype=dtype, options={"igemm_bm": 128})
    ob = b.forward_frames(frames)
    assert not any("96x64" in r["kernel"] for r in b.plan_report())
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(oa[k], ob[k]), k


@pytest.mark.parametrize("dim,dtype", [(672, "float32"), (672, "bf16"), (1024, "bf16")])
def test_patch_kernel_edge_tiles_match_implicit_gemm(dim, dtype):
    """2-D patch kernel (8 x 32 output tiles) on maps that are not a multiple of the tile (672 -> 168 = 5.25 x 32 wide,
    21 x 8 high) and on a 256-wide map against the run with those layers on the implicit GEMM: bit-identical in bf16
    and in float32 (all MFMA conv kernels run chunk-major)."""
    from yolov3 import _hip
    lib = _hip.lib()
    frames = synth_frames(dim, 1, dim, dim)
    try:
        outs = []
        for mask in (_hip.AM_HALO_ALL | _hip.AM_PATCH_WIDE, _hip.AM_HALO_ALL):
            _hip.check(lib.y3_set_tuning(b"auto_mask", mask))
            net = _net("yolov3", dtype=dtype)
            outs.append({k: v.clone() for k, v in net.forward_frames(frames).items()})
            assert any("conv_patch" in r["kernel"] for r in net.plan_report()) == bool(mask & _hip.AM_PATCH_WIDE)
        for k in ("bbox_xywh", "class_prob", "class_idx"):
            assert torch.equal(outs[0][k], outs[1][k]), k
    finally:
        lib.y3_set_tuning(b"auto_mask", DEFAULT_KNOBS["auto_mask"])


def test_wave_specialised_igemm_is_bit_identical():
    """igemm v3 (loader / consumer waves) runs the same MFMA sequence per accumulator as v2: whole-network
    outputs must be bit-identical, fp32 against the goldens too, for 2 and 3 LDS stages."""
    from yolov3 import _hip
    lib = _hip.lib()
    g = np.load(os.path.join(GOLDEN, "forward_yolov3.npz"))
    frames = np.stack([resize_bilinear_u8(load_jpeg_bgr("000000035279.jpg"), 608, 608), synth_frames(5, 1, 608, 608)[0]])
    x = torch.from_numpy(orc.frames_to_input(list(frames)))
    _hip.check(lib.y3_set_tuning(b"auto_mask", 0))      # every MFMA conv through the implicit GEMM
    try:
        ref32 = _net("yolov3").forward(x)
        ref16 = _net("yolov3", dtype="bf16").forward_frames(frames)
        ref16 = {k: v.clone() for k, v in ref16.items()}
        for ns in (2, 3, 4):
            _hip.check(lib.y3_set_tuning(b"igemm_version", 3))
            _hip.check(lib.y3_set_tuning(b"igemm_ns", ns))
            out = _net("yolov3").forward(x)
            np.testing.assert_allclose(out["bbox_xywh"].cpu().numpy(), g["bbox_xywh"], rtol=1e-4, atol=BOX_ATOL)
            for k in ("bbox_xywh", "class_prob", "class_idx"):
                assert torch.equal(out[k], ref32[k]), (ns, k)
            out16 = _net("yolov3", dtype="bf16").forward_frames(frames)
            for k in ("bbox_xywh", "class_prob", "class_idx"):
                assert torch.equal(out16[k], ref16[k]), (ns, k, "bf16")
    finally:
        lib.y3_set_tuning(b"igemm_version", 2)
        lib.y3_set_tuning(b"igemm_ns", 2)
        lib.y3_set_tuning(b"auto_mask", DEFAULT_KNOBS["auto_mask"])


def _pair_dtypes():
    from yolov3 import _hip
    return {"bf16": (_hip.Y3_BF16, torch.bfloat16), "fp16": (_hip.Y3_F16, torch.float16)}


_PAIR_DTYPES = _pair_dtypes()      # storage type of the hand-built two-op plans below: (y3_op.dtype, torch dtype)


def _resblock_plan(net, x, fuse, dev, dtype="bf16"):
    """1x1 (64 -> 32) + 3x3 (32 -> 64) + shortcut of yolov3's first residual block as a hand-built two-op plan
    (``dtype``: "bf16" / "fp16", the storage type of x, the weights and the output)."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    b, h, w, _ = x.shape
    c_dtype, t_dtype = _PAIR_DTYPES[dtype]
    w2 = net._device_weights(2, _hip.PATH_IGEMM, dtype, dev)
    w3 = net._device_weights(3, _hip.PATH_IGEMM, dtype, dev)
    mid = torch.zeros((b, h, w, 32), dtype=t_dtype, device=dev)
    out = torch.zeros((b, h, w, 64), dtype=t_dtype, device=dev)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    ops = (_hip.Y3Op * 2)()
    for op, (wt, cin, cout, k) in zip(ops, ((w2, 64, 32, 1), (w3, 32, 64, 3))):
        op.kind, op.dtype, op.batch = _hip.OP_CONV, c_dtype, b
        op.ksize, op.stride, op.pad = k, 1, (k - 1) // 2
        op.in_c, op.out_c, op.in_ld, op.out_ld = cin, cout, cin, cout
        op.in_h = op.out_h = h
        op.in_w = op.out_w = w
        op.cout_pad, op.k_ld = wt["cout_pad"], wt["k_ld"]
        op.d_weight, op.d_scale, op.d_bias = wt["weight"].data_ptr(), wt["scale"].data_ptr(), wt["bias"].data_ptr()
        op.flags = _hip.F_LEAKY
    ops[0].d_in, ops[0].d_out = x.data_ptr(), mid.data_ptr()
    ops[0].flags |= _hip.F_FUSE_NEXT if fuse else 0
    ops[1].d_in, ops[1].d_out, ops[1].d_res, ops[1].res_ld = mid.data_ptr(), out.data_ptr(), x.data_ptr(), 64
    ops[1].flags |= _hip.F_RESIDUAL
    ops[1].block_idx = 1
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create(ops, 2, zero.data_ptr(), ctypes.byref(handle)))
    _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
    torch.cuda.synchronize()
    name0 = lib.y3_plan_op_kernel(handle, 0).decode()
    lib.y3_plan_destroy(handle)
    return out, name0


@pytest.mark.parametrize("dim,batch", [(304, 1), (48, 2), (40, 3)])
def test_fused_residual_block_is_bit_identical(dim, batch):
    """One kernel for 1x1 + 3x3 + shortcut (64 -> 32 -> 64): same operands, MFMA order and epilogue arithmetic as the
    two implicit-GEMM launches, so the block's output must match bit for bit (40 = 2.5 tiles per side)."""
    net = _net("yolov3", dtype="bf16")
    dev = net._torch_device()
    g = torch.Generator().manual_seed(dim)
    x = (torch.randn((batch, dim, dim, 64), generator=g) * 0.7).to(torch.bfloat16).to(dev)
    fused, n_f = _resblock_plan(net, x, True, dev)
    plain, n_p = _resblock_plan(net, x, False, dev)
    assert n_f == "conv_resblock_fused_bf16_64_32_64" and n_p.startswith("conv_igemm2")
    assert torch.equal(fused, plain), float((fused.float() - plain.float()).abs().max())


def _first_two_convs_plan(net, frames, fuse, dev, dtype="bf16"):
    """A two-op plan (stem conv + stride-2 conv of yolov3) built by hand so the second conv's output can be read
    (``dtype``: "bf16" / "fp16", the storage type of the weights, the intermediate and the output)."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    b, h, w, _ = frames.shape
    c_dtype, t_dtype = _PAIR_DTYPES[dtype]
    w0 = net._device_weights(0, _hip.PATH_STEM_MFMA, dtype, dev)
    w1 = net._device_weights(1, _hip.PATH_IGEMM, dtype, dev)
    mid = torch.zeros((b, h, w, 32), dtype=t_dtype, device=dev)
    out = torch.zeros((b, h // 2, w // 2, 64), dtype=t_dtype, device=dev)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    ops = (_hip.Y3Op * 2)()
    for op, (wt, cin, cout, k, st) in zip(ops, ((w0, 3, 32, 3, 1), (w1, 32, 64, 3, 2))):
        op.kind, op.dtype, op.batch = _hip.OP_CONV, c_dtype, b
        op.ksize, op.stride, op.pad = k, st, 1
        op.in_c, op.out_c = cin, cout
        op.cout_pad, op.k_ld = wt["cout_pad"], wt["k_ld"]
        op.d_weight, op.d_scale, op.d_bias = wt["weight"].data_ptr(), wt["scale"].data_ptr(), wt["bias"].data_ptr()
        op.flags = _hip.F_LEAKY
    ops[0].in_h, ops[0].in_w, ops[0].in_ld = h, w, 3
    ops[0].out_h, ops[0].out_w, ops[0].out_ld = h, w, 32
    ops[0].flags |= _hip.F_PLAN_INPUT | _hip.F_IN_NHWC_U8BGR | (_hip.F_FUSE_NEXT if fuse else 0)
    ops[0].d_out = mid.data_ptr()
    ops[1].in_h, ops[1].in_w, ops[1].in_ld = h, w, 32
    ops[1].out_h, ops[1].out_w, ops[1].out_ld = h // 2, w // 2, 64
    ops[1].d_in, ops[1].d_out = mid.data_ptr(), out.data_ptr()
    ops[1].block_idx = 1
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create(ops, 2, zero.data_ptr(), ctypes.byref(handle)))
    dfr = torch.from_numpy(frames).to(dev)
    _hip.check(lib.y3_plan_run(handle, dfr.data_ptr(), _hip.stream_ptr()))
    torch.cuda.synchronize()
    name0 = lib.y3_plan_op_kernel(handle, 0).decode()
    lib.y3_plan_destroy(handle)
    return out.float().cpu().numpy(), name0


@pytest.mark.parametrize("dim,batch", [(608, 1), (96, 2), (80, 1)])
def test_fused_first_two_convs_output(dim, batch):
    """Output of the second conv, fused kernel against the two separate kernels, on frames whose borders and tile
    edges matter (96 = 3 tiles per side at the second conv, 80 = 2.5).  A geometry error would show as O(1)
    differences; what remains is bf16 rounding of a few stem values."""
    net = _net("yolov3", dtype="bf16")
    dev = net._torch_device()
    frames = synth_frames(77 + dim, batch, dim, dim)
    fused, n_f = _first_two_convs_plan(net, frames, True, dev)
    plain, n_p = _first_two_convs_plan(net, frames, False, dev)
    assert n_f == "conv_stem_s2_fused_u8_bf16" and n_p == "conv_stem_mfma_u8_bf16"
    scale = np.abs(plain).mean()
    d = np.abs(fused - plain)
    assert d.max() <= 0.1 * max(1.0, np.abs(plain).max()) and d.mean() <= 2e-3 * scale, (d.max(), d.mean(), scale)
    assert (d > 0).mean() < 0.2      # most values identical


@pytest.mark.parametrize("dim,batch", [(608, 1), (96, 2), (80, 1), (48, 5), (16, 3)])
def test_wave_specialised_stem_kernel_is_bit_identical_to_phase_kernel(dim, batch):
    """The default fused stem kernel (conv waves + stem waves, two stem images in LDS, patches fetched four steps ahead)
    does the arithmetic of the phase-by-phase kernel (`fuse_stem` = 2) in the same order: same bits, for full tiles,
    partial tiles (80 -> 40 outputs = 2.5 tiles wide), frame borders, and fewer tiles than the prefetch distance."""
    from yolov3 import _hip
    lib = _hip.lib()
    net = _net("yolov3", dtype="bf16")
    dev = net._torch_device()
    frames = synth_frames(5 + dim, batch, dim, dim)
    try:
        _hip.check(lib.y3_set_tuning(b"fuse_stem", 2))
        phase, n0 = _first_two_convs_plan(net, frames, True, dev)
        _hip.check(lib.y3_set_tuning(b"fuse_stem", 1))
        ws, n1 = _first_two_convs_plan(net, frames, True, dev)
    finally:
        lib.y3_set_tuning(b"fuse_stem", 1)
    assert n0 == n1 == "conv_stem_s2_fused_u8_bf16"
    assert np.abs(phase).max() > 0
    assert np.array_equal(phase, ws)


@pytest.mark.parametrize("dim,batch", [(608, 2), (416, 1), (320, 3)])
def test_fused_stem_and_stride2_conv_matches_unfused(dim, batch):
    """The first two convs of yolov3 / yolov3-spp run as one kernel (uint8 frames -> 32-channel stem kept in LDS ->
    stride-2 conv).  Same bf16 operands and fp32 accumulation as the two separate kernels; only the position of the
    27 stem products inside the MFMA K dimension differs, so outputs agree to bf16 rounding noise."""
    from yolov3 import _hip
    lib = _hip.lib()
    frames = synth_frames(31 + dim, batch, dim, dim)
    try:
        _hip.check(lib.y3_set_tuning(b"fuse_stem", 1))
        net = _net("yolov3", dtype="bf16")
        fused = {k: v.clone() for k, v in net.forward_frames(frames).items()}
        names = [r["kernel"] for r in net.plan_report()]
        assert names[0] == "conv_stem_s2_fused_u8_bf16" and names[1].startswith("(fused")
        _hip.check(lib.y3_set_tuning(b"fuse_stem", 0))
        net2 = _net("yolov3", dtype="bf16")
        plain = net2.forward_frames(frames)
        assert net2.plan_report()[0]["kernel"] == "conv_stem_mfma_u8_bf16"
        d = (fused["class_prob"] - plain["class_prob"]).abs()
        assert float(d.max()) < 0.1 and float(d.median()) < 2e-3, (float(d.max()), float(d.median()))
        assert float((fused["class_idx"] == plain["class_idx"]).float().mean()) > 0.98
        torch.testing.assert_close(fused["bbox_xywh"], plain["bbox_xywh"], rtol=5e-2, atol=5e-3)
    finally:
        lib.y3_set_tuning(b"fuse_stem", 1)


@pytest.mark.parametrize("model,dim,batch", [("yolov3", 608, 2), ("yolov3", 320, 3), ("yolov3-tiny", 416, 2), ("yolov3-spp", 416, 1)])
def test_fused_head_conv_and_decode_matches_separate_kernels(model, dim, batch):
    """Detection heads in bf16 networks: 1x1 conv + YOLO decode in one launch (float32 logits stay in LDS) against the
    head conv kernel followed by the decode kernel."""
    from yolov3 import _hip
    lib = _hip.lib()
    frames = synth_frames(17 + dim, batch, dim, dim)
    try:
        _hip.check(lib.y3_set_tuning(b"fuse_head", 1))
        net = _net(model, dtype="bf16")
        fused = {k: v.clone() for k, v in net.forward_frames(frames).items()}
        names = [r["kernel"] for r in net.plan_report()]
        assert sum(k.startswith("conv_head_decode_") for k in names) == (2 if model == "yolov3-tiny" else 3)
        _hip.check(lib.y3_set_tuning(b"fuse_head", 0))
        net2 = _net(model, dtype="bf16")
        plain = net2.forward_frames(frames)
        assert not any("head_decode" in r["kernel"] for r in net2.plan_report())
        assert torch.equal(fused["class_idx"], plain["class_idx"])
        torch.testing.assert_close(fused["class_prob"], plain["class_prob"], rtol=2e-6, atol=1e-9)
        torch.testing.assert_close(fused["bbox_xywh"], plain["bbox_xywh"], rtol=2e-6, atol=1e-9)
    finally:
        lib.y3_set_tuning(b"fuse_head", 1)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("model,dim,batch", [("yolov3", 608, 1), ("yolov3", 608, 16), ("yolov3", 352, 3), ("yolov3-tiny", 416, 5),
                                             ("yolov3-spp", 416, 2)])
def test_direct_weights_head_kernel_equals_tiled_head_kernel(model, dim, batch, dtype):
    """Round 6: the detection heads on the direct-weights 1x1 kernel (conv_head_decode_dw: whole activation tile in LDS, weight
    fragments from the fragment-order copy, logits parked in the same LDS, the shared four-lane decode) against the tiled head kernel
    (y3_options.fuse_head = 2): the same K order and the same epilogue arithmetic -- every output bit-equal; 48- and 96-pixel tiles
    forced (fuse_head = 3 / 4) as well.  Replaces /root/reference/yolov3/darknet.py:244-257 (head conv) + :86-116 (YOLOLayer)."""
    frames = synth_frames(23 + dim + batch, batch, dim, dim)
    outs = {}
    for mode in (1, 2, 3, 4):
        net = _net(model, dtype=dtype, options={"fuse_head": mode})
        outs[mode] = {k: v.clone() for k, v in net.forward_frames(frames).items()}
        names = [r["kernel"] for r in net.plan_report() if r["kernel"].startswith("conv_head_decode_")]
        assert len(names) == (2 if model == "yolov3-tiny" else 3), names
        if mode == 2:
            assert all("_dw_" not in k for k in names), names
        else:
            assert all(k.startswith("conv_head_decode_dw_") for k in names), names
        if mode == 3:
            assert all(k.endswith("_48x256") for k in names), names
        if mode == 4:
            assert any(k.endswith("_96x256") for k in names), names
    assert float(outs[2]["class_prob"].max()) > 0
    for mode in (1, 3, 4):
        for k in ("bbox_xywh", "class_prob", "class_idx"):
            assert torch.equal(outs[mode][k], outs[2][k]), (mode, k)


def test_split_class_decode_matches_sequential_decode():
    """bf16 networks decode every box with four lanes (class range split, shuffle-combined); against the sequential
    class loop of the float32 path on the same head tensors: identical arg-max, scores equal to float32 rounding of
    the exp-sum, boxes identical.  (Plan options are fixed per plan: two networks.)"""
    frames = synth_frames(91, 2, 416, 416)
    fast = _net("yolov3", dtype="bf16", options={"decode_lanes": 4, "fuse_head": 0}).forward_frames(frames)
    seq = _net("yolov3", dtype="bf16", options={"decode_lanes": 1, "fuse_head": 0}).forward_frames(frames)
    assert torch.equal(fast["class_idx"], seq["class_idx"])
    assert torch.equal(fast["bbox_xywh"], seq["bbox_xywh"])
    torch.testing.assert_close(fast["class_prob"], seq["class_prob"], rtol=2e-6, atol=1e-9)


_HEAD_CFG = """[net]
batch=1
height=%(dim)d
width=%(dim)d
channels=3

[convolutional]
batch_normalize=1
filters=64
size=3
stride=2
pad=1
activation=leaky

[convolutional]
batch_normalize=1
filters=%(mid)d
size=3
stride=1
pad=1
activation=leaky

[convolutional]
size=1
stride=1
pad=1
filters=%(filters)d
activation=linear

[yolo]
mask = %(mask)s
anchors = 10,13, 16,30, 33,23, 30,61
classes=%(ncls)d
num=4
"""


@pytest.mark.parametrize("ncls,mask,mid", [(60, "0,1,2", 128), (23, "1,2,3,0", 128), (80, "0,1,2", 128), (122, "0,1", 128),
                                           (60, "0,1,2", 256), (23, "1,2,3,0", 512), (122, "0,1", 256)])
def test_fused_head_other_class_counts(tmp_path, ncls, mask, mid):
    """Fused head conv + decode for heads that are not COCO's 3 x 85: generic class loop of the four-lane decode, 2-4
    anchors per head, against the two-kernel path and against the bf16-emulating oracle.  128 channels in front of the head: the
    tiled head kernel; 256 / 512: the direct-weights head kernel (round 6)."""
    n_anchor = len(mask.split(","))
    cfg = tmp_path / "head.cfg"
    cfg.write_text(_HEAD_CFG % dict(dim=96, filters=n_anchor * (5 + ncls), mask=mask, ncls=ncls, mid=mid))
    from yolov3.cfgparse import parse_config
    blocks, net_info = parse_config(str(cfg))
    params = W.synth_params(blocks, net_info, seed=3, obj_bias=-2.0, calib=None)
    frames = synth_frames(900 + ncls, 3, 96, 96)
    outs = {}
    for fuse in (1, 0):
        net = yolov3.Darknet(str(cfg), device="cuda", dtype="bf16", options={"fuse_head": fuse}).eval()
        net.set_params(params)
        outs[fuse] = {k: v.clone() for k, v in net.forward_frames(frames).items()}
        names = [r["kernel"] for r in net.plan_report()]
        # (heads of at most 128 channels keep the two kernels: the fused tile is 256 channels wide)
        assert any("head_decode" in k for k in names) == (bool(fuse) and n_anchor * (5 + ncls) > 128), names
        if fuse and n_anchor * (5 + ncls) > 128:
            assert any("head_decode_dw_" in k for k in names) == (mid >= 256), names
    fused, plain = outs[1], outs[0]
    assert torch.equal(fused["class_idx"], plain["class_idx"])
    torch.testing.assert_close(fused["class_prob"], plain["class_prob"], rtol=2e-6, atol=1e-9)
    torch.testing.assert_close(fused["bbox_xywh"], plain["bbox_xywh"], rtol=2e-6, atol=1e-9)
    onet = orc.OracleDarknet(str(cfg)).set_params(params)
    want = onet.forward(torch.from_numpy(orc.frames_to_input(list(frames))), emulate_bf16=True)
    np.testing.assert_allclose(fused["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=5e-2, atol=5e-3)
    d = np.abs(fused["class_prob"].cpu().numpy() - want["class_prob"].numpy())
    assert d.max() < 3e-2 and np.median(d) < 2e-3, (d.max(), np.median(d))


@pytest.mark.parametrize("ncls,n_anchor,h,w", [(1, 3, 5, 7), (3, 1, 4, 4), (7, 2, 6, 5), (20, 3, 5, 5), (80, 3, 7, 6),
                                               (81, 2, 3, 9), (6, 8, 2, 3)])
@pytest.mark.parametrize("dtype", ["bf16", "float32"])
def test_yolo_decode_op_any_class_count(dtype, ncls, n_anchor, h, w):
    """The decode op alone (y3_op_run) against the oracle's YOLOLayer restatement for class counts other than COCO's 80:
    the four-lanes-per-box form (bf16 networks: decode_core.h) keeps its 80-class lanes in registers and has a generic
    loop with a ragged last lane for everything else; the float32 form is the sequential loop."""
    import ctypes
    from yolov3 import _hip
    lib = _hip.lib()
    _hip.require_gpu()
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(ncls * 131 + n_anchor)
    batch, n_attr = 2, 5 + ncls
    ld = (n_anchor * n_attr + 3) // 4 * 4
    x = (rng.randn(batch, n_anchor * n_attr, h, w) * 2.0).astype(np.float32)
    anchors = [(float(rng.randint(8, 200)), float(rng.randint(8, 200))) for _ in range(n_anchor)]
    net_w, net_h = 32.0 * w, 32.0 * h
    nhwc = np.zeros((batch, h, w, ld), dtype=np.float32)
    nhwc[..., :n_anchor * n_attr] = x.transpose(0, 2, 3, 1)
    d_in = torch.from_numpy(nhwc).to(dev)
    rows = n_anchor * h * w
    bbox = torch.zeros((batch, rows, 4), dtype=torch.float32, device=dev)
    prob = torch.zeros((batch, rows), dtype=torch.float32, device=dev)
    cls = torch.full((batch, rows), -1, dtype=torch.int64, device=dev)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    op = _hip.Y3Op()
    op.kind, op.dtype, op.batch = _hip.OP_YOLO, (_hip.Y3_BF16 if dtype == "bf16" else _hip.Y3_F32), batch
    op.in_h, op.in_w, op.in_c, op.in_ld = h, w, n_anchor * n_attr, ld
    op.n_anchor, op.n_attr = n_anchor, n_attr
    for i, (aw, ah) in enumerate(anchors):
        op.anchor_w[i], op.anchor_h[i] = aw, ah
    op.row_offset, op.rows_total = 0, rows
    op.net_w, op.net_h = net_w, net_h
    op.d_in, op.d_bbox, op.d_prob, op.d_cls = d_in.data_ptr(), bbox.data_ptr(), prob.data_ptr(), cls.data_ptr()
    _hip.check(lib.y3_op_run(ctypes.byref(op), None, zero.data_ptr(), _hip.stream_ptr()))
    torch.cuda.synchronize()
    bb, pr, ci = orc.yolo_decode(torch.from_numpy(x), anchors)
    bb = bb.clone()
    bb[..., 2] /= net_w                                   # Darknet.forward divides w, h by the network size
    bb[..., 3] /= net_h
    np.testing.assert_allclose(bbox.cpu().numpy(), bb.numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(prob.cpu().numpy(), pr.numpy(), rtol=1e-5, atol=1e-8)
    got, want = cls.cpu().numpy(), ci.numpy()
    differ = got != want
    if differ.any():                                      # only where the top two class logits are within float rounding
        t = x.reshape(batch, n_anchor, n_attr, h, w)[:, :, 5:].transpose(0, 1, 3, 4, 2).reshape(batch, rows, ncls)
        top2 = np.sort(t[differ], axis=-1)[:, -2:]
        assert np.all(top2[:, 1] - top2[:, 0] < 1e-5), "arg-max differs beyond a rounding tie"


def test_graph_replay_equals_eager_launches():
    """With the plan option use_graph, y3_plan_run replays a captured hipGraph on non-default streams (one launch per
    forward instead of ~80); same bits as launching every kernel, for repeated calls and alternating inputs."""
    eager = _net("yolov3", dtype="bf16", options={"use_graph": 0})
    graph = _net("yolov3", dtype="bf16", options={"use_graph": 1})
    dev = eager._torch_device()
    a = torch.from_numpy(synth_frames(1, 2, 416, 416)).to(dev)
    b = torch.from_numpy(synth_frames(2, 2, 416, 416)).to(dev)
    ref = [{k: v.clone() for k, v in eager.forward_frames(x).items()} for x in (a, b)]
    torch.cuda.synchronize()                       # the side stream below does not wait for the default stream
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        for rep in range(3):                       # eager warm-up, capture, replay -- for both inputs
            for x, want in ((a, ref[0]), (b, ref[1])):
                got = graph.forward_frames(x)
                stream.synchronize()
                for k in want:
                    assert torch.equal(got[k], want[k]), (rep, k)


def test_plan_options_are_per_plan():
    """Two networks with different kernel-selection options live side by side; y3_set_tuning (the A/B tool) only changes
    the defaults of plans created later."""
    from yolov3 import _hip
    lib = _hip.lib()
    frames = synth_frames(3, 1, 416, 416)
    plain = _net("yolov3", dtype="bf16", options={"auto_mask": 0, "fuse_stem": 0, "fuse_head": 0})
    fast = _net("yolov3", dtype="bf16", options={"auto_mask": _hip.AM_DEFAULT | _hip.AM_NO_SMALL_GRID})
    dflt = _net("yolov3", dtype="bf16")
    o_plain = {k: v.clone() for k, v in plain.forward_frames(frames).items()}
    o_fast = {k: v.clone() for k, v in fast.forward_frames(frames).items()}
    o_dflt = {k: v.clone() for k, v in dflt.forward_frames(frames).items()}
    assert not any("halo" in r["kernel"] or "fused" in r["kernel"] or "igemm3" in r["kernel"] for r in plain.plan_report())
    assert any("halo" in r["kernel"] for r in fast.plan_report())
    names_dflt = [r["kernel"] for r in dflt.plan_report()]
    # (one frame: the small-grid kernel of round 6 takes what the wave-specialised implicit GEMM took until then)
    assert any("igemm3" in k or "conv_dw48" in k for k in names_dflt) and any("fused" in k for k in names_dflt)
    try:
        _hip.check(lib.y3_set_tuning(b"auto_mask", 0))       # must not reach into the existing plans
        again = dflt.forward_frames(frames)
        assert [r["kernel"] for r in dflt.plan_report()] == names_dflt
        for k in o_dflt:
            assert torch.equal(again[k], o_dflt[k])
        late = _net("yolov3", dtype="bf16")                 # created under the changed defaults
        late.forward_frames(frames)
        assert not any("halo" in r["kernel"] or "igemm3" in r["kernel"] or "conv_dw48" in r["kernel"] for r in late.plan_report())
    finally:
        lib.y3_set_tuning(b"auto_mask", DEFAULT_KNOBS["auto_mask"])
    assert float((o_plain["class_prob"] - o_fast["class_prob"]).abs().median()) < 2e-3
    assert float((o_plain["class_prob"] - o_dflt["class_prob"]).abs().median()) < 2e-3


def test_plan_options_choose_fragment_weight_kernels():
    """A plan's own options decide which convs read fragment-order weights, also where the process defaults would not pick
    those kernels: a small-grid direct-weights kernel wherever it fits (Y3_AM_SMALL_DW_ALWAYS) at batch 16, and 96-pixel head
    tiles (fuse_head 4) while y3_set_tuning has fuse_head 0.  Both compile, run other kernels than the defaults, and give the
    same bits (every MFMA conv kernel sums in the same K order)."""
    from yolov3 import _hip
    lib = _hip.lib()
    frames = synth_frames(5, 16, 608, 608)
    dflt = _net("yolov3", dtype="bf16")
    o_dflt = {k: v.clone() for k, v in dflt.forward_frames(frames).items()}
    names_dflt = [r["kernel"] for r in dflt.plan_report()]
    small = _net("yolov3", dtype="bf16", options={"auto_mask": _hip.AM_DEFAULT | _hip.AM_SMALL_DW_ALWAYS})
    o_small = {k: v.clone() for k, v in small.forward_frames(frames).items()}
    assert [r["kernel"] for r in small.plan_report()] != names_dflt
    try:
        _hip.check(lib.y3_set_tuning(b"fuse_head", 0))
        head = _net("yolov3", dtype="bf16", options={"fuse_head": 4})
        o_head = {k: v.clone() for k, v in head.forward_frames(frames).items()}
    finally:
        lib.y3_set_tuning(b"fuse_head", DEFAULT_KNOBS["fuse_head"])
    names_head = [r["kernel"] for r in head.plan_report()]
    assert names_head != names_dflt and any(k.startswith("conv_head_decode_dw_") and k.endswith("_96x256") for k in names_head)
    for k in o_dflt:
        assert torch.equal(o_small[k], o_dflt[k]), k
        assert torch.equal(o_head[k], o_dflt[k]), k


@pytest.mark.parametrize("dtype,dim,batch", [("bf16", 608, 2), ("float32", 416, 1), ("bf16", 320, 3), ("fp16", 416, 2)])
def test_spp_pyramid_kernel_is_bit_identical_to_three_pools(dtype, dim, batch):
    """yolov3-spp's three stride-1 max-pools (5 / 9 / 13, zero pad right / bottom) as ONE LDS-staged cascade launch
    against the three separate gather kernels: max is exact, so every output bit must agree."""
    frames = synth_frames(dim + batch, batch, dim, dim)
    one = _net("yolov3-spp", dtype=dtype, options={"fuse_spp": 1})
    three = _net("yolov3-spp", dtype=dtype, options={"fuse_spp": 0})
    a = {k: v.clone() for k, v in one.forward_frames(frames).items()}
    b = three.forward_frames(frames)
    names = [r["kernel"] for r in one.plan_report()]
    assert sum(k.startswith("maxpool_spp_pyramid") for k in names) == 1 and not any(k.startswith("maxpool_") and "spp" not in k for k in names)
    assert sum(r["kernel"].startswith("maxpool_") for r in three.plan_report()) == 3
    for k in a:
        assert torch.equal(a[k], b[k]), k
        if a[k].dtype == torch.float32:               # bits, not values: -0.0 == +0.0 as floats
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k


def test_bf16_agreement_report_yolov3():
    """bf16 is the throughput path, not a parity path: report (and loosely bound) its agreement
    with the fp32 HIP path on the golden frames."""
    g = np.load(os.path.join(GOLDEN, "forward_yolov3.npz"))
    dim = 608
    frames = np.stack([resize_bilinear_u8(load_jpeg_bgr("000000035279.jpg"), dim, dim), synth_frames(5, 1, dim, dim)[0]])
    out = _net("yolov3", dtype="bf16").forward_frames(frames)
    pr = out["class_prob"].cpu().numpy()
    ci = out["class_idx"].cpu().numpy()
    d = np.abs(pr - g["class_prob"])
    agree = (ci == g["class_idx"]).mean()
    print("bf16 vs reference fp32: score |d| median %.2e p99 %.2e max %.2e; arg-max agreement %.4f" % (
        np.median(d), np.percentile(d, 99), d.max(), agree))
    assert np.isfinite(pr).all() and np.median(d) < 2e-2 and agree > 0.5
