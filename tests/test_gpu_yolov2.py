"""YOLOv2 on the GPU (-m gpu), against the float32 restatement of tests/yolov2_restate.py.

* ``y3_reorg`` as one-op plans through the C ABI: both forms, three dtypes, strided input and output slices inside poisoned
  allocations; the slice is bit-exact and every byte around and between the slices keeps its poison.
* The region decode on a 64 x 64 mini network with five fractional anchors: every row against the restatement's decode of the
  product's own float32 logits (read back with ``keep_all``), under the tolerances of test_gpu_yolov4_families.py's decode
  gate, classes identical.  A fused head kernel never stores its logits: those runs are held to the restatement's decode of the
  restatement's logits from the product's head input, classes identical wherever the soft-max margin is clear (1e-3, the rule
  of test_gpu_yolov4.py).  135 / 225-channel heads are ones a fused head kernel takes with five anchors (``classes`` 22 / 40
  on top of the 1, 20, 80 of the shipped heads' range); the test prints which kernel ran.
* yolov2-tiny at 416 and yolov2 at 608 / 320 with calibrated procedural weights, batch 2: float32 under the bounds of
  ``test_csp_float32_matches_restatement``; bf16 / fp16 teacher-forced block by block at one storage ulp; the reorg block
  bit-exact in every mode.
* ``detect_in_frames`` and the command line on yolov2-tiny, letterbox on and off; ``multi_label=True`` is refused by name.
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

import yolov2_restate as R
from golden_util import GOLDEN, MODEL_DIR, ROOT, SAMPLE_IMAGES, load_jpeg_bgr
from test_gpu_bf16 import MODES, _close_bf16
from test_gpu_parity import BOX_ATOL, SCORE_ATOL
from test_yolov2_host import ANCHORS

pytestmark = pytest.mark.gpu

DTYPES = {"float32": (_hip.Y3_F32, torch.int32, "f32"), "bf16": (_hip.Y3_BF16, torch.int16, "bf16"),
          "fp16": (_hip.Y3_F16, torch.int16, "f16")}
GUARD = 4096          # elements of poison in front of and behind each allocation


# ------------------------------------------------------------------ reorg, one op at a time

# (C, H, W), s, input channel offset / pixel stride beyond the slice, output likewise
REORG_CASES = [((4, 2, 2), 2, (4, 12), (8, 8)),           # the smallest legal case
               ((8, 4, 6), 2, (0, 8), (16, 24)),          # non-square
               ((64, 26, 26), 2, (8, 16), (0, 1024)),     # the yolov2 layer at 416, written in front of the 1024-channel trunk
               ((12, 6, 4), 2, (3, 5), (5, 7)),           # C not a power of two, odd offsets and strides
               ((16, 8, 8), 4, (0, 3), (1, 2))]           # s = 4


def _poison(n, dtype, value):
    return torch.full((n,), value, dtype=dtype, device="cuda")


@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
@pytest.mark.parametrize("form3d", [False, True], ids=["flat", "3d"])
@pytest.mark.parametrize("case", REORG_CASES, ids=lambda c: "c%dx%dx%d_s%d" % (c[0] + (c[1],)))
def test_reorg_op_is_bit_exact_and_stays_in_its_slice(case, form3d, dtype):
    (c, h, w), s, (in_c0, in_more), (out_c0, out_more) = case
    batch = 2
    y3_dtype, idt, tag = DTYPES[dtype]
    es = 4 if dtype == "float32" else 2
    co, ho, wo = c * s * s, h // s, w // s
    in_ld, out_ld = in_c0 + c + in_more, out_c0 + co + out_more
    assert in_ld > c and out_ld > co
    gen = torch.Generator().manual_seed(c * 1000 + h * 10 + s + form3d)
    lo, hi = (-2 ** 31, 2 ** 31) if es == 4 else (-2 ** 15, 2 ** 15)
    n_in, n_out = batch * h * w * in_ld, batch * ho * wo * out_ld
    # random storage values everywhere in the input allocation (any bit pattern: the op moves storage elements)
    in_all = torch.randint(lo, hi, (GUARD + n_in + GUARD,), generator=gen, dtype=torch.int64).to(idt).cuda()
    in_before = in_all.clone()
    poison = 0x5A5A5A5A if es == 4 else 0x5A5A
    out_all = _poison(GUARD + n_out + GUARD, idt, poison)
    zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")

    op = _hip.Y3Op()
    op.kind, op.dtype, op.batch, op.block_idx = _hip.OP_REORG, y3_dtype, batch, 27
    op.flags = _hip.F_REORG_3D if form3d else 0
    op.in_c, op.in_h, op.in_w, op.in_ld = c, h, w, in_ld
    op.out_c, op.out_h, op.out_w, op.out_ld = co, ho, wo, out_ld
    op.ksize, op.stride = 1, s
    op.d_in = in_all.data_ptr() + (GUARD + in_c0) * es
    op.d_out = out_all.data_ptr() + (GUARD + out_c0) * es
    lib = _hip.lib()
    ops = (_hip.Y3Op * 1)(op)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, 1, zero.data_ptr(), None, ctypes.byref(handle)))
    try:
        assert lib.y3_plan_op_kernel(handle, 0).decode() == ("reorg3d_" if form3d else "reorg_") + tag
        _hip.check(lib.y3_plan_run(handle, in_all.data_ptr(), _hip.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)

    assert torch.equal(in_all, in_before), "the input allocation changed"
    x = in_all[GUARD:GUARD + n_in].view(batch, h, w, in_ld)[..., in_c0:in_c0 + c].permute(0, 3, 1, 2).cpu().numpy()
    want = torch.from_numpy(R.reorg(x, s, form3d)).permute(0, 2, 3, 1)            # NHWC
    out = out_all.cpu()
    body = out[GUARD:GUARD + n_out].view(batch, ho, wo, out_ld)
    assert torch.equal(body[..., out_c0:out_c0 + co], want), "slice differs from the restatement"
    # canaries: the guards in front and behind, and the channels of every pixel on either side of the slice
    assert bool((out[:GUARD] == poison).all()) and bool((out[GUARD + n_out:] == poison).all()), "guard overwritten"
    assert bool((body[..., :out_c0] == poison).all()) and bool((body[..., out_c0 + co:] == poison).all()), \
        "bytes between the slices overwritten"


# ------------------------------------------------------------------ region decode

def _conv(f, k, act="leaky", bn=True):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=%s\n\n" % (
        "batch_normalize=1\n" if bn else "", f, k, act)


def region_cfg(classes):
    """64 x 64 -> an 8 x 8 grid; the head conv reads 128 channels (what both fused head kernels need)."""
    anchors = ", ".join("%g, %g" % tuple(a) for a in ANCHORS)
    return ("[net]\nwidth=64\nheight=64\nchannels=3\n\n" +
            _conv(32, 3) + "[maxpool]\nsize=2\nstride=2\n\n" +
            _conv(64, 3) + "[maxpool]\nsize=2\nstride=2\n\n" +
            _conv(128, 3) + "[maxpool]\nsize=2\nstride=2\n\n" +
            _conv(128, 1) +                                          # 6
            _conv(5 * (5 + classes), 1, "linear", False) +           # 7: head
            "[region]\nanchors = %s\nclasses=%d\ncoords=4\nnum=5\nsoftmax=1\n" % (anchors, classes))


REGION_HEAD = 7


def _mini_params(cfg):
    blocks, net_info = parse_config(cfg)
    calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
    return W.synth_params(blocks, net_info, seed=7, obj_bias=-2.0, calib=calib)


REGION_RUNS = [("float32", {"fuse_head": 0}), ("float32", {}),
               ("bf16", {"fuse_head": 0}), ("bf16", {}), ("bf16", {"fuse_head": 2}), ("bf16", {"fuse_head": 3}),
               ("fp16", {"fuse_head": 0}), ("fp16", {"fuse_head": 2})]


def _margin(logits, na):
    """per row: soft-max probability of the best class minus that of the second (1 for a single class)"""
    b, ch, h, w = logits.shape
    p = torch.softmax(logits.reshape(b, na, ch // na, h, w)[:, :, 5:], dim=2)
    if p.shape[2] == 1:
        return torch.ones(b, na * h * w)
    top2 = torch.topk(p, 2, dim=2).values
    return (top2[:, :, 0] - top2[:, :, 1]).reshape(b, -1)


@pytest.mark.parametrize("dtype,options", REGION_RUNS, ids=lambda v: v if isinstance(v, str) else "fh%s" % v.get("fuse_head", "d"))
@pytest.mark.parametrize("classes", [1, 20, 80, 22, 40])
def test_region_decode_five_fractional_anchors(tmp_path, classes, dtype, options):
    cfg = str(tmp_path / "region.cfg")
    with open(cfg, "w") as fh:
        fh.write(region_cfg(classes))
    params = _mini_params(cfg)
    ref = R.Restatement(cfg, params)
    frames = synth_frames(300 + classes, 2, 64, 64)
    net = yolov3.Darknet(cfg, device="cuda", dtype=dtype, keep_all=True, fuse=True, options=options).set_params(params)
    out = net.forward(R.frames_to_input(frames)) if dtype == "float32" else net.forward_frames(frames)
    torch.cuda.synchronize()
    kernels = [r["kernel"] for r in net.plan_report()[-2:]]
    fused = kernels[1].startswith("(fused")
    print("region head", classes, "classes", dtype, options, kernels)
    assert out["bbox_xywh"].shape == (2, 5 * 8 * 8, 4)
    assert not fused or (dtype != "float32" and options.get("fuse_head", 1) != 0 and 128 < 5 * (5 + classes) <= 256)
    if fused:
        emulate = MODES[dtype]["emulate"]
        logits = ref.conv(REGION_HEAD, net.block_output(REGION_HEAD - 1).cpu(), emulate)
    else:
        logits = net.block_output(REGION_HEAD).cpu()                   # the product's own float32 logits
    box, prob, idx = ref.decode(REGION_HEAD + 1, logits)
    what = "%d classes %s %s (%s)" % (classes, dtype, options, kernels)
    torch.testing.assert_close(out["bbox_xywh"].cpu(), box, rtol=2e-4, atol=2e-5, msg=lambda m: what + " boxes: " + m)
    torch.testing.assert_close(out["class_prob"].cpu(), prob, rtol=5e-4, atol=2e-5, msg=lambda m: what + " scores: " + m)
    differ = out["class_idx"].cpu() != idx
    if fused:
        differ &= _margin(logits, 5) > 1e-3
    assert int(differ.sum()) == 0, what + ": classes differ"
    # the anchors really are in cells: Darknet's exp(tw) * a / grid, not pixels over the net size
    a = torch.tensor(ANCHORS, dtype=torch.float32)
    tw = logits.reshape(2, 5, 5 + classes, 8, 8)[:, :, 2:4].permute(0, 1, 3, 4, 2).reshape(2, 320, 2)
    want_wh = torch.exp(tw) * a.repeat_interleave(64, 0).unsqueeze(0) / 8
    torch.testing.assert_close(out["bbox_xywh"].cpu()[..., 2:], want_wh, rtol=2e-4, atol=2e-5)


# ------------------------------------------------------------------ whole networks

NETS = [("yolov2-tiny", 416), ("yolov2", 608), ("yolov2", 320)]
OBJ_BIAS = -5.0
_cache = {}


def _cfg(model):
    return os.path.join(MODEL_DIR, model + ".cfg")


def _params(model):
    if model not in _cache:
        blocks, net_info = parse_config(_cfg(model))
        _cache[model] = W.synth_params(blocks, net_info, seed=0, obj_bias=OBJ_BIAS, calib=W.load_calibration(model))
    return _cache[model]


def _frames(dim, n=2, seed=17):
    return synth_frames(seed, n, dim, dim)


def _reference_f32(model, dim):
    """the restatement's float32 forward, computed once per network and size and left unchanged"""
    key = (model, dim, "f32")
    if key not in _cache:
        _cache[key] = R.Restatement(_cfg(model), _params(model)).forward(R.frames_to_input(_frames(dim)))
    return _cache[key]


@pytest.mark.parametrize("model,dim", NETS)
def test_float32_matches_restatement(model, dim):
    net = yolov3.Darknet(_cfg(model), device="cuda", dtype="float32", keep_all=True, fuse=True).set_params(_params(model)).eval()
    got = net.forward(R.frames_to_input(_frames(dim)))
    torch.cuda.synchronize()
    want = _reference_f32(model, dim)
    g = dim // 32
    assert got["bbox_xywh"].shape == want["bbox_xywh"].shape == (2, 5 * g * g, 4)
    np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=SCORE_ATOL)
    assert float(got["class_prob"].max()) > 0.05                       # the procedural head does fire
    for i, blk in enumerate(net.blocks):
        if blk["type"] in ("reorg", "reorg3d"):
            assert torch.equal(net.block_output(i).cpu(), R.reorg_block(net.block_output(i - 1).cpu(), blk)), "reorg block %d" % i


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("model,dim", NETS)
def test_16bit_every_block_teacher_forced(model, dim, mode):
    rnd, emulate = MODES[mode]["rnd"], MODES[mode]["emulate"]
    frames = _frames(dim)
    net = yolov3.Darknet(_cfg(model), device="cuda", dtype=MODES[mode]["dtype"], keep_all=True, fuse=True)
    net.set_params(_params(model)).eval()
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    kernel_of = {}
    for r in net.plan_report():
        kernel_of.setdefault(r["block"], []).append(r["kernel"])
    assert not [k for ks in kernel_of.values() for k in ks if k.startswith("(fused")], kernel_of   # every block's tensor exists
    ref = R.Restatement(_cfg(model), net._params)
    blocks = ref.blocks
    x_net = rnd(R.frames_to_input(frames))

    def hip(i):
        return x_net if i < 0 else net.block_output(i).cpu()

    checked = 0
    for i, blk in enumerate(blocks):
        kind = blk["type"]
        what = "%s %s at %d block %d (%s, %s)" % (mode, model, dim, i, kind, ",".join(kernel_of.get(i, ["-"])))
        if kind == "convolutional":
            if i == 0 and kernel_of[0][0].startswith("conv_stem3x3"):
                # the VALU stem computes in float32 from the bytes and float32 weights; only its output is stored in 16 bits
                y = ref.conv(0, R.frames_to_input(frames))
            else:
                y = ref.conv(i, hip(i - 1), emulate)
            if blocks[i + 1]["type"] == "region":
                # the head: its float32 logits are not stored rounded.  The rows against the decode of the restatement's logits
                # (classes on clear soft-max margins, as test_gpu_yolov4.py gates its heads), then against the decode of the
                # product's own logits (classes identical)
                for logits, own in ((y, False), (hip(i), True)):
                    box, prob, idx = ref.decode(i + 1, logits)
                    tag = what + (" own logits" if own else " restated logits")
                    torch.testing.assert_close(out["bbox_xywh"].cpu(), box, rtol=2e-4, atol=2e-5, msg=lambda m: tag + " boxes: " + m)
                    torch.testing.assert_close(out["class_prob"].cpu(), prob, rtol=5e-4, atol=2e-5, msg=lambda m: tag + " scores: " + m)
                    differ = out["class_idx"].cpu() != idx
                    if not own:
                        differ &= _margin(logits, 5) > 1e-3
                    assert int(differ.sum()) == 0, tag + ": classes differ"
            else:
                _close_bf16(hip(i), rnd(y), what, None, mode)
        elif kind == "maxpool":
            assert torch.equal(hip(i), orc.maxpool(hip(i - 1), blk["size"], blk["stride"])), what
        elif kind == "route":
            assert torch.equal(hip(i), torch.cat([hip(j) for j in blk["layers"]], dim=1)), what
        elif kind in ("reorg", "reorg3d"):
            assert torch.equal(hip(i), R.reorg_block(hip(i - 1), blk)), what      # bit-exact
        elif kind == "region":
            continue
        else:
            raise AssertionError(what)
        checked += 1
    assert checked == len(blocks) - 1


# ------------------------------------------------------------------ callers

def test_tiny_detect_in_frames_cli_and_multi_label(tmp_path):
    model = "yolov2-tiny"
    weights = str(tmp_path / "yolov2-tiny.weights")
    W.write_darknet_weights(weights, _params(model), header=np.array([0, 1, 0, 0], dtype=np.int32))    # a version 0.1 file
    net = yolov3.Darknet(_cfg(model), device="cuda", dtype="bf16").load_weights(weights).eval()
    assert net.header.tolist() == [0, 1, 0, 0]
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES[:5]]
    img = os.path.join(GOLDEN, "images", SAMPLE_IMAGES[0])
    for letterbox in (False, True):
        streamed = list(yolov3.detect_in_frames(net, images, batch_size=4, letterbox=letterbox))
        assert len(streamed) == len(images)
        for f in (0, 4):
            one = yolov3.inference(net, images[f], device="cuda", letterbox=letterbox)[0]
            for a, b in zip(streamed[f], one):
                assert np.array_equal(np.asarray(a), np.asarray(b)), "frame %d" % f
        dump = tmp_path / ("det%d.json" % letterbox)
        cmd = [sys.executable, "-m", "yolov3", "-c", _cfg(model), "-w", weights, "-I", img, "--dtype", "bf16", "-p", "0.05",
               "--json", str(dump)] + (["--letterbox"] if letterbox else [])
        res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300,
                             env=dict(os.environ, PYTHONPATH=os.path.join(ROOT, "pytorch-yolov3_amd")))
        assert res.returncode == 0, res.stderr[-2000:]
        with open(dump) as fh:
            coco = json.load(fh)
        tlbr, prob, cls = streamed[0]
        assert len(coco["annotations"]) == len(prob) > 0
        got = sorted((a["category_id"], a["score"], tuple(a["bbox"])) for a in coco["annotations"])
        want = sorted((int(c), float(p), (int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])))
                      for b, p, c in zip(tlbr.tolist(), prob.tolist(), cls.tolist()))
        assert got == want
    with pytest.raises(ValueError, match=r"region block 15: multi_label"):
        yolov3.Darknet(_cfg(model), device="cuda", scores="darknet", multi_label=True)
