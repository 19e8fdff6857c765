"""Logistic on every conv kernel family, the new_coords decode on every decode path, and yolov4-csp end to end (-m gpu).

Logistic: test_gpu_yolov4_families.py's family network and option sets (FAMILY_RUNS) with activation=logistic, and six
channels of every BN conv driven to +-20, +-90 and +-inf.  float32: each logistic conv run once more as a linear op on the
same input gives the pre-activation t, and the plan must hold torch.sigmoid(t) (+ the shortcut operand) within 4 float32 ulp
or 1e-6; 16-bit: every block fed with the product's own input against tests/new_coords_restate.py at one storage ulp.

new_coords: a small network whose logistic head feeds a [yolo] block with new_coords=1, for several class counts, in float32
(sequential decode) and bf16 / fp16 with fuse_head 0 (four-lane decode), 2 (tiled fused head), 1 / 3 / 4 (direct-weights
fused head where the shape allows).  Every path is bit-identical to the restatement's decode of the product's own head-conv
output (the fuse_head=0 plan stores it), so in 16-bit the fused and the two-kernel paths give identical bits.
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
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

import new_coords_restate as NR
import yolov4_restate as R
from golden_util import GOLDEN, MODEL_DIR, SAMPLE_IMAGES, load_jpeg_bgr
from test_gpu_bf16 import MODES, _close_bf16
from test_gpu_parity import BOX_ATOL, SCORE_ATOL
from test_gpu_yolov4_families import (FAMILIES_16, FAMILIES_32, FAMILY_CFG, FAMILY_DIM, FAMILY_RUNS, HEAD, _conv, _net, _run,
                                      _ulp_close, _write)

pytestmark = pytest.mark.gpu

EXTREMES = (20.0, -20.0, 90.0, -90.0, float("inf"), float("-inf"))
LOGISTIC_CFG = FAMILY_CFG.replace("activation=mish", "activation=logistic")


def _params(cfg, seed=7, extremes=False):
    blocks, net_info = parse_config(cfg)
    calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
    params = W.synth_params(blocks, net_info, seed=seed, obj_bias=-4.0, calib=calib)
    if extremes:
        for p in params:
            if "bn_beta" in p:        # the BN shift, so the folded bias and the pre-activation, is driven there
                p["bn_beta"] = p["bn_beta"].copy()
                p["bn_beta"][:len(EXTREMES)] = EXTREMES
    return params


@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_logistic_on_every_conv_family(tmp_path, dtype):
    cfg = _write(tmp_path, LOGISTIC_CFG, "family.cfg")
    params = _params(cfg, extremes=True)
    ref = NR.Restatement(cfg, params)
    blocks = ref.blocks
    rounds = ref.rounding_points()
    seen = set()
    for name, options, batch in FAMILY_RUNS:
        frames = synth_frames(600 + batch, batch, FAMILY_DIM, FAMILY_DIM)
        net = _net(cfg, dtype, params, options)
        out = _run(net, frames, dtype == "float32")
        report = net.plan_report()
        kernel_of = {}
        for r in report:
            kernel_of.setdefault(r["block"], []).append(r["kernel"])
        seen.update(r["kernel"] for r in report)
        for i, blk in enumerate(blocks):
            if blk["type"] == "convolutional":
                assert not kernel_of[i][0].startswith("(fused") or i == HEAD, (name, i, kernel_of[i])
        sel = [0, batch - 1] if batch > 2 else list(range(batch))

        def hip(i):
            if i < 0:
                x = R.frames_to_input([frames[j] for j in sel])
                return x if dtype == "float32" else MODES[dtype]["rnd"](x)
            return net.block_output(i)[sel].cpu()

        for i, blk in enumerate(blocks):
            if blk["type"] == "convolutional" and i != HEAD and rounds[i]:
                y = hip(i)
                what = "%s %s block %d (%s)" % (dtype, name, i, kernel_of[i][0])
                assert not torch.isnan(y).any(), what
                # saturated channels, exactly: pre-activations near +90 and +inf give 1, -inf gives 0
                assert bool((y[:, 2] == 1).all() and (y[:, 4] == 1).all() and (y[:, 5] == 0).all()), what
        if dtype == "float32":
            lib = _hip.lib()
            x_in = R.frames_to_input(frames).cuda()
            cp = net._last_plan
            n_log = 0
            for n in range(cp.n_ops):
                op = cp.ops[n]
                if op.kind != _hip.OP_CONV or not op.flags & _hip.F_LOGISTIC:
                    continue
                n_log += 1
                i = op.block_idx
                lin = _hip.Y3Op()
                ctypes.memmove(ctypes.byref(lin), ctypes.byref(op), ctypes.sizeof(lin))
                lin.flags &= ~(_hip.F_LOGISTIC | _hip.F_RESIDUAL | _hip.F_FUSE_NEXT)
                lin.d_res = None
                buf = torch.zeros(batch * op.out_h * op.out_w * op.out_ld, dtype=torch.float32, device="cuda")
                lin.d_out = buf.data_ptr()
                _hip.check(lib.y3_op_run(ctypes.byref(lin), x_in.data_ptr(), net._zero.data_ptr(), _hip.stream_ptr()))
                torch.cuda.synchronize()
                t = buf.view(batch, op.out_h, op.out_w, op.out_ld)[..., :op.out_c].permute(0, 3, 1, 2)[sel].cpu()
                what = "%s block %d (%s)" % (name, i, kernel_of[i][0])
                # the logits really reach +-20, +-90 and +-inf
                assert bool((t[:, 4] == float("inf")).all() and (t[:, 5] == float("-inf")).all()), what
                assert float(t[:, 2].min()) > 80 and float(t[:, 3].max()) < -80, what
                assert float(t[:, 0].min()) > 10 and float(t[:, 1].max()) < -10, what
                if op.flags & _hip.F_RESIDUAL:
                    sc = i + 1
                    m = torch.sigmoid(t)
                    want = m + hip(sc + blocks[sc]["from"])
                    d = (hip(sc).double() - want.double()).abs()
                    tol = torch.maximum(4 * torch.from_numpy(R.f32_ulp(m.numpy()) + R.f32_ulp(want.numpy())).double(),
                                        torch.full_like(d, 1e-6))
                    assert float((d / tol).max()) <= 1.0, what + " + shortcut: max |d| %.3g" % float(d.max())
                else:
                    _ulp_close(hip(i), torch.sigmoid(t), what)
            assert n_log == sum(1 for i, b in enumerate(blocks) if b["type"] == "convolutional" and i != HEAD)
        else:
            rnd = MODES[dtype]["rnd"]
            emulate = MODES[dtype]["emulate"]
            for i, blk in enumerate(blocks):
                if blk["type"] != "convolutional" or i == HEAD:
                    continue
                y = ref.conv(i, hip(i - 1), emulate)
                what = "%s %s block %d (%s)" % (dtype, name, i, kernel_of[i][0])
                if not rounds[i]:
                    sc = i + 1
                    _close_bf16(hip(sc), rnd(y + hip(sc + blocks[sc]["from"])), what + " + shortcut", None, dtype)
                else:
                    _close_bf16(hip(i), rnd(y), what, None, dtype)
        assert bool(torch.isfinite(out["class_prob"]).all())
        del net
    want = FAMILIES_32 if dtype == "float32" else tuple(f.replace("bf16", MODES[dtype]["tag"]) for f in FAMILIES_16)
    missing = [f for f in want if not any(f in k for k in seen)]
    assert not missing, "kernel families not exercised: %s (seen %s)" % (missing, sorted(seen))


def _nc_cfg(classes, cin, sxy):
    """a small mish network with a logistic head (3 anchors, ``classes`` classes, ``cin`` input channels) read by a
    new_coords [yolo] block"""
    return ("[net]\nwidth=128\nheight=128\nchannels=3\n\n" + _conv(32, 3) + _conv(64, 3, 2) + _conv(128, 3, 2) +
            _conv(cin, 1) + _conv(3 * (5 + classes), 1, act="logistic", bn=False) +
            "[yolo]\nmask=0,1,2\nanchors=10,14, 23,27, 37,58\nclasses=%d\nnum=3\nscale_x_y=%s\nnew_coords=1\n" % (classes, sxy))


NC_HEAD = 4
# (classes, head input channels, scale_x_y): 255 and 150 channels take the fused head kernels; 36 the two-kernel path
NC_CASES = ((80, 256, "2.0"), (45, 512, "1.05"), (7, 256, "2.0"))


def _bits(out):
    return tuple(out[k].cpu().numpy().tobytes() for k in ("bbox_xywh", "class_prob", "class_idx"))


@pytest.mark.parametrize("classes,cin,sxy", NC_CASES)
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_new_coords_decode_every_path(tmp_path, dtype, classes, cin, sxy):
    cfg = _write(tmp_path, _nc_cfg(classes, cin, sxy), "nc.cfg")
    params = _params(cfg, seed=3)
    ref = NR.Restatement(cfg, params)
    frames = synth_frames(91, 4, 128, 128)
    heads = (0,) if dtype == "float32" else (0, 1, 2, 3, 4)
    outs, names = {}, {}
    for fh in heads:
        net = _net(cfg, dtype, params, {"fuse_head": fh})
        outs[fh] = _run(net, frames, dtype == "float32")
        names[fh] = [r["kernel"] for r in net.plan_report()][-2:]
        if fh == 0:
            probs = net.block_output(NC_HEAD).cpu()       # the head conv's own (logistic) output
        del net
    assert float(probs.min()) >= 0.0 and float(probs.max()) <= 1.0
    box, prob, idx = ref.decode(NC_HEAD + 1, probs)
    want = (box.numpy().tobytes(), prob.numpy().tobytes(), idx.numpy().astype(np.int64).tobytes())
    for fh in heads:
        assert _bits(outs[fh]) == want, "%s classes %d fuse_head %d (%s): not bit-identical to the restated decode" % (
            dtype, classes, fh, names[fh])
    if dtype != "float32" and classes >= 40:
        assert all("head_decode" in names[fh][0] for fh in (1, 2, 3, 4)), names
        assert "head_decode_dw" in names[3][0] and "head_decode_dw" not in names[2][0], names


def test_new_coords_flag_reaches_the_decode(tmp_path):
    """The same logistic head with and without new_coords decodes differently on the fused path."""
    text = _nc_cfg(80, 256, "2.0")
    cfg = _write(tmp_path, text, "nc.cfg")
    cfg_old = _write(tmp_path, text.replace("new_coords=1\n", ""), "old.cfg")
    params = _params(cfg, seed=3)
    frames = synth_frames(92, 2, 128, 128)
    a = _run(_net(cfg, "bf16", params, {}), frames, False)
    b = _run(_net(cfg_old, "bf16", params, {}), frames, False)
    assert not torch.equal(a["bbox_xywh"], b["bbox_xywh"])


# ---- yolov4-csp end to end --------------------------------------------------------------------------------------------

CSP = os.path.join(MODEL_DIR, "yolov4-csp.cfg")
OBJ_BIAS = -5.0


def _csp_params():
    blocks, net_info = parse_config(CSP)
    return W.synth_params(blocks, net_info, seed=0, obj_bias=OBJ_BIAS, calib=W.load_calibration("yolov4-csp"))


def _csp_net(dtype, params, **kw):
    return yolov3.Darknet(CSP, device="cuda", dtype=dtype, **kw).set_params(params).eval()


@pytest.mark.parametrize("dim", [512, 320])
def test_csp_float32_matches_restatement(dim):
    params = _csp_params()
    net = _csp_net("float32", params)
    ref = NR.Restatement(CSP, params)
    frames = synth_frames(13, 2, dim, dim)
    got = net.forward(R.frames_to_input(frames))
    want = ref.forward(R.frames_to_input(frames))
    assert got["bbox_xywh"].shape == want["bbox_xywh"].shape
    np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=SCORE_ATOL)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_csp_16bit_every_conv_teacher_forced(mode):
    """Every conv of yolov4-csp at 512, fed with the product's own input, at one storage ulp (the float32 logistic heads within
    1e-4); the three heads' decode bit-identical to the restatement's decode of the product's own head outputs (a fuse_head=0
    plan), and the default plan, which fuses all three heads, bit-identical to that."""
    rnd, emulate = MODES[mode]["rnd"], MODES[mode]["emulate"]
    params = _csp_params()
    frames = synth_frames(21, 2, 512, 512)
    net = _csp_net(MODES[mode]["dtype"], params, keep_all=True, fuse=True, options={"fuse_head": 0})
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    ref = NR.Restatement(CSP, params)
    blocks, rounds = ref.blocks, ref.rounding_points()
    x_net = rnd(R.frames_to_input(frames))

    def hip(i):
        return x_net if i < 0 else net.block_output(i).cpu()

    checked, dec = 0, []
    for i, blk in enumerate(blocks):
        if blk["type"] == "convolutional":
            y = ref.conv(i, hip(i - 1), emulate)
            what = "%s yolov4-csp block %d" % (mode, i)
            if blk["activation"] == "logistic":
                np.testing.assert_allclose(hip(i).numpy(), y.numpy(), rtol=1e-3, atol=1e-4, err_msg=what)
            elif not rounds[i]:
                sc = i + 1
                _close_bf16(hip(sc), rnd(y + hip(sc + blocks[sc]["from"])), what + " + shortcut", None, mode)
            else:
                _close_bf16(hip(i), rnd(y), what, None, mode)
            checked += 1
        elif blk["type"] == "yolo":
            dec.append(ref.decode(i, hip(i - 1)))
    assert checked == 115
    want = [torch.cat([d[k] for d in dec], 1) for k in range(3)]
    assert out["bbox_xywh"].cpu().numpy().tobytes() == want[0].numpy().tobytes()
    assert out["class_prob"].cpu().numpy().tobytes() == want[1].numpy().tobytes()
    assert torch.equal(out["class_idx"].cpu(), want[2])
    del net
    fused = _csp_net(MODES[mode]["dtype"], params)
    got = fused.forward_frames(frames)
    torch.cuda.synchronize()
    assert sum("head_decode" in r["kernel"] for r in fused.plan_report()) == 3
    assert _bits(got) == _bits(out)


def test_csp_detect_in_frames_and_cli(tmp_path):
    params = _csp_params()
    weights = str(tmp_path / "csp.weights")
    W.write_darknet_weights(weights, params)
    net = yolov3.Darknet(CSP, device="cuda", dtype="bf16").load_weights(weights).eval()
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES[:3]] * 6             # 18 frames: a full batch and a partial one
    streamed = list(yolov3.detect_in_frames(net, images, batch_size=16))
    assert len(streamed) == len(images)
    for f in (0, 1, 17):
        one = yolov3.inference(net, images[f], device="cuda")[0]
        for a, b in zip(streamed[f], one):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "frame %d" % f
    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    img = os.path.join(GOLDEN, "images", SAMPLE_IMAGES[0])
    dump = tmp_path / "det.json"
    cmd = [sys.executable, "-m", "yolov3", "-c", CSP, "-w", weights, "-I", img, "--dtype", "bf16", "-p", "0.05",
           "--json", str(dump)]
    res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, PYTHONPATH=os.path.join(root, "pytorch-yolov3_amd")))
    assert res.returncode == 0, res.stderr[-2000:]
    with open(dump) as fh:
        coco = json.load(fh)
    assert len(coco["images"]) == 1 and coco["annotations"]
    assert all(0 <= a["category_id"] < 80 for a in coco["annotations"])
