"""Mish on every conv kernel family and scale_x_y on every decode path (-m gpu), on a small network made for it.

FAMILY_CFG is a mish network whose layers, under the option sets of FAMILY_RUNS, reach every kernel family the plans can
pick for a conv: the VALU and MFMA stems, the three implicit GEMMs, the halo strip kernel and its direct-weights form, the
patch kernel, the weights-resident and direct-weights 1x1 kernels, the small-grid kernel (1x1 and 3x3), with and without a
fused shortcut, in float32, bf16 and fp16; its head has scale_x_y = 1.05 and runs on the float32 decode, the four-lane 16-bit
decode and both fused head kernels.

Gates.  float32: every mish conv of the plan run once more as a linear op on the same input (same sums) gives the
pre-activation t; the plan must hold F.mish(t) (+ the shortcut operand) within 4 float32 ulp or 1e-6.  16-bit: each block fed with the
product's own input against the restatement (tests/yolov4_restate.py) at one storage ulp, as test_gpu_bf16.py gates its
blocks.  Decode: the head's rows against the restatement's decode of the product's float32 logits; at scale_x_y = 1 the
boxes are bit-identical to those of a zero (unset) y3_op.scale_x_y.
"""
import ctypes

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

import yolov4_restate as R
from test_gpu_bf16 import MODES, _close_bf16

pytestmark = pytest.mark.gpu


def _conv(f, k, s=1, act="mish", bn=True):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=%d\npad=1\nactivation=%s\n\n" % (
        "batch_normalize=1\n" if bn else "", f, k, s, act)


FAMILY_CFG = ("[net]\nwidth=288\nheight=288\nchannels=3\n\n" +
              _conv(32, 3) +                      # 0  stem: MFMA stem (uint8 frames, 16-bit) / VALU stem (float32)
              _conv(64, 3, 2) +                   # 1  3x3 stride 2
              _conv(128, 1) +                     # 2  1x1 64 -> 128 at 144^2
              _conv(128, 1) +                     # 3  1x1 128 -> 128
              _conv(128, 3) +                     # 4  3x3 128 -> 128 at 144^2 (+ shortcut): patch / halo / implicit GEMMs
              "[shortcut]\nfrom=-3\nactivation=linear\n\n" +   # 5
              _conv(256, 3, 2) +                  # 6  3x3 stride 2 -> 72^2
              _conv(256, 1) +                     # 7
              _conv(256, 3) +                     # 8  3x3 256 -> 256 at 72^2 (+ shortcut)
              "[shortcut]\nfrom=-2\nactivation=linear\n\n" +   # 9
              _conv(1024, 1) +                    # 10 1x1 256 -> 1024
              _conv(256, 1) +                     # 11 1x1 1024 -> 256 (deep K)
              _conv(255, 1, act="linear", bn=False) +          # 12 head
              "[yolo]\nmask=0,1,2\nanchors=10,14, 23,27, 37,58\nclasses=80\nnum=3\nscale_x_y=1.05\n")
FAMILY_DIM = 288
HEAD = 12
_D = _hip.AM_DEFAULT
# (name, plan options, batch)
FAMILY_RUNS = (
    ("default", {}, 2),
    ("default_b16", {}, 16),
    ("igemm1", {"auto_mask": 0, "igemm_version": 1}, 2),
    ("igemm2", {"auto_mask": 0, "igemm_version": 2}, 2),
    ("igemm3", {"auto_mask": 0, "igemm_version": 3, "fuse_head": 2}, 2),
    ("halo", {"auto_mask": _hip.AM_HALO_ALL | _hip.AM_NO_SMALL_GRID, "fuse_head": 0}, 2),
    ("halo_dw", {"auto_mask": _D | _hip.AM_HALO_DW_ALWAYS | _hip.AM_NO_SMALL_GRID, "fuse_head": 3}, 4),
    ("wres", {"auto_mask": (_D & ~_hip.AM_SMALL_DW) | _hip.AM_WRES_ALWAYS, "fuse_head": 4}, 2),
    ("small_dw", {"auto_mask": _D | _hip.AM_SMALL_DW_ALWAYS}, 1),
)
# kernel-name fragments the runs must cover, per dtype
FAMILIES_16 = ("conv_stem_mfma", "conv_igemm_", "conv_igemm2", "conv_igemm3", "conv_halo_ws", "conv_halo_dw", "conv_patch",
               "conv1x1_wres", "conv1x1_dw", "conv_dw48_k1", "conv_dw48_k3", "head_decode")
FAMILIES_32 = ("conv_stem3x3", "conv_igemm_", "conv_igemm2", "conv_igemm3", "conv_halo_ws", "conv_patch")


def _write(tmp_path, text, name):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _params(cfg):
    blocks, net_info = parse_config(cfg)
    calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
    return W.synth_params(blocks, net_info, seed=7, obj_bias=-4.0, calib=calib)


def _net(cfg, dtype, params, options):
    return yolov3.Darknet(cfg, device="cuda", dtype=dtype, keep_all=True, fuse=True, options=options).set_params(params)


def _run(net, frames, f32_input):
    if f32_input:
        out = net.forward(R.frames_to_input(frames))
    else:
        out = net.forward_frames(frames)
    torch.cuda.synchronize()
    return out


def _ulp_close(got, want, what):
    got, want = got.double(), want.double()
    d = (got - want).abs()
    tol = torch.maximum(4 * torch.from_numpy(R.f32_ulp(want.float().numpy())).double(), torch.full_like(d, 1e-6))
    worst = float((d / tol).max())
    assert worst <= 1.0, "%s: |d| up to %.2f x (4 ulp or 1e-6), max |d| %.3g" % (what, worst, float(d.max()))


@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_mish_on_every_conv_family(tmp_path, dtype):
    _mish_on_the_family_network(tmp_path, dtype, FAMILY_DIM, True)


@pytest.mark.parametrize("dim", [32, 4])
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_mish_on_small_maps(tmp_path, dtype, dim):
    """The same network, runs and gates at a 32-pixel input (maps of 32, 16 and 8 pixels: the network's stride is 4) and at a
    4-pixel one, whose maps are 4 x 4, 2 x 2 and 1 x 1: mish, the fused shortcut and the scale_x_y head on one cell.  Which
    kernel takes a layer differs from the 288-pixel run's (no map is wide enough for the patch kernel), so the list of families
    is not asked for here: tests/test_gpu_tiny_maps.py and the footprint rows hold kernels to maps."""
    _mish_on_the_family_network(tmp_path, dtype, dim, False)


def _mish_on_the_family_network(tmp_path, dtype, dim, every_family):
    cfg = _write(tmp_path, FAMILY_CFG, "family.cfg")
    params = _params(cfg)
    ref = R.Restatement(cfg, params)
    blocks = ref.blocks
    rounds = ref.rounding_points()
    seen = set()
    for name, options, batch in FAMILY_RUNS:
        frames = synth_frames(500 + batch, batch, dim, dim)
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

        if dtype == "float32":
            # each mish conv once more as a LINEAR op on the same input (y3_op_run: no shortcut, own output buffer); the MFMA
            # kernels all sum in one K order and the stems are one kernel, so this is the pre-activation the plan's kernel had
            lib = _hip.lib()
            x_in = R.frames_to_input(frames).cuda()
            cp = net._last_plan
            for n in range(cp.n_ops):
                op = cp.ops[n]
                if op.kind != _hip.OP_CONV or not op.flags & _hip.F_MISH:
                    continue
                i = op.block_idx
                lin = _hip.Y3Op()
                ctypes.memmove(ctypes.byref(lin), ctypes.byref(op), ctypes.sizeof(lin))
                lin.flags &= ~(_hip.F_MISH | _hip.F_RESIDUAL | _hip.F_FUSE_NEXT)
                lin.d_res = None
                buf = torch.zeros(batch * op.out_h * op.out_w * op.out_ld, dtype=torch.float32, device="cuda")
                lin.d_out = buf.data_ptr()
                _hip.check(lib.y3_op_run(ctypes.byref(lin), x_in.data_ptr(), net._zero.data_ptr(), _hip.stream_ptr()))
                torch.cuda.synchronize()
                t = buf.view(batch, op.out_h, op.out_w, op.out_ld)[..., :op.out_c].permute(0, 3, 1, 2)[sel].cpu()
                what = "%s block %d (%s)" % (name, i, kernel_of[i][0])
                if op.flags & _hip.F_RESIDUAL:
                    sc = i + 1
                    m = torch.nn.functional.mish(t)
                    want = m + hip(sc + blocks[sc]["from"])
                    d = (hip(sc).double() - want.double()).abs()
                    tol = torch.maximum(4 * torch.from_numpy(R.f32_ulp(m.numpy()) + R.f32_ulp(want.numpy())).double(),
                                        torch.full_like(d, 1e-6))
                    assert float((d / tol).max()) <= 1.0, what + " + shortcut: max |d| %.3g" % float(d.max())
                else:
                    _ulp_close(hip(i), torch.nn.functional.mish(t), what)
                # and the restatement from the product's input, at the float32 gate of test_gpu_parity.py
                want = ref.conv(i, hip(i - 1))
                if op.flags & _hip.F_RESIDUAL:
                    want = want + hip(i + 1 + blocks[i + 1]["from"])
                    i += 1
                np.testing.assert_allclose(hip(i).numpy(), want.numpy(), rtol=1e-4, atol=2e-5, err_msg=what)
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
        # the head: decode (scale_x_y 1.05) of the restatement's logits from the product's head input
        logits = ref.conv(HEAD, hip(HEAD - 1), None if dtype == "float32" else MODES[dtype]["emulate"])
        box, prob, _ = ref.decode(HEAD + 1, logits)
        what = "%s %s head (%s)" % (dtype, name, kernel_of[HEAD][0])
        torch.testing.assert_close(out["bbox_xywh"][sel].cpu(), box, rtol=2e-4, atol=2e-5, msg=lambda m: what + ": " + m)
        torch.testing.assert_close(out["class_prob"][sel].cpu(), prob, rtol=5e-4, atol=2e-5, msg=lambda m: what + ": " + m)
        del net
    if not every_family:
        return
    want = FAMILIES_32 if dtype == "float32" else tuple(f.replace("bf16", MODES[dtype]["tag"]) for f in FAMILIES_16)
    missing = [f for f in want if not any(f in k for k in seen)]
    assert not missing, "kernel families not exercised: %s (seen %s)" % (missing, sorted(seen))


@pytest.mark.parametrize("dtype,options", [("float32", {}), ("bf16", {"fuse_head": 0}), ("bf16", {"fuse_head": 2}),
                                           ("bf16", {"fuse_head": 3}), ("fp16", {"fuse_head": 0})])
def test_scale_x_y_decode(tmp_path, dtype, options):
    """The float32 decode, the four-lane 16-bit decode and both fused head kernels against the restatement at s = 1.05; at
    s = 1 every path gives the bits of an op whose scale_x_y is left at zero (the decode before scale_x_y existed)."""
    cfg = _write(tmp_path, FAMILY_CFG, "family.cfg")
    params = _params(cfg)
    ref = R.Restatement(cfg, params)
    frames = synth_frames(77, 2, FAMILY_DIM, FAMILY_DIM)
    net = _net(cfg, dtype, params, options)
    out = _run(net, frames, dtype == "float32")
    kern = net.plan_report()[-2:]
    x = net.block_output(HEAD - 1).cpu()
    logits = ref.conv(HEAD, x, None if dtype == "float32" else MODES[dtype]["emulate"])
    box, prob, idx = ref.decode(HEAD + 1, logits)
    what = "%s %s (%s)" % (dtype, options, [k["kernel"] for k in kern])
    got = out["bbox_xywh"].cpu()
    torch.testing.assert_close(got, box, rtol=2e-4, atol=2e-5, msg=lambda m: what + ": " + m)
    torch.testing.assert_close(out["class_prob"].cpu(), prob, rtol=5e-4, atol=2e-5, msg=lambda m: what + ": " + m)
    # the centre really is stretched: up to 0.05 * 0.5 / 72 = 3.5e-4 away from the s = 1 decode at this 72 x 72 head
    box1, _, _ = R.yolo_decode(logits, [(10, 14), (23, 27), (37, 58)], 1.0)
    assert float((got[..., :2] - box1[..., :2]).abs().max()) > 2.5e-4

    # s = 1 against s = 0 (unset): the compiled ops with the head's field set, as plans of their own on the same buffers
    lib = _hip.lib()
    cp = net._last_plan
    opt = _hip.options(**options) if options else None
    x_in = (R.frames_to_input(frames) if dtype == "float32" else torch.from_numpy(frames)).cuda()
    outs = []
    for s in (1.0, 0.0):
        ops = (_hip.Y3Op * cp.n_ops)()
        ctypes.memmove(ops, cp.ops, ctypes.sizeof(ops))
        for n in range(cp.n_ops):
            if ops[n].kind == _hip.OP_YOLO:
                ops[n].scale_x_y = s
        h = ctypes.c_void_p()
        _hip.check(lib.y3_plan_create_ex(ops, cp.n_ops, net._zero.data_ptr(), ctypes.byref(opt) if opt is not None else None,
                                         ctypes.byref(h)))
        try:
            _hip.check(lib.y3_plan_run(h, x_in.data_ptr(), _hip.stream_ptr()))
            torch.cuda.synchronize()
        finally:
            lib.y3_plan_destroy(h)
        outs.append((cp.bbox.cpu().numpy().tobytes(), cp.prob.cpu().numpy().tobytes()))
    assert outs[0] == outs[1], what
    assert np.frombuffer(outs[0][0], dtype=np.float32).size == got.numel()
