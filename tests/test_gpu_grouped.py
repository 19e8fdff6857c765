"""Grouped and depthwise convs on the GPU (-m gpu): csrc/conv_grouped.hip through ``y3_op_run``, through ``Darknet`` on
tests/golden/cfg/grouped.cfg, and on strided slices of poisoned buffers.

* One-op cases (tests/grouped_cases.py), float32 / bf16 / fp16, each against the restatement (tests/grouped_restate.py: the
  oracle's conv_block per group) computed from the same input: float32 under ``F32_BLOCK_TOL``, the 16-bit modes under
  ``_close_bf16`` at one storage ulp (tests/test_gpu_bf16.py).  tests/test_grouped_host.py shows on the CPU that the gates fit.
  Every linear and leaky case must also be, bit for bit, the float32 restatement in the kernels' stated sum order
  (tests/grouped_ordered.py); mish and logistic cases (``GC.NOT_ORDERED``) stay on the gates above.
* Every depthwise case again under ``grouped_generic``: ``conv_grouped_*`` gives the bits ``conv_dwise_*`` gave.
* grouped.cfg block by block, teacher-forced, as tests/test_gpu_odd_cfg.py walks odd.cfg; which kernel ran which block; the arena
  against ``keep_all=True``; two runs of one plan.
* The footprint of every kernel instance, as tests/test_gpu_footprint.py takes it, with the launch census: the kernels are
  compiled into libyolov3_hip_grouped.so, whose census is tests/golden/kernel_instances_grouped.json.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.synthdata import synth_frames

import footprint_util as fu
import grouped_cases as GC
import grouped_ordered as GO
import grouped_restate as GR
import kernel_census as census
from golden_util import GOLDEN
from test_gpu_bf16 import F32_BLOCK_TOL, MODES, _close_bf16

pytestmark = pytest.mark.gpu

CFG = os.path.join(GOLDEN, "cfg", "grouped.cfg")
TAG = {"float32": "f32", "bf16": "bf16", "fp16": "f16"}
DT_CODE = {"float32": _hip.Y3_F32, "bf16": _hip.Y3_BF16, "fp16": _hip.Y3_F16}
ACT_FLAG = {"leaky": _hip.F_LEAKY, "linear": 0, "mish": _hip.F_MISH, "logistic": _hip.F_LOGISTIC}
_ref_cache = {}


def _nhwc(t, tdt):
    return t.permute(0, 2, 3, 1).contiguous().to(tdt)


def _reference(case, dtype):
    """(data, unrounded float32 reference) of a case: computed once, left unchanged"""
    key = (case["id"], dtype)
    if key not in _ref_cache:
        data = GC.make(case, dtype)
        _ref_cache[key] = (data, GC.reference(case, dtype, data))
    return _ref_cache[key]


def _kernel_name(case, dtype, generic):
    if GC.is_dwise(case) and not generic:
        form = "k3s%d" % case["s"] if case["k"] == 3 and case["s"] in (1, 2) else "kn"
        return "conv_dwise_%s_%s" % (TAG[dtype], form)
    return "conv_grouped_%s_%s" % (TAG[dtype], "oc8" if (case["cout"] // case["groups"]) % 8 == 0 else "oc1")


def _run_one_op(case, dtype, generic=False):
    """the case through y3_op_run -> (B, cout, ho, wo) float32 holding the stored values, and the kernel's name"""
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    tdt = GC.TORCH_DT[dtype]
    data, _ = _reference(case, dtype)
    B, cin, cout, k = case.get("B", 3), case["cin"], case["cout"], case["k"]
    ho, wo = GC.out_hw(case)
    (in_off, in_ld), (out_off, out_ld) = GC.strides(case, cin, dtype), GC.strides(case, cout, dtype)
    res_off, res_ld = (out_off + 8, out_ld + 16) if case.get("wide") else (out_off, out_ld)
    nan = float("nan")
    xin = torch.full((B, case["h"], case["w"], in_ld), nan, dtype=tdt, device=dev)
    xin[..., in_off:in_off + cin] = _nhwc(data["x"], tdt).to(dev)
    out = torch.full((B, ho, wo, out_ld), nan, dtype=tdt, device=dev)
    res = None
    if data["res"] is not None:
        res = torch.full((B, ho, wo, res_ld), nan, dtype=tdt, device=dev)
        res[..., res_off:res_off + cout] = _nhwc(data["res"], tdt).to(dev)
    with _hip.grouped_generic(generic):
        ops = (_hip.Y3Op * 1)()
        op = ops[0]
        op.kind, op.dtype, op.batch, op.block_idx = _hip.OP_CONV, DT_CODE[dtype], B, 1
        op.flags = ACT_FLAG[case.get("act", "leaky")] | (_hip.F_RESIDUAL if res is not None else 0)
        op.in_h, op.in_w, op.in_c, op.in_ld = case["h"], case["w"], cin, in_ld
        op.out_h, op.out_w, op.out_c, op.out_ld = ho, wo, cout, out_ld
        op.ksize, op.stride, op.pad, op.groups = k, case["s"], case["pad"], case["groups"]
        es = xin.element_size()
        op.d_in, op.d_out = xin.data_ptr() + in_off * es, out.data_ptr() + out_off * es
        if res is not None:
            op.d_res, op.res_ld = res.data_ptr() + res_off * es, res_ld
        op.cout_pad, op.k_ld = 128, 1 << 20                    # (provisional: the path does not depend on them)
        path = lib.y3_conv_path(ctypes.byref(op))
        assert path == (GC.PATH_DWISE if GC.is_dwise(case) and not generic else GC.PATH_GROUPED), (case["id"], path)
        host, op.cout_pad, op.k_ld = GC.device_weights(case, path, data["p"]["weight"])
        wdev = torch.from_numpy(host).to(tdt).to(dev)
        assert torch.equal(wdev.float().cpu(), torch.from_numpy(host))          # storage-exact weights
        sc, bi = torch.zeros(op.cout_pad), torch.zeros(op.cout_pad)
        sc[:cout], bi[:cout] = torch.from_numpy(data["scale"]), torch.from_numpy(data["bias"])
        sc, bi = sc.to(dev), bi.to(dev)
        op.d_weight, op.d_scale, op.d_bias = wdev.data_ptr(), sc.data_ptr(), bi.data_ptr()
        zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
        handle = ctypes.c_void_p()
        _hip.check(lib.y3_plan_create(ops, 1, zero.data_ptr(), ctypes.byref(handle)))
        name = lib.y3_plan_op_kernel(handle, 0).decode()
        lib.y3_plan_destroy(handle)
        _hip.check(lib.y3_op_run(ops, None, zero.data_ptr(), _hip.stream_ptr()))
    torch.cuda.synchronize()
    assert name == _kernel_name(case, dtype, generic), (case["id"], name)
    o = out.float().cpu()
    written = torch.zeros(out_ld, dtype=torch.bool)
    written[out_off:out_off + cout] = True
    assert bool(torch.isnan(o[..., ~written]).all()), "%s: wrote outside its channel slice" % case["id"]
    got = o[..., written]
    assert not bool(torch.isnan(got).any()), "%s: output elements left unwritten or NaN" % case["id"]
    return got.permute(0, 3, 1, 2).contiguous(), name


_ordered_cache = {}


def _ordered_gate(case, dtype, got, what):
    """linear and leaky ops: the stored bits are those of tests/grouped_ordered.py, the float32 restatement in the kernels' stated
    sum order.  True where the demand was made; mish and logistic cases (GC.NOT_ORDERED) are left out."""
    exact = case.get("act", "leaky") in GO.EXACT_ACTS
    assert exact == (case["id"] not in GC.NOT_ORDERED), case["id"]
    if not exact:
        return False
    key = (case["id"], dtype)
    if key not in _ordered_cache:
        _ordered_cache[key] = torch.from_numpy(GO.of_case(case, dtype, _reference(case, dtype)[0]))
    want = _ordered_cache[key]
    if not torch.equal(got, want):
        bad = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
        b, c, y, x = (int(v) for v in bad[0])
        pytest.fail("%s: %d of %d stored values are not the ordered restatement's; first at frame %d channel %d pixel (%d, %d): got %r (%08x), want %r (%08x)" % (
            what, len(bad), got.numel(), b, c, y, x, float(got[b, c, y, x]), int(got.view(torch.int32)[b, c, y, x]) & 0xffffffff,
            float(want[b, c, y, x]), int(want.view(torch.int32)[b, c, y, x]) & 0xffffffff))
    return True


def _gate(got, want_unrounded, dtype, what):
    if dtype == "float32":
        np.testing.assert_allclose(got.numpy(), want_unrounded.numpy(), err_msg=what, **F32_BLOCK_TOL)
    else:
        _close_bf16(got, MODES[dtype]["rnd"](want_unrounded), what, None, dtype)


@pytest.mark.parametrize("dtype", GC.DTYPES)
@pytest.mark.parametrize("cid", [c["id"] for c in GC.DWISE])
def test_depthwise_kernel_one_op(cid, dtype):
    case = GC.CASES[cid]
    got, name = _run_one_op(case, dtype)
    _gate(got, _reference(case, dtype)[1], dtype, "%s %s (%s)" % (cid, dtype, name))
    _ordered_gate(case, dtype, got, "%s %s (%s)" % (cid, dtype, name))
    # the same op on the grouped kernel: the same sum order, the same epilogue, the same bits
    again, other = _run_one_op(case, dtype, generic=True)
    assert other.startswith("conv_grouped_")
    _ordered_gate(case, dtype, again, "%s %s (%s)" % (cid, dtype, other))
    assert torch.equal(got, again), "%s %s: %s and %s differ in %d values" % (cid, dtype, name, other, int((got != again).sum()))


@pytest.mark.parametrize("dtype", GC.DTYPES)
@pytest.mark.parametrize("cid", [c["id"] for c in GC.GROUPED])
def test_grouped_kernel_one_op(cid, dtype):
    case = GC.CASES[cid]
    got, name = _run_one_op(case, dtype)
    _gate(got, _reference(case, dtype)[1], dtype, "%s %s (%s)" % (cid, dtype, name))
    _ordered_gate(case, dtype, got, "%s %s (%s)" % (cid, dtype, name))


def test_ordered_gate_covers_every_linear_and_leaky_case():
    """exactly the mish and logistic cases stay on the toleranced gates alone"""
    left_out = sorted(c["id"] for c in GC.DWISE + GC.GROUPED if c.get("act", "leaky") not in GO.EXACT_ACTS)
    assert left_out == sorted(GC.NOT_ORDERED) == ["dw_logistic", "dw_mish", "dw_res_mish", "gr_4x4_wide_res", "gr_4x8_wide_res"]


# ---------------------------------------------------------------------------------------------- grouped.cfg through Darknet

DWISE_BLOCKS = {2: "k3s1", 7: "k3s2", 9: "kn", 22: "k3s1", 24: "k3s1", 26: "k3s1"}
GROUPED_BLOCKS = {11: "oc1", 14: "oc8", 18: "oc8", 20: "oc8"}
HEAD = 28
_cache = {}


def _params():
    if "params" not in _cache:
        net = yolov3.Darknet(CFG)
        calib = [[0.0, 1.0]] * sum(1 for b in net.blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
        _cache["params"] = W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-2.0, calib=calib)
    return _cache["params"]


def _frames():
    return synth_frames(53, 2, 64, 96)


def _net(dtype, **kw):
    return yolov3.Darknet(CFG, device="cuda", dtype=dtype, **kw).set_params(_params()).eval()


def _kernels(net, dtype):
    kernel_of = {}
    for r in net.plan_report():
        kernel_of.setdefault(r["block"], []).append(r["kernel"])
    print("grouped.cfg %s: %s" % (dtype, {b: ",".join(k) for b, k in sorted(kernel_of.items())}))
    for b, form in DWISE_BLOCKS.items():
        assert kernel_of[b] == ["conv_dwise_%s_%s" % (TAG[dtype], form)], (b, kernel_of[b])
    for b, form in GROUPED_BLOCKS.items():
        assert kernel_of[b] == ["conv_grouped_%s_%s" % (TAG[dtype], form)], (b, kernel_of[b])
    other = [k for b, ks in kernel_of.items() if b not in DWISE_BLOCKS and b not in GROUPED_BLOCKS for k in ks]
    assert not any("dwise" in k or "grouped" in k for k in other), other
    assert 5 not in kernel_of                                   # [dropout] runs nothing
    return kernel_of


@pytest.mark.parametrize("dtype", GC.DTYPES)
def test_grouped_cfg_every_block_teacher_forced(dtype):
    frames = _frames()
    net = _net(dtype, keep_all=True, fuse=True)
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    kernel_of = _kernels(net, dtype)
    assert kernel_of[HEAD][0].startswith("conv_") and "head_decode" not in kernel_of[HEAD][0]     # the logits are in memory
    blocks, params = net.blocks, net._params
    slot_of = {c["block_idx"]: s for s, c in enumerate(net._convs)}
    emulate = GC.EMULATE[dtype]
    acc = "f64" if dtype == "float32" else "f32"
    x_net = torch.from_numpy(orc.frames_to_input(list(frames)))
    if dtype != "float32":
        # the MFMA stem stores byte / 255 in the storage type before it multiplies (tests/test_gpu_footprint.py: x_of)
        assert kernel_of[0] == ["conv_stem_mfma_u8_%s" % TAG[dtype]], kernel_of[0]
        x_net = MODES[dtype]["rnd"](x_net)
    fused = {i - 1: i for i, b in enumerate(blocks) if b["type"] == "shortcut"}      # (every shortcut of this cfg is fused)

    def hip(i):
        return x_net if i < 0 else net.block_output(i).cpu()

    checked = 0
    for i, blk in enumerate(blocks):
        kind = blk["type"]
        what = "%s grouped.cfg block %d (%s, %s)" % (dtype, i, kind, ",".join(kernel_of.get(i, ["-"])))
        if kind == "convolutional":
            k = blk["size"]
            y = GR.grouped_conv_block(hip(i - 1), params[slot_of[i]], blk["stride"], (k - 1) // 2 if "pad" in blk else 0,
                                      blk["activation"], int(blk.get("groups", 1)), round_weights=emulate, accumulate=acc)
            at = i
            if i in fused:
                at = fused[i]
                y = y + hip(at + blocks[at]["from"])              # added in float32 in the conv's epilogue, one rounding
            if dtype == "float32" or i == HEAD:
                np.testing.assert_allclose(hip(at).numpy(), y.numpy(), err_msg=what, **F32_BLOCK_TOL)
            else:
                _close_bf16(hip(at), MODES[dtype]["rnd"](y), what, None, dtype)
        elif kind == "route":
            assert torch.equal(hip(i), torch.cat([hip(j) for j in blk["layers"]], dim=1)), what
        elif kind == "dropout":
            assert torch.equal(hip(i), hip(i - 1)), what
        elif kind == "shortcut":
            assert i - 1 in fused, what
            continue
        else:
            assert kind == "yolo", what
            box, prob, idx = orc.yolo_decode(hip(HEAD), [blk["anchors"][m] for m in blk["mask"]])
            box[:, :, 2] /= net.net_info["width"]
            box[:, :, 3] /= net.net_info["height"]
            torch.testing.assert_close(out["bbox_xywh"].cpu(), box, rtol=2e-4, atol=2e-5, msg=lambda m: what + " boxes: " + m)
            torch.testing.assert_close(out["class_prob"].cpu(), prob, rtol=5e-4, atol=2e-5, msg=lambda m: what + " scores: " + m)
            assert torch.equal(out["class_idx"].cpu(), idx), what
        checked += 1
    assert checked == len(blocks) - 3 == 27

    # the arena (tensors reuse one another's memory) against keep_all, and one plan twice
    lean = _net(dtype)
    a = lean.forward_frames(frames)
    _kernels(lean, dtype)
    b = lean.forward_frames(frames)
    torch.cuda.synchronize()
    assert len(lean._plans) == 1
    for key in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(a[key], out[key]), (dtype, key, "arena against keep_all")
        assert torch.equal(a[key], b[key]), (dtype, key, "second run of the plan")
    # ... and under grouped_generic the whole network gives the same bits
    with _hip.grouped_generic():
        gen = _net(dtype)
        g = gen.forward_frames(frames)
        torch.cuda.synchronize()
        names = [r["kernel"] for r in gen.plan_report()]
    assert not any("dwise" in n for n in names) and sum("conv_grouped_" in n for n in names) == 10
    for key in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(a[key], g[key]), (dtype, key, "grouped_generic")


def test_grouped_cfg_through_the_entry_points(tmp_path):
    """``inference``, ``detect_in_frames`` and the command line on a cfg with ``groups=``, from a ``.weights`` file: the three
    agree detection for detection, and ``forward`` on a float tensor runs the same grouped kernels"""
    import json

    from PIL import Image

    from yolov3.__main__ import main
    weights = str(tmp_path / "grouped.weights")
    W.write_darknet_weights(weights, _params())
    net = yolov3.Darknet(CFG, device="cuda", dtype="bf16").load_weights(weights).eval()
    frames = list(_frames())
    first = yolov3.inference(net, frames, prob_thresh=0.05, nms_iou_thresh=0.3)
    assert len(first) == 2 and sum(len(r[1]) for r in first) > 0
    streamed = list(yolov3.detect_in_frames(net, frames, batch_size=2, prob_thresh=0.05, nms_iou_thresh=0.3))
    assert len(streamed) == 2
    for a, b in zip(first, streamed):
        for u, v in zip(a, b):
            assert np.array_equal(np.asarray(u), np.asarray(v))
    out = net.forward(torch.from_numpy(orc.frames_to_input(frames)))
    torch.cuda.synchronize()
    _kernels(net, "bf16")
    assert bool(torch.isfinite(out["class_prob"]).all())
    folder = tmp_path / "images"
    folder.mkdir()
    for i, im in enumerate(frames):
        Image.fromarray(np.ascontiguousarray(im[:, :, ::-1])).save(str(folder / ("%d.png" % i)))
    dump = tmp_path / "det.json"
    assert main(["-c", CFG, "-w", weights, "-I", str(folder), "-p", "0.05", "--dtype", "bf16", "--batch-size", "2", "--json", str(dump)]) == 0
    with open(str(dump)) as fh:
        coco = json.load(fh)
    ids = {im["file_name"]: im["id"] for im in coco["images"]}
    assert sorted(ids) == ["0.png", "1.png"]
    for i, (tlbr, prob, cls) in enumerate(first):
        got = sorted((a["category_id"], a["score"], tuple(a["bbox"])) for a in coco["annotations"] if a["image_id"] == ids["%d.png" % i])
        want = sorted((int(c), float(p), (int(b[0]), int(b[1]), int(b[2] - b[0]), int(b[3] - b[1])))
                      for b, p, c in zip(np.asarray(tlbr).tolist(), np.asarray(prob).tolist(), np.asarray(cls).tolist()))
        assert got == want, i


# ---------------------------------------------------------------------------------------------- footprint and census

# one case per compiled instance; every operand a channel slice of a wider stride between NaN / pattern canaries
FOOTPRINT = {"dwise_k3s1": "dw_wide_13x10_s1", "dwise_k3s2": "dw_wide_13x10_s2", "dwise_kn": "dw_k5_13x10_res",
             "grouped_oc8": "gr_4x8_wide_res", "grouped_oc1": "gr_4x4_wide_res"}


def census_key(instance, dtype):
    return "grouped_%s-%s" % (instance, dtype)


def _footprint_layout(case, dtype, base, path):
    """(ops, layout) of the case with every activation operand strided (tests/footprint_util.py's layout and fills)"""
    es = fu.ES[dtype]
    unit = 16 // es if dtype != "float32" else 8        # (the depthwise kernel's grain is 8 channels in every dtype)
    B, cin, cout, k = case.get("B", 3), case["cin"], case["cout"], case["k"]
    ho, wo = GC.out_hw(case)
    P, Po = B * case["h"] * case["w"], B * ho * wo
    used = set()

    def act(name, side, pixels, c, v):
        c0, ld = fu.strided_ld(c, unit, v, used)
        used.add(ld)
        return fu.Operand(name, side, dtype, pixels, ld, [(c0, c)])

    host, cp, k_ld = GC.device_weights(case, path, np.zeros((cout, cin // case["groups"], k, k), dtype=np.float32))
    operands = [act("input", "in", P, cin, 0), act("output", "out", Po, cout, 1)]
    if case.get("res"):
        operands.append(act("residual", "in", Po, cout, 2))
    operands += [fu.flat("weight", "in", dtype, host.size), fu.flat("scale", "in", "float32", cp), fu.flat("bias", "in", "float32", cp),
                 fu.flat("zero page", "in", dtype, 4096 // es)]
    lay = fu.Layout(operands)
    ops = (_hip.Y3Op * 1)()
    op = ops[0]
    op.kind, op.dtype, op.batch, op.block_idx = _hip.OP_CONV, DT_CODE[dtype], B, 1
    op.flags = ACT_FLAG[case.get("act", "leaky")] | (_hip.F_RESIDUAL if case.get("res") else 0)
    op.in_h, op.in_w, op.in_c, op.in_ld = case["h"], case["w"], cin, lay["input"].ld
    op.out_h, op.out_w, op.out_c, op.out_ld = ho, wo, cout, lay["output"].ld
    op.ksize, op.stride, op.pad, op.groups = k, case["s"], case["pad"], case["groups"]
    op.cout_pad, op.k_ld = cp, k_ld
    op.d_in, op.d_out = lay["input"].ptr(base), lay["output"].ptr(base)
    if case.get("res"):
        op.d_res, op.res_ld = lay["residual"].ptr(base), lay["residual"].ld
    op.d_weight, op.d_scale, op.d_bias = lay["weight"].ptr(base), lay["scale"].ptr(base), lay["bias"].ptr(base)
    return ops, lay


@pytest.mark.parametrize("dtype", GC.DTYPES)
@pytest.mark.parametrize("instance", sorted(FOOTPRINT))
def test_footprint_and_census(instance, dtype):
    lib = _hip.lib()
    case = GC.CASES[FOOTPRINT[instance]]
    path = GC.PATH_DWISE if instance.startswith("dwise") else GC.PATH_GROUPED
    tdt = GC.TORCH_DT[dtype]
    data, want = _reference(case, dtype)
    dev = torch.device("cuda:0")
    _, lay0 = _footprint_layout(case, dtype, 1 << 44, path)
    raw = torch.empty(lay0.total + fu.ALIGN, dtype=torch.uint8, device=dev)
    shift = -raw.data_ptr() % fu.ALIGN
    alloc = raw[shift:shift + lay0.total]
    base = alloc.data_ptr()
    ops, lay = _footprint_layout(case, dtype, base, path)
    assert lib.y3_conv_path(ctypes.byref(ops[0])) == path
    host, cp, _ = GC.device_weights(case, path, data["p"]["weight"])
    sc, bi = torch.zeros(cp), torch.zeros(cp)
    sc[:case["cout"]], bi[:case["cout"]] = torch.from_numpy(data["scale"]), torch.from_numpy(data["bias"])
    B = case.get("B", 3)
    feed = {"input": [_nhwc(data["x"], tdt).reshape(-1, case["cin"])], "weight": [torch.from_numpy(host).to(tdt).reshape(1, -1)],
            "scale": [sc.reshape(1, -1)], "bias": [bi.reshape(1, -1)], "zero page": [torch.zeros(lay["zero page"].slices[0][1], dtype=tdt)]}
    if case.get("res"):
        feed["residual"] = [_nhwc(data["res"], tdt).reshape(-1, case["cout"])]
    fu.fill(alloc, lay, feed, poisoned=True)
    torch.cuda.synchronize()
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create(ops, 1, lay["zero page"].ptr(base), ctypes.byref(handle)))
    try:
        name = lib.y3_plan_op_kernel(handle, 0).decode()
        assert name == "conv_%s" % instance.replace("_", "_%s_" % TAG[dtype], 1), name
        assert _hip.plan_op_dims(handle, 0)[1] % 64 == 0
        before = alloc.clone()
        del census.LAUNCHED[:]
        census.logged(lambda: _hip.check(lib.y3_plan_run(handle, None, None)))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    msg = fu.footprint_violations(before, alloc, lay)
    assert msg is None, "%s %s: %s" % (instance, dtype, msg)
    o = lay["output"]
    got = fu.read_slice(alloc, o, 0, tdt).float().cpu()
    assert not bool(torch.isnan(got).any()), "%s %s: the NaN of the output slice survived (or a NaN operand was read)" % (instance, dtype)
    ho, wo = GC.out_hw(case)
    _gate(got.reshape(B, ho, wo, -1).permute(0, 3, 1, 2).contiguous(), want, dtype, "%s %s" % (instance, dtype))
    # the launch log against the census of the grouped kernels' own library (tests/golden/kernel_instances_grouped.json)
    census.assert_census(census_key(instance, dtype), library="grouped")
