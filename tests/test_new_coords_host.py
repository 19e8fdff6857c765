"""Scaled-YOLOv4 (yolov4-csp) without a GPU: the cfg, the plan, the C ABI's logistic / new_coords bits, the kernel choice on
fake addresses, and the restatement of tests/new_coords_restate.py pinned with hand-computed answers."""
import ctypes
import json
import os

import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.plan import build_plan

import new_coords_restate as NR
from golden_util import GOLDEN, MODEL_DIR

CSP = os.path.join(MODEL_DIR, "yolov4-csp.cfg")
MINI = os.path.join(GOLDEN, "cfg", "mini.cfg")
V4_FIXTURE = os.path.join(GOLDEN, "yolov4_plans.json")
HEADS = (143, 158, 173)


def _blocks(path=CSP):
    blocks, net_info = parse_config(path)
    for i, blk in enumerate(blocks):
        if blk["type"] == "route":
            blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
    return blocks, net_info


def test_csp_cfg_blocks_and_weight_stream():
    """175 blocks, 512 x 512, mish everywhere but the three logistic 255-channel heads, and the weight stream the layer table
    implies: a 20-byte header and, per conv, 4 x Cout BN floats (or Cout biases) + Cout Cin k^2."""
    blocks, net_info = parse_config(CSP)
    assert len(blocks) == 175
    assert net_info["width"] == net_info["height"] == 512
    convs = [(i, b) for i, b in enumerate(blocks) if b["type"] == "convolutional"]
    assert len(convs) == 115
    assert [i for i, b in convs if b["activation"] == "logistic"] == list(HEADS)
    assert all(b["activation"] == "mish" for i, b in convs if i not in HEADS)
    assert all(blocks[i]["filters"] == 255 and "batch_normalize" not in blocks[i] for i in HEADS)
    yolos = [b for b in blocks if b["type"] == "yolo"]
    assert [i for i, b in enumerate(blocks) if b["type"] == "yolo"] == [h + 1 for h in HEADS]
    assert all(int(b["new_coords"]) == 1 and float(b["scale_x_y"]) == 2.0 for b in yolos)
    assert 20 + 4 * W.stream_length(blocks, net_info) == 211944840
    # the three routes whose indices tie the neck to the backbone and to the SPP block
    assert [blocks[i]["layers"] for i in (116, 130, 147, 162)] == [[79], [48], [-1, -20], [-1, -49]]


def test_plan_carries_logistic_heads_and_new_coords():
    blocks, net_info = _blocks()
    d = build_plan(blocks, net_info, 2, 512, 512, 2, reuse=True, fuse=True)
    convs = [o for o in d["ops"] if o["kind"] == "conv"]
    assert sorted(o["block"] for o in convs if o.get("logistic")) == list(HEADS)
    assert all(o.get("logistic") is None for o in convs if o["block"] not in HEADS)
    assert all(o.get("mish") for o in convs if o["block"] not in HEADS)
    yolos = [o for o in d["ops"] if o["kind"] == "yolo"]
    assert [o["block"] for o in yolos] == [h + 1 for h in HEADS]
    assert all(o["new_coords"] is True and o["scale_x_y"] == 2.0 for o in yolos)
    assert d["rows_total"] == 3 * (64 * 64 + 32 * 32 + 16 * 16)


def _mini_head(tmp_path, act):
    """mini.cfg with new_coords=1 on its first [yolo] block and the conv in front of it given activation ``act``"""
    text = open(MINI).read()
    k = text.index("[yolo]")
    head = text.rindex("activation=", 0, k)
    end = text.index("\n", head)
    text = text[:head] + "activation=" + act + text[end:k] + "[yolo]\nnew_coords=1" + text[k + len("[yolo]"):]
    p = tmp_path / "mini_nc.cfg"
    p.write_text(text)
    blocks, _ = parse_config(str(p))
    yi = next(i for i, b in enumerate(blocks) if b["type"] == "yolo")
    return str(p), yi


@pytest.mark.parametrize("act", ["linear", "leaky", "mish"])
def test_new_coords_behind_a_non_logistic_head_is_refused(tmp_path, act):
    cfg, yi = _mini_head(tmp_path, act)
    with pytest.raises(ValueError, match=r"yolo block %d: new_coords" % yi):
        yolov3.Darknet(cfg)


def test_new_coords_behind_a_logistic_head_is_accepted(tmp_path):
    cfg, yi = _mini_head(tmp_path, "logistic")
    net = yolov3.Darknet(cfg)
    assert net.blocks[yi]["type"] == "yolo"


def test_library_reports_logistic_and_new_coords():
    lib = _hip.lib()
    want = _hip.CAP_MISH | _hip.CAP_SCALE_X_Y | _hip.CAP_LOGISTIC | _hip.CAP_NEW_COORDS
    assert lib.y3_capabilities() & want == want
    assert (_hip.F_LOGISTIC, _hip.F_NEW_COORDS, _hip.CAP_LOGISTIC, _hip.CAP_NEW_COORDS) == (256, 512, 4, 8)
    assert ctypes.sizeof(_hip.Y3Op) == 248 and _hip.ABI_VERSION == 6


def test_stale_library_is_refused(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: _hip.CAP_MISH | _hip.CAP_SCALE_X_Y)
    with pytest.raises(_hip.HipLibraryError, match="logistic, new_coords"):
        _hip.require_capabilities(_hip.CAP_MISH | _hip.CAP_LOGISTIC | _hip.CAP_NEW_COORDS, "yolov4-csp.cfg")
    _hip.require_capabilities(_hip.CAP_MISH | _hip.CAP_SCALE_X_Y, "yolov4.cfg")


def test_yolov4_plans_unchanged_op_for_op():
    """YOLOv4 and YOLOv4-tiny compile to exactly the plans of the compiler before logistic and new_coords
    (tests/golden/yolov4_plans.json, tools/make_yolov4_plan_fixture.py)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "tools"))
    try:
        import make_yolov4_plan_fixture as mk
    finally:
        sys.path.pop(0)
    with open(V4_FIXTURE) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(mk.snapshot(build_plan), sort_keys=True))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def _csp_ops(dtype, batch, opt):
    import kernel_choice_util as kc
    ops, _, fake = kc.build_ops("yolov4-csp", 512, dtype, batch, "u8", opt)
    blocks, _ = _blocks()
    convs = {i: b["activation"] for i, b in enumerate(blocks) if b["type"] == "convolutional"}
    assert {op.block_idx for op in ops if op.flags & _hip.F_MISH} == {i for i, act in convs.items() if act == "mish"}
    assert {op.block_idx for op in ops if op.flags & _hip.F_LOGISTIC} == {i for i, act in convs.items() if act == "logistic"}
    yolos = [op for op in ops if op.kind == _hip.OP_YOLO]
    assert [op.block_idx for op in yolos] == [h + 1 for h in HEADS]
    assert all(op.flags & _hip.F_NEW_COORDS and op.scale_x_y == float(blocks[op.block_idx]["scale_x_y"]) for op in yolos)
    return ops, fake


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("batch", [1, 16])
def test_csp_heads_fuse_and_no_leaky_kernel_takes_a_logistic_op(dtype, batch):
    """Plan creation on fake addresses with every fusion switched on: no logistic conv lands in a fused LeakyReLU kernel (stem,
    residual block, bottleneck), and all three heads run on a fused head-decode kernel, the hot path."""
    lib = _hip.lib()
    opt = _hip.options(fuse_block=2, fuse_stem=1, fuse_head=1)
    ops, fake = _csp_ops(dtype, batch, opt)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
    finally:
        lib.y3_plan_destroy(handle)
    heads = [n for n in range(len(ops)) if ops[n].flags & _hip.F_LOGISTIC]
    assert [ops[n].block_idx for n in heads] == list(HEADS)
    for n in heads:
        assert "head_decode" in names[n], (n, ops[n].block_idx, names[n])
        assert not any(f in names[n] for f in ("stem_s2", "resblock", "block_fused")), names[n]
        assert ops[n + 1].kind == _hip.OP_YOLO and names[n + 1].startswith("(fused"), names[n + 1]


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
@pytest.mark.parametrize("other", ["leaky", "mish"])
def test_dispatch_refuses_logistic_with_another_activation(other):
    lib = _hip.lib()
    opt = _hip.options()
    ops, fake = _csp_ops("bf16", 1, opt)
    n = next(k for k in range(len(ops)) if ops[k].kind == _hip.OP_CONV and ops[k].flags & _hip.F_MISH and k > 0)
    ops[n].flags |= _hip.F_LOGISTIC
    if other == "leaky":
        ops[n].flags = (ops[n].flags & ~_hip.F_MISH) | _hip.F_LEAKY
    handle = ctypes.c_void_p()
    rc = lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle))
    assert rc != 0 and b"exclusive" in lib.y3_last_error()


def test_restated_logistic_known_answers():
    """The restatement's logistic is torch.sigmoid: pinned at the saturation points the kernels promise."""
    x = torch.tensor([0.0, 20.0, -20.0, 90.0, -90.0, float("inf"), float("-inf")])
    s = torch.sigmoid(x)
    assert s[0] == 0.5 and s[1] == 1.0 and s[3] == 1.0 and s[5] == 1.0 and s[6] == 0.0
    assert 0 < float(s[2]) < 2.1e-9 and float(s[4]) < 1e-38
    assert not torch.isnan(s).any()


def test_restated_new_coords_decode_known_answers():
    """One 2 x 2 head, one anchor (20 x 40 px), 3 classes, scale_x_y 2, worked by hand."""
    t = torch.zeros(1, 8, 2, 2)
    # cell (x=1, y=0): tx .5 ty .25 tw .5 th 1 obj .8, classes .5 .75 .75 (tie: the first of the two wins)
    t[0, :, 0, 1] = torch.tensor([0.5, 0.25, 0.5, 1.0, 0.8, 0.5, 0.75, 0.75])
    box, prob, idx = NR.new_coords_decode(t, [(20, 40)], 2.0)
    row = 1                                               # a * h * w + y * w + x
    # x: (0.5 * 2 - 0.5 + 1) / 2 = 0.75;  y: (0.25 * 2 - 0.5 + 0) / 2 = 0;  w: 0.25 * 4 * 20 = 20;  h: 1 * 4 * 40 = 160
    assert box[0, row].tolist() == [0.75, 0.0, 20.0, 160.0]
    assert float(prob[0, row]) == float(torch.tensor(0.75) * torch.tensor(0.8)) and int(idx[0, row]) == 1
    # an all-zero cell (x=0, y=1): centre (0 - 0.5 + cell) / 2, zero size, zero score, class 0
    assert box[0, 2].tolist() == [-0.25, 0.25, 0.0, 0.0] and float(prob[0, 2]) == 0.0 and int(idx[0, 2]) == 0
    # saturated class logits: 1.0f for both of the last two classes -> the first of them, whatever the logits were
    sat = torch.sigmoid(torch.tensor([3.0, 18.0, 25.0]))
    assert sat[1] == sat[2] == 1.0
    t[0, 5:, 1, 1] = sat
    t[0, 4, 1, 1] = 1.0
    _, prob, idx = NR.new_coords_decode(t, [(20, 40)], 2.0)
    assert int(idx[0, 3]) == 1 and float(prob[0, 3]) == 1.0
