"""YOLOv4 / YOLOv4-tiny on the host (no GPU): the two cfgs, their weight streams and plans (mish, grouped routes,
scale_x_y), what is refused, the library's capability bits, and the YOLOv3 plans pinned op for op."""
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

import plan_fixture
from golden_util import GOLDEN, MODEL_DIR

V4 = {"yolov4": os.path.join(MODEL_DIR, "yolov4.cfg"), "yolov4-tiny": os.path.join(MODEL_DIR, "yolov4-tiny.cfg")}
MINI = os.path.join(GOLDEN, "cfg", "mini.cfg")


def _blocks(model):
    blocks, net_info = parse_config(V4[model])
    for i, blk in enumerate(blocks):
        if blk["type"] == "route":
            blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
    return blocks, net_info


@pytest.mark.parametrize("model,n_blocks,nbytes,dim", [("yolov4", 162, 257717640, 608), ("yolov4-tiny", 38, 24251276, 416)])
def test_cfg_blocks_and_weight_stream_bytes(model, n_blocks, nbytes, dim):
    """The published .weights sizes: a 20-byte header and, per conv, 4 x Cout BN floats (or Cout biases) + Cout Cin k^2."""
    blocks, net_info = parse_config(V4[model])
    assert len(blocks) == n_blocks
    assert net_info["width"] == net_info["height"] == dim
    assert 20 + 4 * W.stream_length(blocks, net_info) == nbytes


def test_tiny_grouped_route_is_a_32_channel_alias():
    blocks, net_info = _blocks("yolov4-tiny")
    _, convs = W.conv_layout(blocks, net_info)
    assert [c["cin"] for c in convs if c["block_idx"] == 4] == [32]          # the conv after the first grouped route
    for dtype_bytes in (4, 2):
        d = build_plan(blocks, net_info, 2, 416, 416, dtype_bytes)
        assert d["shapes"][3] == (32, 104, 104)
        src, grp = d["tensor_of"][2], d["tensor_of"][3]
        assert (grp.buf, grp.off, grp.c, grp.ld) == (src.buf, src.off + 32, 32, src.ld)   # second half, same pixel stride
        assert not [op for op in d["ops"] if op["block"] == 3]                # no copy
        conv4 = next(op for op in d["ops"] if op["block"] == 4)
        assert conv4["inp"] is grp
        for b in (11, 19):                                                    # the other two CSP stages
            assert d["tensor_of"][b].off == d["tensor_of"][b - 1].off + d["tensor_of"][b].c


def test_grouped_route_off_the_channel_grid_is_copied(tmp_path):
    """A group that starts off the 8-channel slice grid cannot be an alias: the plan copies it."""
    cfg = tmp_path / "g.cfg"
    cfg.write_text("[net]\nwidth=32\nheight=32\nchannels=3\n\n"
                   "[convolutional]\nbatch_normalize=1\nfilters=24\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
                   "[route]\nlayers=-1\ngroups=2\ngroup_id=1\n\n"
                   "[convolutional]\nbatch_normalize=1\nfilters=16\nsize=1\nstride=1\npad=1\nactivation=mish\n\n"
                   "[convolutional]\nsize=1\nstride=1\npad=1\nfilters=255\nactivation=linear\n\n"
                   "[yolo]\nmask=0,1,2\nanchors=10,14, 23,27, 37,58\nclasses=80\nnum=3\n")
    net = yolov3.Darknet(str(cfg))
    assert [c["cin"] for c in net._convs] == [3, 12, 16]
    d = build_plan(net.blocks, net.net_info, 1, 32, 32, 2)
    copy = [op for op in d["ops"] if op["kind"] == "copy"]
    assert len(copy) == 1 and copy[0]["block"] == 1 and copy[0]["inp"].off == 12 and copy[0]["inp"].c == 12
    assert d["tensor_of"][1].off == 0 and d["tensor_of"][1].c == 12


def test_mish_and_scale_x_y_reach_the_plan():
    blocks, net_info = _blocks("yolov4")
    d = build_plan(blocks, net_info, 1, 608, 608, 2)
    convs = [op for op in d["ops"] if op["kind"] == "conv"]
    mish = [op["block"] for op in convs if op.get("mish")]
    assert len(mish) == 72 and max(mish) == 104                               # the whole CSPDarknet-53 backbone, nothing after
    assert not any(op["leaky"] for op in convs if op.get("mish"))
    assert [op.get("scale_x_y") for op in d["ops"] if op["kind"] == "yolo"] == [1.2, 1.1, 1.05]
    tiny = build_plan(*_blocks("yolov4-tiny"), 1, 416, 416, 2)
    assert [op.get("scale_x_y") for op in tiny["ops"] if op["kind"] == "yolo"] == [1.05, 1.05]
    assert not any(op.get("mish") for op in tiny["ops"])


def _mini_with(tmp_path, edit):
    text = open(MINI).read()
    new = edit(text)
    assert new != text
    p = tmp_path / "edited.cfg"
    p.write_text(new)
    return str(p)


def _first(text, section, extra):
    """add `extra` lines to the first [section] of a cfg text"""
    head = "[%s]\n" % section
    i = text.index(head) + len(head)
    return text[:i] + extra + text[i:]


@pytest.mark.parametrize("edit,msg", [
    (lambda t: t.replace("activation=leaky", "activation=swish", 1), "activation 'swish'"),
    (lambda t: _first(t, "convolutional", "groups=2\n"), "grouped convolution"),
    (lambda t: _first(t, "convolutional", "dilation=2\n"), "dilated convolution"),
    (lambda t: _first(t, "yolo", "new_coords=1\n"), "new_coords"),
    (lambda t: _first(t, "shortcut", "weights_type=per_feature\n"), "weights_type"),
    (lambda t: t[:t.index("[shortcut]")] + t[t.index("[shortcut]"):].replace("activation=linear", "activation=leaky", 1),
     "shortcut block"),
])
def test_refuses_what_it_cannot_compute(tmp_path, edit, msg):
    cfg = _mini_with(tmp_path, edit)
    with pytest.raises(ValueError, match=msg):
        yolov3.Darknet(cfg)
    blocks, net_info = parse_config(cfg)
    with pytest.raises(ValueError, match=msg):
        build_plan(blocks, net_info, 1, 64, 64, 4)


def test_refuses_groups_on_a_multi_layer_route(tmp_path):
    cfg = _mini_with(tmp_path, _multi_route)
    with pytest.raises(ValueError, match="single-layer routes"):
        yolov3.Darknet(cfg)


def _multi_route(text):
    lines = text.split("\n")
    out, seen = [], False
    for ln in lines:
        out.append(ln)
        if not seen and ln.replace(" ", "").startswith("layers=") and "," in ln:
            out += ["groups=2", "group_id=0"]
            seen = True
    assert seen, "mini.cfg has no multi-layer route"
    return "\n".join(out)


def test_yolov3_plans_unchanged_op_for_op():
    """The YOLOv3 cfgs and mini.cfg compile to exactly the plans of the compiler before mish, grouped routes and scale_x_y
    (tests/golden/yolov3_plans.json, tools/make_plan_fixture.py)."""
    with open(plan_fixture.FIXTURE) as fh:
        want = json.load(fh)
    got = json.loads(json.dumps(plan_fixture.snapshot(build_plan), sort_keys=True))
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key] == want[key], key


def test_library_reports_mish_and_scale_x_y():
    lib = _hip.lib()
    assert lib.y3_capabilities() & (_hip.CAP_MISH | _hip.CAP_SCALE_X_Y) == (_hip.CAP_MISH | _hip.CAP_SCALE_X_Y)
    assert _hip.capabilities() == lib.y3_capabilities()
    # the former `int32_t reserved` of y3_op: same offset, same size
    assert _hip.Y3Op.scale_x_y.offset == _hip.Y3Op.block_idx.offset + 4 and _hip.Y3Op.scale_x_y.size == 4
    assert ctypes.sizeof(_hip.Y3Op) == 248 and _hip.ABI_VERSION == 6


def test_stale_library_is_refused(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: 0)
    with pytest.raises(_hip.HipLibraryError, match="mish, scale_x_y"):
        _hip.require_capabilities(_hip.CAP_MISH | _hip.CAP_SCALE_X_Y, "yolov4.cfg")
    _hip.require_capabilities(0, "yolov3.cfg")


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
@pytest.mark.parametrize("model,dim", [("yolov4", 608), ("yolov4-tiny", 416)])
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
@pytest.mark.parametrize("batch", [1, 16])
def test_no_fused_kernel_takes_a_mish_op(model, dim, dtype, batch):
    """Plan creation on fake addresses (tests/kernel_choice_util.py): with every fusion switched on, no mish conv lands in a
    fused step (the fused stem, residual-block and bottleneck kernels hard-wire LeakyReLU), and every mish conv of the
    backbone gets a kernel of its own."""
    import kernel_choice_util as kc
    lib = _hip.lib()
    opt = _hip.options(fuse_block=2, fuse_stem=1, fuse_head=1)
    ops, _, fake = kc.build_ops(model, dim, dtype, batch, "u8", opt)
    blocks, _ = _blocks(model)
    mish_blocks = {i for i, b in enumerate(blocks) if b["type"] == "convolutional" and b["activation"] == "mish"}
    assert {op.block_idx for op in ops if op.flags & _hip.F_MISH} == mish_blocks
    assert not any(op.flags & _hip.F_LOGISTIC for op in ops)
    assert [op.scale_x_y for op in ops if op.kind == _hip.OP_YOLO] == [
        ctypes.c_float(float(b["scale_x_y"])).value for b in blocks if b["type"] == "yolo"]
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
    finally:
        lib.y3_plan_destroy(handle)
    fused = ("fused", "head_decode", "block_fused")
    for n in range(len(ops)):
        if ops[n].flags & _hip.F_MISH:
            assert not any(f in names[n] for f in fused), (n, ops[n].block_idx, names[n])
            assert n + 1 >= len(ops) or not names[n + 1].startswith("(fused"), (n, ops[n].block_idx, names[n], names[n + 1])
    if model == "yolov4":
        assert not any("resblock" in k for k in names)                          # every residual block of v4 is mish
    if model == "yolov4-tiny":
        assert names[0].startswith("conv_stem3x3_u8_"), names[0]                # 3x3 stride-2 layer on the uint8 frames


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
def test_dispatch_refuses_mish_and_leaky_together():
    import kernel_choice_util as kc
    lib = _hip.lib()
    opt = _hip.options()
    ops, _, fake = kc.build_ops("yolov4-tiny", 416, "bf16", 1, "u8", opt)
    n = next(k for k in range(len(ops)) if ops[k].kind == _hip.OP_CONV and ops[k].flags & _hip.F_LEAKY and k > 0)
    ops[n].flags |= _hip.F_MISH
    handle = ctypes.c_void_p()
    rc = lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle))
    assert rc != 0 and b"exclusive" in lib.y3_last_error()
