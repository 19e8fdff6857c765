"""``plan_ops.fill_ops`` on every shipped cfg without a GPU: the ops ``Darknet`` compiles, filled on fake addresses
(tests/kernel_choice_util.py), make a plan; the capability mask is what the cfg and the mode imply; the activation flags are the
cfg's; the head views of a multi-label fill are the YOLO ops' inputs."""
import ctypes

import pytest
import torch

from yolov3 import _hip
from yolov3.plan import build_plan
from yolov3.plan_ops import fill_ops, head_views, multi_label_options

import kernel_choice_util as kc

C = _hip
# cfg -> (the capabilities its blocks imply in every mode, has [maxpool] blocks, has heads that Darknet scores with a logistic per
# class -- [yolo] without new_coords --, admits multi_label)
CFGS = {
    "yolov3": (0, False, True, True),
    "yolov3-spp": (0, True, True, True),
    "yolov3-tiny": (0, True, True, True),
    "yolov4": (C.CAP_MISH | C.CAP_SCALE_X_Y, True, True, True),
    "yolov4-tiny": (C.CAP_SCALE_X_Y, True, True, True),
    "yolov4-csp": (C.CAP_MISH | C.CAP_SCALE_X_Y | C.CAP_LOGISTIC | C.CAP_NEW_COORDS, True, False, True),
    "yolov2": (C.CAP_REORG, True, False, False),
    "yolov2-tiny": (0, True, False, False),
}
MODES = {"reference": {}, "darknet": dict(pool="darknet", scores="darknet"),
         "multi_label": dict(pool="darknet", scores="darknet", multi_label=True)}
CASES = [(model, mode) for model in CFGS for mode in MODES if mode != "multi_label" or CFGS[model][3]]


def _fill(model, mode, dtype, batch):
    """(network, ops, capability mask, allocator, plan options) of one fill as Darknet._compile_on_device makes it"""
    net = kc.network(model, dtype, **MODES[mode])
    opt = _hip.options(**(multi_label_options(None, net.multi_label) or {}))
    desc = build_plan(net.blocks, net.net_info, batch, net.net_info["height"], net.net_info["width"], kc.DTYPES[dtype][1],
                      reuse=True, fuse=True, pool=net.pool, keep_heads=net.multi_label)
    fake = kc._Fake(net._convs, kc.DTYPES[dtype][1])
    ops, needs, _ = fill_ops(desc, net.net_info, net._convs, dtype, batch, "u8", net.scores, opt, fake)
    return net, ops, needs, fake, opt


def test_the_matrix_is_132_plans():
    assert len(CASES) * len(kc.DTYPE_NAMES) * 2 == 132


@pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
@pytest.mark.parametrize("model,mode", CASES)
def test_every_cfg_fills_and_plans(model, mode):
    lib = _hip.lib()
    base, pools, logistic_scores, _ = CFGS[model]
    want = base
    if mode != "reference":
        want |= (C.CAP_POOL_DARKNET if pools else 0) | (C.CAP_SCORES_DARKNET if logistic_scores else 0)
    if mode == "multi_label":
        want |= C.CAP_MULTI_LABEL
    for dtype in kc.DTYPE_NAMES:
        for batch in (1, 16):
            net, ops, needs, fake, opt = _fill(model, mode, dtype, batch)
            assert needs == want, (dtype, batch, needs, want)
            assert needs & ~lib.y3_capabilities() == 0
            acts = {i: b.get("activation") for i, b in enumerate(net.blocks) if b["type"] == "convolutional"}
            for flag, name in ((C.F_MISH, "mish"), (C.F_LOGISTIC, "logistic"), (C.F_LEAKY, "leaky")):
                assert {op.block_idx for op in ops if op.flags & flag} == {i for i, a in acts.items() if a == name}, name
            handle = ctypes.c_void_p()
            _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
            lib.y3_plan_destroy(handle)


@pytest.mark.parametrize("model", [m for m in CFGS if CFGS[m][3]])
def test_head_views_are_the_yolo_ops_inputs(model):
    net, ops, _, _, opt = _fill(model, "multi_label", "bf16", 2)
    assert opt.fuse_head == 0
    yolo = [op for op in ops if op.kind == C.OP_YOLO]
    heads = head_views(ops)
    assert len(heads) == len(yolo) == sum(b["type"] == "yolo" for b in net.blocks)
    for view, op in zip(heads, yolo):
        assert view.d_head == op.d_in and view.d_head
        assert (view.h, view.w, view.ld) == (op.in_h, op.in_w, op.in_ld)
        assert (view.n_anchor, view.n_attr, view.row_offset) == (op.n_anchor, op.n_attr, op.row_offset)
        assert view.new_coords == int(model == "yolov4-csp") == int(bool(op.flags & C.F_NEW_COORDS))
    assert len({view.d_head for view in heads}) == len(yolo)         # kept heads: no two share an arena slot
