"""One-op cases of the grouped conv kernels (csrc/conv_grouped.hip), shared by tests/test_grouped_host.py (which proves on the
CPU that the gates fit the chosen inputs) and tests/test_gpu_grouped.py (which runs them through ``y3_op_run``).

A case is a dict: ``cin, cout, groups, k, s, pad, h, w`` and optionally ``B`` (3), ``act`` ("leaky"), ``res`` (False) and
``wide`` (False: dense tensors; True: every activation operand is a channel slice at a non-zero offset of a wider pixel
stride, as a member of a route's concat buffer is).  Inputs, parameters and the shortcut operand are seeded by the case's id and
hold storage-exact values of the dtype, so the product and the restatement start from the same numbers.

The device layouts are written out here, independently of ``yolov3.darknet.grouped_weight_layout``:
  grouped   [cout_pad][k_ld], row = output channel, column (ky * k + kx) * (cin / groups) + c
  depthwise [k * k][k_ld], row = tap, column = channel
"""
import numpy as np
import torch

import grouped_restate as GR
from oracle import darknet_oracle as orc

TORCH_DT = {"float32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
EMULATE = {"float32": None, "bf16": "bf16", "fp16": "f16"}
DTYPES = ("float32", "bf16", "fp16")
PATH_GROUPED, PATH_DWISE = 4, 5


def _dw(cid, c, h, w, k=3, s=1, pad=1, **kw):
    return dict(id=cid, cin=c, cout=c, groups=c, k=k, s=s, pad=pad, h=h, w=w, **kw)


def _gr(cid, cin, cout, groups, h, w, k=3, s=1, pad=1, **kw):
    return dict(id=cid, cin=cin, cout=cout, groups=groups, k=k, s=s, pad=pad, h=h, w=w, **kw)


MAPS = ((1, 1), (1, 5), (5, 1), (7, 7), (13, 10))

# depthwise kernel: chunk counts that do not fill a wave and that straddle one (C = 8, 24, 40, 136: 1, 3, 5, 17 chunks), every
# pixel-run tail (widths 1, 5, 7, 10 and the output widths stride 2 makes of them), stride 1 and 2 on odd and even maps, 3x3 with
# and without padding, 5x5, slices of wider strides, every activation, the shortcut operand
DWISE = (
    [_dw("dw_c%d" % c, c, 7, 7) for c in (8, 24, 40, 136)] +
    [_dw("dw_%dx%d_s%d" % (h, w, s), 24, h, w, s=s) for h, w in MAPS for s in (1, 2)] +
    [_dw("dw_pad0_7x7_s1", 24, 7, 7, pad=0), _dw("dw_pad0_7x7_s2", 24, 7, 7, s=2, pad=0),
     _dw("dw_pad0_13x10_s1", 40, 13, 10, pad=0), _dw("dw_pad0_13x10_s2", 40, 13, 10, s=2, pad=0),
     _dw("dw_k5_7x7", 24, 7, 7, k=5, pad=2), _dw("dw_k5_13x10_s2", 40, 13, 10, k=5, s=2, pad=2), _dw("dw_k5_1x5", 8, 1, 5, k=5, pad=2),
     _dw("dw_k5_13x10_res", 24, 13, 10, k=5, pad=2, res=True),
     _dw("dw_wide_13x10_s1", 40, 13, 10, wide=True, res=True), _dw("dw_wide_13x10_s2", 40, 13, 10, s=2, wide=True, res=True),
     _dw("dw_wide_c136", 136, 5, 5, wide=True),
     _dw("dw_linear", 24, 7, 7, act="linear"), _dw("dw_mish", 24, 7, 7, act="mish"), _dw("dw_logistic", 24, 7, 7, act="logistic"),
     _dw("dw_res_13x10_s2", 24, 13, 10, s=2, res=True), _dw("dw_res_mish", 40, 7, 7, act="mish", res=True)])

# grouped kernel: the group shapes of tests/golden/cfg/grouped.cfg (4 groups of 8 -> 8, 3 groups of 8 -> 16, a 1x1 with 2 groups
# of 20 -> 24: eight output channels per thread, with 16-byte and with scalar loads), 4 channels per group and a depthwise conv
# on 20 channels (one output element per thread); TINY_MAPS below adds maps of one pixel and of one pixel across
GROUPED = [
    _gr("gr_4x8", 32, 32, 4, 13, 10), _gr("gr_4x8_s2_res", 32, 32, 4, 13, 10, s=2, res=True),
    _gr("gr_4x8_wide_res", 32, 32, 4, 7, 7, wide=True, res=True, act="mish"),
    _gr("gr_3x8_16", 24, 48, 3, 13, 10), _gr("gr_2x20_24_1x1", 40, 48, 2, 13, 10, k=1, pad=0),
    _gr("gr_2x20_24_wide", 40, 48, 2, 7, 7, k=1, pad=0, wide=True, res=True),
    _gr("gr_4x4", 16, 16, 4, 13, 10), _gr("gr_4x4_wide_res", 16, 16, 4, 7, 7, s=2, wide=True, res=True, act="logistic"),
    _dw("gr_dw_c20", 20, 13, 10), _dw("gr_dw_c20_k5_res", 20, 7, 7, k=5, pad=2, res=True, act="linear"),
    # depthwise on 8-channel strides but at a channel offset of 4: addresses off the 16-byte grain, so not the depthwise kernel's
    _dw("gr_dw_c24_off4", 24, 7, 7, wide=True, off=4, res=True), _gr("gr_4x8_off4", 32, 32, 4, 7, 7, wide=True, off=4, res=True)]
# ... and both forms on maps of one pixel and of one pixel across (stride 2 makes 1 x 3 and 3 x 1 of the latter: every tap row or
# column but one lies outside), and 5x5 on one pixel, where 24 of the 25 taps lie outside
TINY_MAPS = ((1, 1), (1, 5), (5, 1))
GROUPED += (
    [_gr("gr_%s_%dx%d_s%d" % (tag, h, w, s), c, c, 4, h, w, s=s)
     for tag, c in (("4x8", 32), ("4x4", 16)) for h, w in TINY_MAPS for s in (1, 2) if not (s == 2 and (h, w) == (1, 1))] +
    [_gr("gr_4x8_k5_1x1", 32, 32, 4, 1, 1, k=5, pad=2), _gr("gr_4x4_k5_1x1", 16, 16, 4, 1, 1, k=5, pad=2)])

CASES = {c["id"]: c for c in DWISE + GROUPED}
assert len(CASES) == len(DWISE) + len(GROUPED)
# mish and logistic run __expf and v_rcp_f32: these cases stay on the toleranced gates alone; every other case is also held bit
# for bit to tests/grouped_ordered.py
NOT_ORDERED = ("dw_mish", "dw_logistic", "dw_res_mish", "gr_4x8_wide_res", "gr_4x4_wide_res")


def out_hw(case):
    return ((case["h"] + 2 * case["pad"] - case["k"]) // case["s"] + 1, (case["w"] + 2 * case["pad"] - case["k"]) // case["s"] + 1)


def is_dwise(case):
    """on the depthwise kernel's grain: dense and wide layouts here keep every stride a multiple of 8; an ``off`` case puts
    its operands 8 bytes past the 16-byte grain (``strides``), which is not the depthwise kernel's"""
    return case["groups"] == case["cin"] == case["cout"] and case["cin"] % 8 == 0 and not case.get("off")


def strides(case, c, dtype="bf16"):
    """(channel offset, pixel stride) of a ``c``-channel operand of the case.  ``off`` cases: 8 bytes past the 16-byte grain"""
    ld = (c + 7) // 8 * 8
    off = (2 if dtype == "float32" else 4) if case.get("off") else 0
    return (8 + off, ld + 24) if case.get("wide") else (0, ld)


def make(case, dtype):
    """Seeded data of a case in ``dtype``: dict(x (B, cin, h, w) float32, res (B, cout, ho, wo) float32 or None, p: the
    parameter dict of the block (storage-exact weights), scale, bias: the folded batch norm as ``Darknet._fold_bn`` folds it)."""
    tdt = TORCH_DT[dtype]
    gen = torch.Generator().manual_seed(sum(map(ord, case["id"])) * 13 + 5)
    B, cin, cout, g, k = case.get("B", 3), case["cin"], case["cout"], case["groups"], case["k"]
    ho, wo = out_hw(case)
    x = ((torch.rand((B, cin, case["h"], case["w"]), generator=gen) - 0.5) * 2.0).to(tdt).float()
    res = ((torch.rand((B, cout, ho, wo), generator=gen) - 0.5) * 2.0).to(tdt).float() if case.get("res") else None
    fan = (cin // g) * k * k
    wt = ((torch.rand((cout, cin // g, k, k), generator=gen) - 0.5) * (12.0 / fan) ** 0.5).to(tdt).float()
    p = {"weight": wt.numpy(),
         "bn_gamma": (torch.rand(cout, generator=gen) + 0.5).numpy(), "bn_beta": (torch.rand(cout, generator=gen) - 0.5).numpy(),
         "bn_mean": ((torch.rand(cout, generator=gen) - 0.5) * 0.2).numpy(), "bn_var": (torch.rand(cout, generator=gen) + 0.5).numpy()}
    scale = (p["bn_gamma"] / np.sqrt(p["bn_var"] + orc.BN_EPS)).astype(np.float32)
    bias = (p["bn_beta"] - p["bn_mean"] * scale).astype(np.float32)
    return dict(x=x, res=res, p=p, scale=scale, bias=bias)


def reference(case, dtype, data, accumulate=None):
    """The restatement's result from the case's data, UNROUNDED float32 (B, cout, ho, wo): float32 storage accumulates in float64
    (the gate is then F32_BLOCK_TOL), the 16-bit modes in float32 with weights as the mode rounds them; the shortcut operand is
    added to the activated value."""
    acc = accumulate or ("f64" if dtype == "float32" else "f32")
    y = GR.grouped_conv_block(data["x"], data["p"], case["s"], case["pad"], case.get("act", "leaky"), case["groups"],
                              round_weights=EMULATE[dtype], accumulate=acc)
    return y + data["res"] if data["res"] is not None else y


def device_weights(case, path, wt):
    """(host float32 array, cout_pad, k_ld) of the case's kernel ``wt`` (cout, cin / groups, k, k) in the layout of ``path``"""
    cout, cg, k = wt.shape[0], wt.shape[1], wt.shape[2]
    cp = (cout + 7) // 8 * 8
    if path == PATH_DWISE:
        host = np.zeros((k * k, cp), dtype=np.float32)
        for ky in range(k):
            for kx in range(k):
                host[ky * k + kx, :cout] = wt[:, 0, ky, kx]
        return host, cp, cp
    k_ld = (k * k * cg + 7) // 8 * 8
    host = np.zeros((cp, k_ld), dtype=np.float32)
    for ky in range(k):
        for kx in range(k):
            for c in range(cg):
                host[:cout, (ky * k + kx) * cg + c] = wt[:, c, ky, kx]
    return host, cp, k_ld
