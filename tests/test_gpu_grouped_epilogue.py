"""The epilogues of the grouped and depthwise conv kernels on planted pre-activations, bit for bit (-m gpu), in the manner of
tests/test_gpu_epilogue.py's ``test_direct_conv_epilogue``.

csrc/conv_grouped.hip ends in three epilogue code paths of its own: ``epilogue8`` with 16-byte stores (every ``conv_dwise_*``
instance, and ``conv_grouped_*_oc8`` on the 16-byte grain), ``epilogue8``'s per-element branch (``conv_grouped_*_oc8`` off that
grain) and the one-element tail on ``y3_bn_act1`` (``conv_grouped_*_oc1``).  tests/grouped_suites.py has one form per compiled
instance and one more for the per-element branch; tests/test_grouped_host.py holds that table to the library's census.

Each form is a one-op plan through ``y3_plan_create_ex`` / ``y3_plan_run`` with the kernel name asserted: zero weights and a finite
random input leave the accumulator at +0 (the depthwise kernel multiplies real taps by zero weights: a negative input gives a -0
product, and +0 + -0 is +0), scale is +1 (-1 on the ``NEG_SCALE_TAG`` entry), the bias is the planted list of
tests/epilogue_cases.py in 128 output channels.  Linear and leaky are demanded exactly, mish and logistic inside
``epilogue_cases.expect``'s interval of storage values; linear and leaky run again with a shortcut operand and the searched
shortcut cases (one rounding of a + r), and once with the non-finite pairs of ``test_shortcut_operand_non_finite``.
"""
import ctypes

import numpy as np
import pytest
import torch

from yolov3 import _hip

import epilogue_cases as E
import grouped_cases as GC
import grouped_suites as GS
from test_gpu_epilogue import ACT_FLAG, _gate, _operand

pytestmark = pytest.mark.gpu

DT_CODE = {"float32": _hip.Y3_F32, "bf16": _hip.Y3_BF16, "fp16": _hip.Y3_F16}
FORMS = sorted(GS.EPILOGUE_FORMS)


def _run_form(form, dtype, act, t, tags, r=None):
    """(stored output (B, C, H, W) float32 on the device, kernel name) of the form's one-op plan with pre-activations ``t`` (one
    per channel) and shortcut operand ``r`` per channel or None"""
    _hip.require_gpu()
    lib = _hip.lib()
    dev = torch.device("cuda:0")
    case = GS.epilogue_case(form)
    tdt = GC.TORCH_DT[dtype]
    B, h, w, cin, cout, k = case["B"], case["h"], case["w"], case["cin"], case["cout"], case["k"]
    ho, wo = GC.out_hw(case)
    (in_off, in_ld), (out_off, out_ld) = GC.strides(case, cin, dtype), GC.strides(case, cout, dtype)
    res_off, res_ld = (out_off + 8, out_ld + 16) if case.get("wide") else (out_off, out_ld)
    nan = float("nan")
    x = torch.full((B, h, w, in_ld), nan, dtype=tdt, device=dev)
    x[..., in_off:in_off + cin] = (torch.rand((B, h, w, cin), generator=torch.Generator().manual_seed(13)) - 0.5).to(tdt).to(dev)
    out = torch.full((B, ho, wo, out_ld), nan, dtype=tdt, device=dev)
    neg = np.asarray([g == E.NEG_SCALE_TAG for g in tags]) & (E.bits(t) == 0x80000000)
    scale = torch.from_numpy(np.where(neg, -1.0, 1.0).astype(np.float32)).to(dev)
    bias = torch.from_numpy(E.f32(t).copy()).to(dev)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    ops = (_hip.Y3Op * 1)()
    op = ops[0]
    op.kind, op.dtype, op.batch, op.block_idx = _hip.OP_CONV, DT_CODE[dtype], B, 1
    op.flags = ACT_FLAG[act] | (_hip.F_RESIDUAL if r is not None else 0)
    op.in_h, op.in_w, op.in_c, op.in_ld = h, w, cin, in_ld
    op.out_h, op.out_w, op.out_c, op.out_ld = ho, wo, cout, out_ld
    op.ksize, op.stride, op.pad, op.groups = k, case["s"], case["pad"], case["groups"]
    es = x.element_size()
    op.d_in, op.d_out = x.data_ptr() + in_off * es, out.data_ptr() + out_off * es
    if r is not None:
        res = torch.full((B, ho, wo, res_ld), nan, dtype=tdt, device=dev)
        res[..., res_off:res_off + cout] = torch.from_numpy(E.f32(r).copy()).to(tdt).to(dev)
        op.d_res, op.res_ld = res.data_ptr() + res_off * es, res_ld
    grain = 8 if case.get("off") else 0
    assert op.d_in % 16 == op.d_out % 16 == grain and (r is None or op.d_res % 16 == grain), form
    op.cout_pad, op.k_ld = 128, 1 << 20                        # (provisional: the path does not depend on them)
    path = lib.y3_conv_path(ctypes.byref(op))
    assert path == (GC.PATH_DWISE if GC.is_dwise(case) else GC.PATH_GROUPED), (form, path)
    host, op.cout_pad, op.k_ld = GC.device_weights(case, path, np.zeros((cout, cin // case["groups"], k, k), dtype=np.float32))
    assert op.cout_pad == cout == len(t)
    wgt = torch.zeros(host.shape, dtype=tdt, device=dev)
    op.d_weight, op.d_scale, op.d_bias = wgt.data_ptr(), scale.data_ptr(), bias.data_ptr()
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, 1, zero.data_ptr(), None, ctypes.byref(handle)))
    try:
        name = lib.y3_plan_op_kernel(handle, 0).decode()
        assert name == GS.kernel_name(case["instance"], dtype), (form, dtype, name)
        _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    o = out.float()
    written = torch.zeros(out_ld, dtype=torch.bool, device=dev)
    written[out_off:out_off + cout] = True
    assert bool(torch.isnan(o[..., ~written]).all()), "%s %s: wrote outside its channel slice" % (form, dtype)
    return o[..., written].permute(0, 3, 1, 2).contiguous(), name


@pytest.mark.parametrize("act", E.ACTS)
@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_grouped_conv_epilogue(form, dtype, act):
    t, idx = E.padded(act)
    tags = [E.cases(act)[i].tag for i in idx]
    assert E.NEG_SCALE_TAG in tags and len(t) == GS.EPILOGUE_C
    if dtype == "float32":
        # the premise on the GPU: the op as a linear, shortcut-free conv gives its bias at every pixel, bit for bit
        pre, name = _run_form(form, dtype, "linear", t, tags)
        _gate(pre, t, t, np.isnan(t), "%s %s pre-activation" % (name, form), tags, t)
    got, name = _run_form(form, dtype, act, t, tags)
    _gate(got, *E.expect(act, dtype, t), "%s %s %s" % (name, form, act), tags, t)
    if act in ("linear", "leaky"):
        # the shortcut operand is added in float32 before the one store: one rounding of the sum
        r = _operand(GS.EPILOGUE_C, 13, dtype)
        ts, stags = E.shortcut_cases(act, dtype, r, 13)
        got, name = _run_form(form, dtype, act, ts, stags, r=r)
        _gate(got, *E.expect(act, dtype, ts, r, fused=True), "%s %s %s + shortcut" % (name, form, act), stags, ts)
        # (float32 storage has no tie and no witness of a second rounding: E.shortcut_cases plants those as "plain")
        kinds = {"shortcut: inexact", "shortcut: cancel", "shortcut: inf", "shortcut: nan"}
        assert set(stags) >= kinds | (set() if dtype == "float32" else {"shortcut: witness", "shortcut: tie"}), sorted(set(stags))


@pytest.mark.parametrize("dtype", ("bf16", "fp16"))
@pytest.mark.parametrize("form", FORMS)
def test_grouped_conv_shortcut_operand_non_finite(form, dtype):
    """inf + -inf, finite + NaN, NaN + inf: the pairs of tests/test_gpu_epilogue.py test_shortcut_operand_non_finite"""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    pairs = [(inf, -inf), (-inf, inf), (np.float32(1.5), nan), (nan, inf), (inf, inf), (-inf, np.float32(2.0)), (nan, nan),
             (np.float32(-3.0), -inf)]
    n = GS.EPILOGUE_C
    t2 = np.asarray([pairs[c % len(pairs)][0] for c in range(n)], dtype=np.float32)
    r2 = np.asarray([pairs[c % len(pairs)][1] for c in range(n)], dtype=np.float32)
    tags = ["shortcut: %r + %r" % (float(a), float(b)) for a, b in zip(t2, r2)]
    for act in ("linear", "leaky"):
        got, name = _run_form(form, dtype, act, t2, tags, r=r2)
        lo, hi, isnan = E.expect(act, dtype, t2, r2)
        assert isnan[0] and isnan[2] and np.isinf(lo[4])
        _gate(got, lo, hi, isnan, "%s %s %s non-finite shortcut operand" % (name, form, act), tags, t2)
