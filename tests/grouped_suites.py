"""The grouped and depthwise conv kernels (csrc/conv_grouped.hip) in the kernel-level suites: the tables and builders shared by
tests/test_gpu_grouped_epilogue.py (epilogue pins), tests/test_gpu_grouped_big.py (operands past 4 GiB) and their host half in
tests/test_grouped_host.py, which also holds both tables to the library's census (the "grouped" library of
tests/kernel_census.py, tests/golden/kernel_instances_grouped.json): an instance compiled later fails there until it has an epilogue form and a big row.

No GPU is needed to import this module; ``build`` lays an op out on fake addresses unless it is given the allocation's.
"""
import numpy as np

import footprint_util as fu
import grouped_cases as GC

INSTANCES = ("dwise_k3s1", "dwise_k3s2", "dwise_kn", "grouped_oc8", "grouped_oc1")
FAKE_BASE = 1 << 44


def census_key(instance, dtype):
    return "grouped_%s-%s" % (instance, dtype)


def kernel_name(instance, dtype):
    return "conv_%s" % instance.replace("_", "_%s_" % fu.TAG[dtype], 1)


def instance_of(case):
    """the compiled instance a case of tests/grouped_cases.py runs on by default"""
    if GC.is_dwise(case):
        return "dwise_k3s%d" % case["s"] if case["k"] == 3 and case["s"] in (1, 2) else "dwise_kn"
    return "grouped_oc8" if (case["cout"] // case["groups"]) % 8 == 0 else "grouped_oc1"


# ---------------------------------------------------------------------------------------------- epilogue forms
# One-op plans with zero weights, so that channel c's pre-activation is its bias bit for bit (tests/epilogue_cases.py): 128 output
# channels hold the whole planted list, B = 2 on a 5 x 7 map.  A width of 7 gives the depthwise kernel a full run of four output
# pixels and a run of three.  ``off``: every activation operand 8 bytes past the 16-byte grain (GC.strides), which takes
# conv_grouped's eight-channel epilogue through its per-element branch (vec_out == 0); the form without it stores 16 bytes at once.
EPILOGUE_B, EPILOGUE_H, EPILOGUE_W, EPILOGUE_C = 2, 5, 7, 128
EPILOGUE_FORMS = {
    "dwise_k3s1": dict(instance="dwise_k3s1", cin=128, groups=128, k=3, s=1, pad=1),
    "dwise_k3s2": dict(instance="dwise_k3s2", cin=128, groups=128, k=3, s=2, pad=1),
    "dwise_kn": dict(instance="dwise_kn", cin=128, groups=128, k=5, s=1, pad=2),
    "grouped_oc8_vec": dict(instance="grouped_oc8", cin=32, groups=4, k=3, s=1, pad=1),
    "grouped_oc8_elem": dict(instance="grouped_oc8", cin=32, groups=4, k=3, s=1, pad=1, wide=True, off=4),
    "grouped_oc1": dict(instance="grouped_oc1", cin=32, groups=32, k=3, s=1, pad=1),
}


def epilogue_case(form):
    """the form as a case of tests/grouped_cases.py (its ``strides``, ``out_hw`` and ``device_weights`` apply)"""
    f = EPILOGUE_FORMS[form]
    case = dict(id="epilogue_" + form, cout=EPILOGUE_C, h=EPILOGUE_H, w=EPILOGUE_W, B=EPILOGUE_B, **f)
    assert instance_of(case) == f["instance"], form
    return case


# ---------------------------------------------------------------------------------------------- rows past 4 GiB
# One row per instance, float32 and bf16 (fp16 shares bf16's address code, as in footprint_util.big_cases()).  Odd maps (for the
# stride-2 instance an odd OUTPUT map, 9 x 9 -> 5 x 5), a shortcut operand, and every activation operand a channel slice of a
# wider stride of its own, so that in_ld, out_ld and res_ld all differ and a frame's byte size is no power of two.  120 channels
# keep the three strides (136, 168, 200) close, and with them the allocation small.  conv_grouped runs at VALU speed: 8 -> 8
# channels a group on the eight-channel form; the one-element form has 16 output channels, so that one thread per output
# element stays below the launch limit while the bytes pass 2^32.  k = 3 throughout but the any-size depthwise instance.
BIG_DTYPES = ("float32", "bf16")
BIG_ROWS = {
    "dwise_k3s1": GC._dw("big_dw_k3s1", 120, 13, 11, res=True),
    "dwise_k3s2": GC._dw("big_dw_k3s2", 120, 9, 9, s=2, res=True),
    "dwise_kn": GC._dw("big_dw_kn", 120, 13, 11, k=5, pad=2, res=True),
    "grouped_oc8": GC._gr("big_gr_oc8", 64, 64, 8, 13, 11, res=True),
    "grouped_oc1": GC._gr("big_gr_oc1", 16, 16, 4, 13, 11, res=True),
}
SPAN_OPERANDS = ("input", "output", "residual")


def flags(case):
    H = fu._H()
    act = {"leaky": H.F_LEAKY, "linear": 0, "mish": H.F_MISH, "logistic": H.F_LOGISTIC}[case.get("act", "leaky")]
    return act | (H.F_RESIDUAL if case.get("res") else 0)


def build(case, dtype, B, mode, base=None, lead=()):
    """(ops, layout) of a one-op plan of ``case`` at batch ``B``: every operand between guards in ONE allocation at ``base`` (fake
    addresses without one).  ``mode`` "strided": the activation operands are channel slices of wider strides, each its own;
    "dense": c0 = 0, ld = c."""
    H = fu._H()
    path = GC.PATH_DWISE if GC.is_dwise(case) else GC.PATH_GROUPED
    cin, cout, k = case["cin"], case["cout"], case["k"]
    ho, wo = GC.out_hw(case)
    used = set()
    operands = list(lead) + [fu._act(used, "input", "in", dtype, B * case["h"] * case["w"], cin, mode, 8, 0),
                             fu._act(used, "output", "out", dtype, B * ho * wo, cout, mode, 8, 1)]
    if case.get("res"):
        operands.append(fu._act(used, "residual", "in", dtype, B * ho * wo, cout, mode, 8, 2))
    host, cp, k_ld = GC.device_weights(case, path, np.zeros((cout, cin // case["groups"], k, k), dtype=np.float32))
    operands += [fu.flat("weight", "in", dtype, host.size), fu.flat("scale", "in", "float32", cp), fu.flat("bias", "in", "float32", cp),
                 fu.flat("zero page", "in", dtype, 4096 // fu.ES[dtype])]
    lay = fu.Layout(operands)
    base = FAKE_BASE if base is None else base
    ops = (H.Y3Op * 1)()
    op = ops[0]
    op.kind, op.dtype, op.batch, op.block_idx, op.flags = H.OP_CONV, fu.DT_CODE[dtype], B, 1, flags(case)
    op.in_h, op.in_w, op.in_c, op.in_ld = case["h"], case["w"], cin, lay["input"].ld
    op.out_h, op.out_w, op.out_c, op.out_ld = ho, wo, cout, lay["output"].ld
    op.ksize, op.stride, op.pad, op.groups = k, case["s"], case["pad"], case["groups"]
    op.cout_pad, op.k_ld = cp, k_ld
    op.d_in, op.d_out = lay["input"].ptr(base), lay["output"].ptr(base)
    if case.get("res"):
        op.d_res, op.res_ld = lay["residual"].ptr(base), lay["residual"].ld
    op.d_weight, op.d_scale, op.d_bias = lay["weight"].ptr(base), lay["scale"].ptr(base), lay["bias"].ptr(base)
    return ops, lay


def span_operands(lay):
    return [lay[n] for n in SPAN_OPERANDS if lay.has(n)]


def big_batch(case, dtype):
    """frames that put every activation operand more than 2^32 bytes plus one frame long (footprint_util.big_batch's rule)"""
    _, lay = build(case, dtype, 3, "strided")
    frames = [o.body_bytes // 3 for o in span_operands(lay)]
    assert all(f * 3 == o.body_bytes for f, o in zip(frames, span_operands(lay)))
    return max((fu.SPAN + f) // f + 1 for f in frames)


def frame_pixels(case):
    ho, wo = GC.out_hw(case)
    return max(case["h"] * case["w"], ho * wo)


def launch_threads(case, B):
    """grid x block of the case's launch at batch ``B``, restated from csrc/conv_grouped.hip: conv_dwise has one lane per 8-channel
    chunk of a run of four output pixels along x, conv_grouped one per pixel and ``bn`` (8 or 1) output channels; blocks of 256"""
    ho, wo = GC.out_hw(case)
    if GC.is_dwise(case):
        lanes = B * ho * -(-wo // 4) * (case["cout"] // 8)
    else:
        lanes = B * ho * wo * (case["cout"] // (8 if instance_of(case) == "grouped_oc8" else 1))
    return -(-lanes // 256) * 256


def create(ops, lay, base=None):
    """(kernel name, (workgroups, block, LDS bytes), None) or (None, None, the library's message) of plan creation"""
    import ctypes
    H = fu._H()
    lib = H.lib()
    handle = ctypes.c_void_p()
    rc = lib.y3_plan_create_ex(ops, 1, lay["zero page"].ptr(FAKE_BASE if base is None else base), None, ctypes.byref(handle))
    if rc != 0:
        return None, None, lib.y3_last_error().decode()
    try:
        return lib.y3_plan_op_kernel(handle, 0).decode(), H.plan_op_dims(handle, 0), None
    finally:
        lib.y3_plan_destroy(handle)
