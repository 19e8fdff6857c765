"""Kernel choice of every plan step, without a GPU (tools/make_kernel_choice.py writes tests/golden/kernel_choice.json,
tests/test_kernel_choice.py checks it).

The ops are those ``Darknet._compile_on_device`` builds -- same plan description, flags, padded weight sizes -- with fake,
aligned device addresses in place of the arena, the parameters and the output buffers.  Every conv whose kernel reads
fragment-order weights gets a (fake) ``d_weight_frag``, so ``y3_plan_create_ex`` neither allocates nor launches anything: it
only decides.  Never hand these ops to a library that can see a GPU (the test skips when torch sees one)."""
import ctypes
import os

from yolov3 import _hip
from yolov3.darknet import DTYPES, _round_up
from yolov3.cfgparse import parse_config
from yolov3.plan import build_plan
from yolov3.weights import conv_layout

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MODEL_DIR = os.path.join(ROOT, "pytorch-yolov3_amd", "models")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_choice.json")

MODELS = (("yolov3", 608), ("yolov3-spp", 608), ("yolov3-tiny", 416))
DTYPE_NAMES = ("float32", "bf16", "fp16")
BATCHES = (1, 2, 3, 4, 8, 16)

_D = _hip.AM_DEFAULT
# (name, y3_options overrides): the defaults, what the pipeline asks for, and the sets the GPU tests and tools use
OPTION_SETS = (
    ("default", {}),
    ("tile256", {"auto_mask": _D | _hip.AM_HALO_TILE256}),
    ("am0", {"auto_mask": 0}),
    ("am63", {"auto_mask": 63}),
    ("am127", {"auto_mask": 127}),
    ("igemm1", {"igemm_version": 1}),
    ("igemm3_am0", {"igemm_version": 3, "auto_mask": 0}),
    ("igemm3", {"igemm_version": 3}),
    ("igemm3_bm64", {"igemm_version": 3, "igemm_bm": 64, "auto_mask": 0}),
    ("igemm3_bm64_ns3", {"igemm_version": 3, "igemm_bm": 64, "igemm_ns": 3, "auto_mask": 0}),
    ("igemm_bm96", {"igemm_bm": 96, "auto_mask": 0}),
    ("halo_dw_always", {"auto_mask": _D | _hip.AM_HALO_DW_ALWAYS}),
    ("small_dw_always", {"auto_mask": _D | _hip.AM_SMALL_DW_ALWAYS}),
    ("no_small_dw", {"auto_mask": _D & ~_hip.AM_SMALL_DW}),
    ("wres_always", {"auto_mask": (_D & ~_hip.AM_SMALL_DW) | _hip.AM_WRES_ALWAYS}),
    ("no_small_grid", {"auto_mask": _D | _hip.AM_NO_SMALL_GRID}),
    ("fuse_head0", {"fuse_head": 0}),
    ("fuse_head2", {"fuse_head": 2}),
    ("fuse_head3", {"fuse_head": 3}),
    ("fuse_head4", {"fuse_head": 4}),
    ("fuse_stem0", {"fuse_stem": 0}),
    ("fuse_stem2", {"fuse_stem": 2}),
    ("fuse_block1", {"fuse_block": 1}),
    ("fuse_block2", {"fuse_block": 2}),
    ("fuse_spp0", {"fuse_spp": 0}),
    ("decode_lanes1", {"decode_lanes": 1}),
)


def configs():
    """(key, model, dim, dtype, batch, input_mode, option overrides) of the whole matrix"""
    for model, dim in MODELS:
        for dtype in DTYPE_NAMES:
            for batch in BATCHES:
                for oname, over in OPTION_SETS:
                    for mode in ("u8", "f32") if oname == "default" else ("u8",):
                        key = "%s|%s|b%d|%s|%s" % (model, dtype, batch, mode, oname)
                        yield key, model, dim, dtype, batch, mode, over


class _Fake:
    """distinct, 4 KiB-aligned fake device addresses"""

    def __init__(self):
        self.next = 1 << 44

    def __call__(self, nbytes):
        a = self.next
        self.next += _round_up(max(int(nbytes), 1), 4096) + 4096
        return a


def build_ops(model, dim, dtype, batch, input_mode, opt, width=None):
    """the ops of one plan (a ctypes array) as Darknet._compile_on_device builds them, and the fragment-weight bytes of each
    conv (None for other ops) asked under ``opt``.  The input is ``dim`` x ``dim``, or ``dim`` high and ``width`` wide."""
    lib = _hip.lib()
    blocks, net_info = parse_config(os.path.join(MODEL_DIR, model + ".cfg"))
    for i, blk in enumerate(blocks):            # absolute route indices (Darknet.__init__)
        if blk["type"] == "route":
            blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
    _, convs = conv_layout(blocks, net_info)
    c_dtype, es = DTYPES[dtype][0], DTYPES[dtype][1]
    desc = build_plan(blocks, net_info, batch, dim, width or dim, es, reuse=True, fuse=True)
    fake = _Fake()
    base = fake(desc["arena_bytes"])

    def addr(t, elem):
        if t is None or t.buf == "input":
            return None
        return base + desc["offsets"][t.buf] + t.off * elem

    ops = (_hip.Y3Op * len(desc["ops"]))()
    frag = []
    for n, od in enumerate(desc["ops"]):
        op = ops[n]
        kind = od["kind"]
        op.dtype = c_dtype
        op.batch = batch
        op.block_idx = od["block"]
        tin = od["inp"]
        op.in_h, op.in_w, op.in_c, op.in_ld = tin.h, tin.w, tin.c, tin.ld
        if tin.buf == "input":
            op.flags |= _hip.F_PLAN_INPUT
            op.flags |= _hip.F_IN_NHWC_U8BGR if input_mode == "u8" else _hip.F_IN_NCHW_F32
        else:
            op.d_in = addr(tin, 4 if tin.f32 else es)
        tout = od.get("out")
        if tout is not None:
            op.out_h, op.out_w, op.out_c, op.out_ld = tout.h, tout.w, tout.c, tout.ld
            op.d_out = addr(tout, 4 if tout.f32 else es)
            if tout.f32 and es == 2:
                op.flags |= _hip.F_OUT_F32
        res = od.get("res")
        if res is not None:
            op.d_res = addr(res, es)
            op.res_ld = res.ld
        nfrag = None
        if kind == "conv":
            op.kind = _hip.OP_CONV
            op.ksize, op.stride, op.pad = od["ksize"], od["stride"], od["pad"]
            if od["leaky"]:
                op.flags |= _hip.F_LEAKY
            if od.get("fuse_next"):
                op.flags |= _hip.F_FUSE_NEXT
            if res is not None:
                op.flags |= _hip.F_RESIDUAL
            c = convs[od["slot"]]
            op.cout_pad = _round_up(c["cout"], 128)
            op.k_ld = _round_up(c["k"] * c["k"] * c["cin"], 128 // es)
            path = lib.y3_conv_path(ctypes.byref(op))
            if path == _hip.PATH_STEM_MFMA:                      # (Darknet._device_weights)
                op.cout_pad, op.k_ld = 32, 32
            elif path == _hip.PATH_STEM:
                op.cout_pad = op.k_ld = _round_up(c["cout"], 8)
            op.d_weight = fake(op.cout_pad * op.k_ld * es)
            op.d_scale = fake(op.cout_pad * 4)
            op.d_bias = fake(op.cout_pad * 4)
            nfrag = int(lib.y3_conv_fragment_weight_bytes(ctypes.byref(op), ctypes.byref(opt)))
            if nfrag:
                op.d_weight_frag = fake(nfrag)
        elif kind == "maxpool":
            op.kind = _hip.OP_MAXPOOL
            op.ksize, op.stride = od["ksize"], od["stride"]
        elif kind == "upsample":
            op.kind = _hip.OP_UPSAMPLE
            op.ksize, op.stride = 1, od["stride"]
        elif kind in ("add", "copy"):
            op.kind = _hip.OP_ADD if kind == "add" else _hip.OP_COPY
            op.ksize = op.stride = 1
        elif kind == "yolo":
            op.kind = _hip.OP_YOLO
            op.n_anchor = len(od["anchors"])
            op.n_attr = od["n_attr"]
            for a, (aw, ah) in enumerate(od["anchors"]):
                op.anchor_w[a] = float(aw)
                op.anchor_h[a] = float(ah)
            op.row_offset, op.rows_total = od["row_offset"], od["rows_total"]
            op.net_w, op.net_h = float(net_info["width"]), float(net_info["height"])
        else:
            raise AssertionError(kind)
        frag.append(nfrag)
    m = desc["rows_total"]
    bbox, prob, cls = fake(batch * m * 16), fake(batch * m * 4), fake(batch * m * 8)
    for n in range(len(ops)):
        if ops[n].kind == _hip.OP_YOLO:
            ops[n].d_bbox, ops[n].d_prob, ops[n].d_cls = bbox, prob, cls
    return ops, frag, fake


def plan_choice(model, dim, dtype, batch, input_mode, overrides, width=None):
    """{"kernel": [y3_plan_op_kernel per op], "frag": [y3_conv_fragment_weight_bytes per op, None for non-convs], "map": [(in_h, in_w)
    per op]}"""
    lib = _hip.lib()
    opt = _hip.options(**overrides)
    ops, frag, fake = build_ops(model, dim, dtype, batch, input_mode, opt, width)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        kernels = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
    finally:
        lib.y3_plan_destroy(handle)
    return {"kernel": kernels, "frag": frag, "map": [(ops[i].in_h, ops[i].in_w) for i in range(len(ops))]}


def all_choices():
    """{"rows": [[kernel, fragment bytes]], "plans": [[row index per op]], "configs": {config key: plan index}}: identical rows and
    identical plans stored once"""
    rows, row_ix, plans, plan_ix, cfgs = [], {}, [], {}, {}
    for key, model, dim, dtype, batch, mode, over in configs():
        ch = plan_choice(model, dim, dtype, batch, mode, over)
        plan = []
        for row in zip(ch["kernel"], ch["frag"]):
            if row not in row_ix:
                row_ix[row] = len(rows)
                rows.append(list(row))
            plan.append(row_ix[row])
        plan = tuple(plan)
        if plan not in plan_ix:
            plan_ix[plan] = len(plans)
            plans.append(list(plan))
        cfgs[key] = plan_ix[plan]
    return {"rows": rows, "plans": plans, "configs": cfgs}


def config_rows(table, key):
    """[[kernel, fragment bytes] per op] of one configuration of an all_choices() table"""
    return [table["rows"][r] for r in table["plans"][table["configs"][key]]]
