"""Kernel choice of every plan step, without a GPU (tools/make_kernel_choice.py writes tests/golden/kernel_choice.json,
tests/test_kernel_choice.py checks it).

The ops are those ``Darknet`` compiles: ``build_ops`` takes the description of a ``Darknet`` on the CPU through ``build_plan`` and
``plan_ops.fill_ops``, the product's own translation, and hands it fake, aligned device addresses in place of the arena, the
parameters and the output buffers.  Every conv whose kernel reads fragment-order weights gets a (fake) ``d_weight_frag``, so
``y3_plan_create_ex`` neither allocates nor launches anything: it only decides.  Never hand these ops to a library that can see a GPU (the test skips when torch sees one)."""
import ctypes
import functools
import os

from yolov3 import _hip
from yolov3.darknet import DTYPES, Darknet
from yolov3.plan import build_plan
from yolov3.plan_ops import fill_ops, padded_weight_dims

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
    """distinct, 4 KiB-aligned fake device addresses: called for one, and the ``mem`` of ``plan_ops.fill_ops``"""

    def __init__(self, convs=(), es=4):
        self.next = 1 << 44
        self.convs, self.es = convs, es

    def __call__(self, nbytes):
        a = self.next
        self.next += (max(int(nbytes), 1) + 4095) // 4096 * 4096 + 4096
        return a

    def arena(self, nbytes):
        self.base = self(nbytes)
        return self.base

    def conv(self, slot, path):
        c = self.convs[slot]
        cout_pad, k_ld = padded_weight_dims(path, c["cout"], c["cin"], c["k"], self.es)
        return self(cout_pad * k_ld * self.es), self(cout_pad * 4), self(cout_pad * 4)

    def fragment(self, slot, op, nbytes):
        return self(nbytes)

    def outputs(self, batch, rows_total):
        return self(batch * rows_total * 16), self(batch * rows_total * 4), self(batch * rows_total * 8)


@functools.lru_cache(maxsize=None)
def network(model, dtype, pool="reference", scores="reference", multi_label=False):
    """the description of a shipped cfg, a ``Darknet`` on the CPU: parsed once, read only"""
    return Darknet(os.path.join(MODEL_DIR, model + ".cfg"), dtype=dtype, pool=pool, scores=scores, multi_label=multi_label)


def build_ops(model, dim, dtype, batch, input_mode, opt, width=None, pool="reference", scores="reference", multi_label=False):
    """the ops of one plan (a ctypes array) as ``Darknet`` compiles them -- its description, ``build_plan`` and
    ``plan_ops.fill_ops`` -- on fake addresses, the fragment-weight bytes of each conv (None for other ops) asked under ``opt``,
    and the allocator.  The input is ``dim`` x ``dim``, or ``dim`` high and ``width`` wide.  A ``multi_label`` network
    compiles with ``fuse_head=0`` (``plan_ops.multi_label_options``): the caller's ``opt`` must say so."""
    net = network(model, dtype, pool, scores, multi_label)
    es = DTYPES[net.dtype][1]
    desc = build_plan(net.blocks, net.net_info, batch, dim, width or dim, es, reuse=not net.keep_all, fuse=net.fuse,
                      pool=net.pool, keep_heads=net.multi_label)
    fake = _Fake(net._convs, es)
    ops, _, frag = fill_ops(desc, net.net_info, net._convs, net.dtype, batch, input_mode, net.scores, opt, fake)
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
