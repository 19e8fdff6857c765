"""Plans and launches at the CU counts of a partitioned GPU (tests/test_cu_count_host.py without a GPU, tests/test_gpu_cu_count.py
on an MI355X).

An MI355X in DPX, QPX or CPX compute-partition mode presents devices of 128, 64 or 32 compute units.  The library reads the
count at plan creation only (csrc/api.hip y3_device_cus); ``y3_set_tuning("device_cus", n)`` -- ``_hip.device_cus(n)`` -- makes
every chooser see ``n`` instead, so the plans such a device gets are made, and run, on an ordinary one: a grid of 32
workgroups computes the same values on 256 CUs as on 32, since no kernel here synchronises between workgroups.

COUNTS: 32, 64 and 128 are the partitions, 256 the whole chip.  1 and 20 are stress values: at 1 one workgroup owns every tile
of a persistent grid and every ``n_cu / 4`` threshold is zero; 20 is no multiple of 8, so csrc/common.h y3_xcd_remap takes its
``r != 0`` branch, and none of 3, so csrc/conv_1x1.hip wres_geom takes its ``n_cu % n_tiles`` branch."""
import ctypes

from yolov3 import _hip

import footprint_util as fu
import kernel_choice_util as kc

COUNTS = (1, 20, 32, 64, 128, 256)
GPU_COUNTS = (1, 20, 32, 64, 128)          # none above the device's own count
OWN = 256                                  # the count of an unpartitioned MI355X, and of a machine without a GPU

MODELS = (("yolov3", 608), ("yolov3-spp", 608), ("yolov3-tiny", 416), ("yolov4", 608), ("yolov4-tiny", 416))
_D = _hip.AM_DEFAULT
# (the sets of kernel_choice_util.OPTION_SETS whose choosers read the count)
OPTION_SETS = {
    "default": {},
    "tile256": {"auto_mask": _D | _hip.AM_HALO_TILE256},
    "small_dw_always": {"auto_mask": _D | _hip.AM_SMALL_DW_ALWAYS},
    "wres_always": {"auto_mask": (_D & ~_hip.AM_SMALL_DW) | _hip.AM_WRES_ALWAYS},
    "fuse_block2": {"fuse_block": 2},
    "fuse_stem2": {"fuse_stem": 2},
}

MAX_BLOCK, MAX_LDS = 1024, 160 * 1024

# The new rows of footprint_util.cases() for the persistent families, and the count (20) at which they must spread unevenly
PERSISTENT_ROWS = ("wres_128_strided_tiles", "wres_64_strided_tiles", "patch_strided_tiles", "stem_s2_strided_tiles",
                   "stem_s2_phased_strided_tiles", "resblock_strided_tiles")


def plan_steps(model, dim, dtype, batch, overrides, width=None, input_mode="u8"):
    """[{"kernel", "dims": (grid, block, lds), "op": a copy of the y3_op} per op] of the plan made on fake addresses under the CU
    count in force (kernel_choice_util.build_ops: the ops ``Darknet`` compiles)"""
    lib = _hip.lib()
    opt = _hip.options(**overrides)
    ops, _, fake = kc.build_ops(model, dim, dtype, batch, input_mode, opt, width)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        return [dict(kernel=lib.y3_plan_op_kernel(handle, i).decode(), dims=_hip.plan_op_dims(handle, i), op=_copy(ops[i]))
                for i in range(len(ops))]
    finally:
        lib.y3_plan_destroy(handle)


def _copy(op):
    c = _hip.Y3Op()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(op), ctypes.sizeof(op))
    return c


def case_steps(case, dtype, opt_name=None, mode="strided"):
    """the same for a row of footprint_util.cases() (fake addresses): [{"kernel", "dims", "op"} per op]"""
    lib = _hip.lib()
    opt = _hip.options(**fu._opts()[opt_name or case["opt"]])
    ops, lay, _, _ = fu.build(case, dtype, mode, opt)
    # (a fused pair that this count or option set leaves as two launches: its convs may read fragment-order weights, of which the
    # layout holds none -- on the GPU the plan makes private copies; here a fake address, so that creation only decides)
    for n in range(len(ops)):
        if ops[n].kind == _hip.OP_CONV and not ops[n].d_weight_frag:
            if int(lib.y3_conv_fragment_weight_bytes(ctypes.byref(ops[n]), ctypes.byref(opt))):
                ops[n].d_weight_frag = (1 << 45) + (n << 32)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), lay["zero page"].ptr(1 << 44), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        return [dict(kernel=lib.y3_plan_op_kernel(handle, i).decode(), dims=_hip.plan_op_dims(handle, i), op=_copy(ops[i]))
                for i in range(len(ops))]
    finally:
        lib.y3_plan_destroy(handle)


def sane(kernel, dims):
    """None, or what is wrong with the recorded launch of a launched step"""
    grid, block, lds = dims
    if grid < 1:
        return "%s: grid %d" % (kernel, grid)
    if block % 64 or not 64 <= block <= MAX_BLOCK:
        return "%s: block %d" % (kernel, block)
    if lds > MAX_LDS:
        return "%s: %d bytes of LDS" % (kernel, lds)
    if grid * block > fu.MAX_THREADS:
        return "%s: %d x %d threads" % (kernel, grid, block)
    return None


def launched(step):
    return not step["kernel"].startswith("(fused")


# ------------------------------------------------------------------------------------------------ the GPU list
# What tests/test_gpu_cu_count.py runs; tests/test_cu_count_host.py asserts that this list crosses every chooser rule that
# reads the count.

# one-op rows: (row of footprint_util.cases(), option set of footprint_util._opts() or None for the row's own, fields of the row
# replaced -- a shape at which one more rule decides by the count at a count that a partition has)
ONE_OP_ROWS = (
    # persistent grids
    ("wres_128_ragged", None, {}), ("wres_64_ragged", None, {}), ("wres_128_strided_tiles", None, {}), ("wres_64_strided_tiles", None, {}),
    ("patch_ragged", None, {}), ("patch_ragged_res", None, {}), ("patch_strided_tiles", None, {}),
    ("stem_s2_ragged", None, {}), ("stem_s2_phased_ragged", None, {}), ("stem_s2_strided_tiles", None, {}),
    ("stem_s2_phased_strided_tiles", None, {}), ("resblock_ragged", None, {}), ("resblock_strided_tiles", None, {}),
    # the fused block: its rectangle, and under fuse_block = 1 the 70 % rule
    ("block_ragged_res", None, {}), ("block_ragged_nores", None, {}), ("block_ragged_res", "fuse_block1", {}), ("block_19x19_res", "fuse_block1", {}),
    # 192- against 256-pixel strips (11 x 4 tiles of 192 pixels are two rounds on 32 CUs, 8 x 4 of 256 are one), the strip kernels'
    # cost model, and the small-grid rule of the default set without the small-grid kernel (44 strip tiles: few on 256 CUs, not on 32)
    ("halo192_ragged", None, {}), ("halo192_ragged_res", None, {}), ("halo192_ragged_res", None, {"cout": 512}), ("halo256_ragged", None, {}),
    ("halo_dw_ragged", None, {}), ("halo_dw_ragged_res", None, {}), ("halo_dw_ragged_29x27", None, {}), ("halo_dw_ragged_29x27", "halo_dw_pays", {}),
    ("halo192_ragged_res", "no_small_dw", {"cout": 512}),
    # wave counts and grid limits of the small-grid kernel (the row's own set forces the widest workgroup whatever the count)
    ("dw48_k1_ragged", None, {}), ("dw48_k3_ragged", None, {}), ("dw48_k3s2_ragged", None, {}),
    ("dw48_k1_ragged", "dw48_auto", {}), ("dw48_k3_ragged", "dw48_auto", {}), ("dw48_k3_ragged_res", "dw48_auto", {}), ("dw48_k3s2_ragged", "dw48_auto", {}),
    # one round of between n_cu / 4 and n_cu tiles
    ("dw1x1_96_ragged", None, {}), ("dw1x1_48_ragged", None, {}),
    # the channel-tile shrink and the 96 x 64 tiles of the LDS-DMA implicit GEMM (27 tiles of 96 x 64 fill 32 CUs in one round where
    # 40 of 128 x 32 need two; 36 K-tiles in float32), and the deep-1x1 rule (24 tiles of 128 x 128: a quarter of 32 CUs, not of 256)
    ("igemm2_128_ragged", "igemm2", {}), ("igemm2_128_ragged", None, {}), ("igemm2_64_ragged_res", "igemm2", {}), ("igemm2_128_ragged_s2_res", "igemm2", {}),
    ("igemm2_64_ragged_res", "igemm2", {"B": 3, "h": 29, "w": 29, "cin": 128}),
    ("igemm3_128_ragged", "deep_1x1", {"cin": 1024, "cout": 512}),
)


def one_op_name(cid, opt, over):
    return "-".join([cid, opt or "own"] + ["%s%s" % kv for kv in sorted(over.items())])


def one_op_case(cid, over):
    return dict(fu.case_by_id(cid), **over)


def one_op_ids():
    return [(n, dtype) for n, (cid, opt, over) in enumerate(ONE_OP_ROWS) for dtype in fu.case_by_id(cid)["dtypes"]]

# whole networks: (model, height, width, batch, option set), every dtype ("wres_always": the 16-bit ones, the kernel has no other)
NET_COUNTS = (1, 32, 128)
NET_OPTIONS = {"default": {}, "wres_always": OPTION_SETS["wres_always"]}
NETS = (("yolov3", 160, 224, 3, "default"), ("yolov3-spp", 160, 224, 3, "default"), ("yolov3-tiny", 160, 224, 3, "default"),
        ("yolov3", 160, 224, 3, "wres_always"))
# in the 16-bit plans of yolov3 under 32 CUs
NET_EXPECT = {"default": ("conv_stem_s2_fused", "conv_resblock_fused", "conv1x1_dw"),
              "wres_always": ("conv_stem_s2_fused", "conv_resblock_fused", "conv1x1_wres_bf16_128x128", "conv1x1_wres_bf16_128x64")}


def net_dtypes(oname):
    return kc.DTYPE_NAMES if oname == "default" else ("bf16", "fp16")


# ------------------------------------------------------------------------------------------------ the chooser rules
# Every rule of csrc that reads the count, as a predicate on one op's step at the device's own count (a) and at another (b): whether
# THIS rule decided differently.  ``op`` is the y3_op.

def _k(step):
    return step["kernel"]


def _is16(op):
    return op.dtype != 0


RULES = {
    # csrc/conv_1x1.hip dw1x1_bm: one round of between n_cu / 4 and n_cu tiles
    "dw1x1_bm": lambda a, b, op: _k(a).startswith("conv1x1_dw_") != _k(b).startswith("conv1x1_dw_") or (
        _k(a).startswith("conv1x1_dw_") and _k(a) != _k(b)),
    # csrc/conv_dw48.hip dw48_waves: the fewest waves per workgroup whose grid still fits the chip
    "dw48_waves": lambda a, b, op: _k(a).startswith("conv_dw48_") and _k(a) == _k(b) and a["dims"] != b["dims"],
    # ... and its 3 n_cu / 2 (3x3) and 8 n_cu (1x1) limits of a grid over one round
    "dw48_limits_k3": lambda a, b, op: op.ksize == 3 and _k(a).startswith("conv_dw48_") != _k(b).startswith("conv_dw48_"),
    "dw48_limits_k1": lambda a, b, op: op.ksize == 1 and _k(a).startswith("conv_dw48_") != _k(b).startswith("conv_dw48_") and not (
        _k(a).startswith("conv1x1_dw_") or _k(b).startswith("conv1x1_dw_")),
    # csrc/conv_halo.hip halo_tile_fragments: 192- against 256-pixel strips
    "halo_tile": lambda a, b, op: _k(a).startswith("conv_halo_ws_") and _k(b).startswith("conv_halo_ws_") and _k(a) != _k(b),
    # csrc/conv_halo.hip y3_conv_halo_dw_pays
    "halo_dw_pays": lambda a, b, op: _k(a).startswith("conv_halo_") and _k(b).startswith("conv_halo_") and (
        _k(a).startswith("conv_halo_dw_") != _k(b).startswith("conv_halo_dw_")),
    # csrc/api.hip choose_conv small_grid: a 3x3 layer of fewer than 3 n_cu / 4 strip tiles goes to the implicit GEMM
    "small_grid": lambda a, b, op: op.ksize == 3 and op.stride == 1 and _is16(op) and (
        _k(a).startswith("conv_igemm3_") != _k(b).startswith("conv_igemm3_")) and (
        _k(a).startswith(("conv_halo_", "conv_patch_")) or _k(b).startswith(("conv_halo_", "conv_patch_"))),
    # csrc/api.hip choose_conv: 1x1 layers with 1024+ input channels, from n_cu / 4 tiles of 128 x 128 on
    "deep_1x1": lambda a, b, op: op.ksize == 1 and op.in_c >= 1024 and (
        _k(a).startswith("conv_igemm3_") != _k(b).startswith("conv_igemm3_")) and (
        _k(a).startswith("conv_igemm") and _k(b).startswith("conv_igemm")),
    # csrc/conv_igemm.hip y3_choose_conv_igemm: the channel tile halves while the grid leaves CUs without a workgroup
    "bn_shrink": lambda a, b, op: _k(a).startswith("conv_igemm2_") and _k(b).startswith("conv_igemm2_") and "_128x" in _k(a) and "_128x" in _k(b) and _k(a) != _k(b),
    # ... and 96 x 64 tiles where they fill one round and the tile above does not
    "igemm2_96x64": lambda a, b, op: _k(a).startswith("conv_igemm2_") and _k(b).startswith("conv_igemm2_") and (
        _k(a).endswith("_96x64") != _k(b).endswith("_96x64")),
    # csrc/conv_block.hip choose_tile: the rectangle by rounds over the count (a non-persistent grid: one workgroup a rectangle)
    "block_tile": lambda a, b, op: _k(a).startswith("conv_block_fused_") and _k(a) == _k(b) and a["dims"][0] != b["dims"][0],
    # ... and the 70 % rule of fuse_block = 1
    "block_70_percent": lambda a, b, op: _k(a).startswith("conv_block_fused_") != _k(b).startswith("conv_block_fused_"),
    # the persistent grids (csrc/conv_1x1.hip wres_geom, csrc/conv_halo.hip patch_geom, csrc/conv_fused.hip fused_geom)
    "wres_grid": lambda a, b, op: _k(a).startswith("conv1x1_wres_") and _k(a) == _k(b) and a["dims"][0] != b["dims"][0],
    "patch_grid": lambda a, b, op: _k(a).startswith("conv_patch_wsp_") and _k(a) == _k(b) and a["dims"][0] != b["dims"][0],
    "stem_s2_grid": lambda a, b, op: _k(a).startswith("conv_stem_s2_fused_") and _k(a) == _k(b) and a["dims"][0] != b["dims"][0],
    "resblock_grid": lambda a, b, op: _k(a).startswith("conv_resblock_fused_") and _k(a) == _k(b) and a["dims"][0] != b["dims"][0],
}


def gpu_list_plans(count):
    """{configuration name: [step per op]} of everything tests/test_gpu_cu_count.py runs, planned under ``count`` on fake addresses"""
    out = {}
    with _hip.device_cus(0 if count == OWN else count):
        for cid, opt, over in ONE_OP_ROWS:
            case = one_op_case(cid, over)
            for dtype in case["dtypes"]:
                out["%s|%s" % (one_op_name(cid, opt, over), dtype)] = case_steps(case, dtype, opt)
        for model, h, w, batch, oname in NETS:
            for dtype in net_dtypes(oname):
                out["%s|%dx%d|b%d|%s|%s" % (model, h, w, batch, oname, dtype)] = plan_steps(model, h, dtype, batch, NET_OPTIONS[oname], width=w)
    return out


def reach_table():
    """[(rule, count, configuration, kernel and grid at 256, kernel and grid at count)]: per rule and count of GPU_COUNTS the first
    configuration of the GPU list in which the rule decides differently than at 256; a rule nothing crosses has no line"""
    own = gpu_list_plans(OWN)
    found = {}
    for count in GPU_COUNTS:
        other = gpu_list_plans(count)
        for name in own:
            for a, b in zip(own[name], other[name]):
                if not launched(a) and not launched(b):
                    continue
                for rule, crossed in RULES.items():
                    if (rule, count) not in found and crossed(a, b, a["op"]):
                        found[rule, count] = (rule, count, name, "%s grid %d" % (_k(a), a["dims"][0]), "%s grid %d" % (_k(b), b["dims"][0]))
    return [found[r, c] for r in RULES for c in GPU_COUNTS if (r, c) in found]


def reach_lines(table):
    """the table as DESIGN.md holds it: per rule the crossing at the LARGEST count (the nearest to the whole chip) and the counts of all"""
    lines = []
    for rule in RULES:
        rows = [r for r in table if r[0] == rule]
        if rows:
            _, count, name, a, b = rows[-1]
            lines.append("| %s | %s | %d | %s | %s | %s |" % (rule, ", ".join(str(r[1]) for r in rows), count, name.replace("|", " "), a, b))
    return lines


def uneven(case, op, grid, tiles):
    """None, or why the workgroups of a persistent ``grid`` do not own two different numbers of the ``tiles``, both at least 2.  A
    workgroup owns tile0, tile0 + grid, ...: ceil or floor of tiles / grid.  The weights-resident kernel deals the PIXEL tiles of each
    channel tile to grid / n_tiles workgroups (csrc/conv_1x1.hip: mstride)."""
    if case["family"].startswith("conv1x1_wres"):
        n_tiles = op.out_c // int(case["family"].rsplit("x", 1)[1])
        if grid % n_tiles or tiles % n_tiles:
            return "grid %d or %d tiles no multiple of %d channel tiles" % (grid, tiles, n_tiles)
        grid, tiles = grid // n_tiles, tiles // n_tiles
    if tiles % grid == 0:
        return "%d tiles on %d workgroups: every workgroup owns %d" % (tiles, grid, tiles // grid)
    if tiles < 2 * grid:
        return "%d tiles on %d workgroups: some own one" % (tiles, grid)
    return None
