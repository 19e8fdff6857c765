"""The direct-weights fused block kernel (csrc/conv_block_dw.hip, libyolov3_hip_block.so; y3_options.fuse_block = 3 / 4) in the
kernel-level suites: a case table of its own in the row format of tests/footprint_util.py ``cases()``, shared by
tests/test_gpu_block_dw_suites.py (footprint trio, exact sums, the row below 2^32 bytes), tests/test_block_dw_host.py (which holds
the table on the CPU and every suite to the library's census) and tools/make_kernel_instances.py.

The rows are NOT rows of ``cases()``: the kernel lives in a library of its own, the "block" row of tests/kernel_census.py, with a
fixture of its own (tests/golden/kernel_instances_block.json), and the main library's rules would refuse symbols it lacks.  They
run under the option set ``fuse_block4`` of footprint_util._opts(), for which footprint_util.build registers fragment-order
copies of BOTH convs' weights.

No GPU is needed to import this module."""
import footprint_util as fu

FAMILY = "conv_block_dw_%s_x128"
OPT = "fuse_block4"
DTYPES = fu.B16
# rows of footprint_util.cases() taken as they are, but for family and option set
FROM_CASES = ("block_full_res", "block_ragged_res", "block_ragged_nores", "block_19x19_res")

# The smallest map csrc/conv_block.hip choose_tile accepts: its rectangles are tw = 8 .. 24 pixels wide and th >= 4 high, and
# ``if (tw > W || th < 4) continue`` declines every width of a map under 8 pixels across and every height of one under 4
SMALLEST_H, SMALLEST_W = 4, 8


def _row(cid, B, h, w, cin, cout, res, **kw):
    return dict(id=cid, group="block", family=FAMILY, opt=OPT, dtypes=DTYPES, B=B, h=h, w=w, cin=cin, cout=cout, res=res, **kw)


def cases():
    """The smallest shapes at which the kernel can still go wrong (the kernel's grid is one workgroup per rectangle per frame; an
    output pass is 128 channels; phase A streams x in sub-steps of 32 channels through a ring of four buffers):

    the four block rows of cases()  32 x 32 cut 2 x 2 into exact 16 x 16 rectangles; 19 x 13 and 21 x 17, one ragged rectangle a
                                    frame, Cin 192 -> 128 without a shortcut (six sub-steps, one pass); 19 x 19, one exact rectangle
    block_dw_25x43_res              2 x 2 rectangles of 13 x 22 that hang over the right and the bottom frame edge
    block_dw_19x19_c384_res         Cin = Cout = 384 WITH the shortcut: three output passes, the shortcut read at np * 128 = 256
    block_dw_19x19_c320             ten sub-steps: the x ring turns 2.5 times; one pass, no shortcut
    block_dw_smallest               8 x 4: one rectangle of 32 pixels a frame, 22 of the 24 pixel fragments empty, three of the
                                    four pixel groups of waves without a live store (ns == 0 in the write-out); B 37 as the tiny rows
    block_dw_19x19_b300             300 workgroups: more than one round on 256 CUs, no multiple of 8 through y3_xcd_remap, the L2
                                    warm-up's share at per_xcd = 38.  55 MB per operand
    block_dw_38x38_b5               20 workgroups: above 8, no multiple of 8"""
    C = [dict(fu.case_by_id(src), id=src.replace("block_", "block_dw_", 1), family=FAMILY, opt=OPT, src=src) for src in FROM_CASES]
    C += [
        _row("block_dw_25x43_res", 3, 43, 25, 256, 256, True),
        _row("block_dw_19x19_c384_res", 3, 19, 19, 384, 384, True),
        _row("block_dw_19x19_c320", 3, 19, 19, 320, 128, False),
        _row("block_dw_smallest", 37, SMALLEST_H, SMALLEST_W, 256, 256, True),
        _row("block_dw_19x19_b300", 300, 19, 19, 256, 256, True),
        _row("block_dw_38x38_b5", 5, 38, 38, 256, 256, True),
    ]
    return C


def case_ids():
    return [(c["id"], d) for c in cases() for d in c["dtypes"]]


def case_by_id(cid):
    return next(c for c in cases() if c["id"] == cid)


def grid(case):
    """workgroups of the case's launch: one per rectangle per frame (footprint_util.block_tile restates choose_tile)"""
    tw, th = fu.block_tile(case["h"], case["w"])
    return -(-case["w"] // tw) * -(-case["h"] // th) * case["B"]


# ---- the row one frame below 2^32 bytes (tests/test_gpu_block_dw_suites.py, tests/test_block_dw_host.py): the kernel keeps 32-bit
# byte offsets into x and z and y3_choose_conv_block_fused diverts the pair at 2^32 bytes of either.  footprint_util.big_cases()'s
# row of conv_block_fused under this kernel's option set: x and z at ONE stride, both within one frame below 2^32 bytes.
def big_row():
    src = fu.big_row("block_ragged_res")
    return dict(src, id="block_dw_ragged_res", family=FAMILY, opt=OPT, dtypes=("bf16",))


# ---- which compiled instance each suite launches: tests/test_block_dw_host.py holds every key below to the census
SUITES = ("footprint", "epilogue", "exact")
PLANTS = ("unit", "wide_x", "wide_w")


def footprint_key(cid, dtype):
    return "%s-%s" % (cid, dtype)


def exact_key(cid, dtype, plant):
    return "exact_%s_%s-%s" % (plant, cid, dtype)


def epilogue_key(dtype):
    return "epilogue_block_dw-%s" % dtype


def big_key(dtype="bf16"):
    return "big_block_dw_ragged_res-%s" % dtype


# ---- in a network (tests/test_gpu_block_dw_network.py; tests/test_block_dw_host.py holds the figures to the CPU plan): yolov3 at
# 160 x 224 x 3 frames under fuse_block = 4.  The /8 stage is a 20 x 28 map; its eight residual pairs and the first pair of the
# 76^2-branch (Cin 384, no shortcut) are named conv_block_dw; the last residual pair writes a 256-channel slice of a route
# buffer of 384.  Blocks are those of the pairs' 1x1 convs.
NET = ("yolov3", 160, 224, 3)
NET_BLOCKS = (13, 16, 19, 22, 25, 28, 31, 34, 99)
NET_ROUTE_SLICE = (34, 256, 384)          # block, channels, pixel stride of the output
