"""Whole networks on maps of one or two pixels a side: the rows of tests/test_gpu_tiny_maps.py, and the planner's word for them
(tests/test_tiny_maps_choice.py, no GPU).

A 32-pixel input gives yolov3, yolov3-spp and yolov3-tiny detection scales of 1 x 1, 2 x 2 and 4 x 4 maps, a 64-pixel input
2 x 2, 4 x 4 and 8 x 8, a 32 x 224 input 1 x 7, 2 x 14 and 4 x 28 (224 x 32: their transposes).  On such a map every pixel is a
border pixel on all four sides, a pixel tile holds dozens of whole frames, and a 13-wide pool window has one tap inside the image.

``ROWS``: one configuration each, with the (kernel, map) pairs it is there for.  A "map" is the INPUT map of the op (the
stride-2 kernels: 2 x 2 in, 1 x 1 out), and a pair is listed when the smaller side of that map is 1 or 2.  Kernel names carry
the bf16 tag; a float32 row's names are written out, an fp16 row is the bf16 row with "f16" in the names (``pairs_of``).  Every
row runs at batch 1 (an op is one to four pixels) and at one odd batch (every tile holds many whole frames and ends inside
one); tests/test_tiny_maps_choice.py holds each row to its pairs at BOTH batches through ``y3_plan_create_ex``, and holds the
union of the rows against every pair the planner can produce from the shipped yolov3 cfgs under
``kernel_choice_util.OPTION_SETS``, so a chooser rule that empties a row fails there, on a machine without a GPU."""
import kernel_choice_util as kc

OPTIONS = dict(kc.OPTION_SETS)
SQUARE_ODD_BATCH = 37           # 37 frames of a 1 x 1 map: a 128-pixel tile ends inside the batch, a 32-pixel one after frame 31
RECT_ODD_BATCH = 61             # 61 x 7 = 427 pixels of a 1 x 7 map: no tile size divides it, every tile boundary is inside a frame
MODELS = ("yolov3", "yolov3-spp", "yolov3-tiny")
SIDES = {1: (1, 1), 2: (2, 2)}


def _row(model, dim, dtype, opt, pairs):
    return dict(id="%s-%d-%s-%s" % (model, dim, dtype, opt), model=model, h=dim, w=dim, dtype=dtype, opt=opt,
                pairs=tuple((k, SIDES[s]) for k, sides in pairs for s in sides))


# (the order and the pairs of the table in DESIGN.md section 1, "Maps of one or two pixels")
ROWS = (
    _row("yolov3-spp", 32, "bf16", "fuse_head0", (
        ("conv_dw48_k1_bf16", (1, 2)), ("conv_dw48_k3_bf16", (1, 2)), ("conv_dw48_k3s2_bf16", (2,)),
        ("conv_igemm2_bf16_128x32", (1,)), ("conv_igemm_bf16_128x128", (1, 2)), ("maxpool_spp_pyramid_bf16", (1,)),
        ("upsample_bf16", (1, 2)), ("yolo_decode_f32", (1, 2)))),
    _row("yolov3-spp", 32, "bf16", "wres_always", (
        ("conv1x1_wres_bf16_128x128", (2,)), ("conv1x1_wres_bf16_128x64", (1, 2)), ("conv_head_decode_dw_bf16_48x256", (1, 2)),
        ("conv_igemm2_bf16_128x32", (2,)), ("conv_igemm3_bf16_128x128", (1, 2)))),
    _row("yolov3-spp", 32, "float32", "no_small_grid", (
        ("conv_halo_ws_f32_192x128", (1, 2)), ("conv_igemm2_f32_128x32", (1, 2)), ("conv_igemm3_f32_128x128", (1,)),
        ("maxpool_spp_pyramid_f32", (1,)), ("upsample_f32", (1, 2)), ("yolo_decode_f32", (1, 2)))),
    _row("yolov3-spp", 32, "bf16", "no_small_grid", (("conv_halo_ws_bf16_192x128", (1, 2)),)),
    _row("yolov3-tiny", 32, "bf16", "igemm3_bm64", (("conv_igemm3_bf16_64x128", (1, 2)), ("maxpool_bf16", (1, 2)))),
    _row("yolov3-tiny", 32, "float32", "igemm1", (("conv_igemm_f32_128x128", (1, 2)), ("maxpool_f32", (1, 2)))),
    _row("yolov3-spp", 32, "bf16", "igemm_bm96", (("conv_igemm2_bf16_96x64", (1, 2)),)),
    _row("yolov3-spp", 32, "float32", "igemm_bm96", (("conv_igemm2_f32_96x64", (1, 2)),)),
    _row("yolov3-spp", 32, "bf16", "fuse_head2", (("conv_head_decode_bf16_64x256", (1, 2)),)),
    _row("yolov3-tiny", 32, "bf16", "fuse_head4", (("conv_head_decode_dw_bf16_96x256", (1, 2)),)),
    _row("yolov3-tiny", 32, "bf16", "wres_always", (("conv1x1_wres_bf16_128x128", (1,)),)),
    _row("yolov3-spp", 64, "float32", "am63", (("conv_igemm3_f32_128x128", (2,)), ("maxpool_spp_pyramid_f32", (2,)))),
    _row("yolov3-spp", 64, "bf16", "default", (("maxpool_spp_pyramid_bf16", (2,)),)),
    # Darknet-53 without the pyramid, default options: what a user who changes nothing runs on a 32-pixel crop
    _row("yolov3", 32, "bf16", "default", (
        ("conv_dw48_k1_bf16", (1, 2)), ("conv_dw48_k3_bf16", (1, 2)), ("conv_dw48_k3s2_bf16", (2,)),
        ("conv_head_decode_dw_bf16_48x256", (1, 2)), ("upsample_bf16", (1, 2)))),
    _row("yolov3", 32, "float32", "default", (("conv_igemm2_f32_128x32", (1, 2)), ("upsample_f32", (1, 2)), ("yolo_decode_f32", (1, 2)))),
)

# fp16 shares the 16-bit templates: the rows of the no_small_grid and wres_always configurations and the default one
FP16_ROWS = tuple(dict(r, id=r["id"].replace("bf16", "fp16"), dtype="fp16") for r in ROWS
                  if r["dtype"] == "bf16" and r["opt"] in ("no_small_grid", "wres_always", "default"))

# Rectangular inputs, at the odd batch: the kernels the planner puts on the 1 x 7 maps of 32 x 224 and the 7 x 1 maps of 224 x 32
# (the same names both ways) per (dtype, option set); a model's own additions follow.  wres_always changes nothing in float32
# (the weights-resident kernel is 16-bit only): the row is kept, it costs a second.
RECT_SIZES = ((32, 224), (224, 32))
RECT_KERNELS = {
    ("bf16", "default"): ("conv_dw48_k1_bf16", "conv_dw48_k3_bf16", "conv_head_decode_dw_bf16_48x256", "upsample_bf16"),
    ("bf16", "no_small_grid"): ("conv_halo_ws_bf16_192x128", "conv_head_decode_dw_bf16_48x256", "conv_igemm2_bf16_128x32",
                                "conv_igemm3_bf16_128x128", "upsample_bf16"),
    ("bf16", "wres_always"): ("conv_head_decode_dw_bf16_48x256", "conv_igemm2_bf16_128x32", "conv_igemm3_bf16_128x128",
                              "upsample_bf16"),
    ("float32", "default"): ("conv_igemm2_f32_128x32", "upsample_f32", "yolo_decode_f32"),
    ("float32", "no_small_grid"): ("conv_halo_ws_f32_192x128", "conv_igemm2_f32_128x32", "conv_igemm3_f32_128x128", "upsample_f32",
                                   "yolo_decode_f32"),
    ("float32", "wres_always"): ("conv_igemm2_f32_128x32", "upsample_f32", "yolo_decode_f32"),
}
RECT_MODEL_KERNELS = {
    ("yolov3", "bf16", "wres_always"): ("conv1x1_wres_bf16_128x64",),
    ("yolov3-spp", "bf16", "default"): ("conv_igemm2_bf16_128x32", "maxpool_spp_pyramid_bf16"),
    ("yolov3-spp", "bf16", "no_small_grid"): ("maxpool_spp_pyramid_bf16",),
    ("yolov3-spp", "bf16", "wres_always"): ("conv1x1_wres_bf16_128x64", "maxpool_spp_pyramid_bf16"),
    ("yolov3-spp", "float32", "default"): ("maxpool_spp_pyramid_f32",),
    ("yolov3-spp", "float32", "no_small_grid"): ("maxpool_spp_pyramid_f32",),
    ("yolov3-spp", "float32", "wres_always"): ("maxpool_spp_pyramid_f32",),
    ("yolov3-tiny", "bf16", "default"): ("maxpool_bf16",),
    ("yolov3-tiny", "bf16", "no_small_grid"): ("maxpool_bf16",),
    ("yolov3-tiny", "bf16", "wres_always"): ("conv1x1_wres_bf16_128x128", "maxpool_bf16"),
    ("yolov3-tiny", "float32", "default"): ("maxpool_f32",),
    ("yolov3-tiny", "float32", "no_small_grid"): ("maxpool_f32",),
    ("yolov3-tiny", "float32", "wres_always"): ("maxpool_f32",),
}


def _rect_rows():
    rows = []
    for model in MODELS:
        for h, w in RECT_SIZES:
            for (dtype, opt), kernels in RECT_KERNELS.items():
                side = (1, 7) if h < w else (7, 1)
                names = kernels + RECT_MODEL_KERNELS.get((model, dtype, opt), ())
                rows.append(dict(id="%s-%dx%d-%s-%s" % (model, h, w, dtype, opt), model=model, h=h, w=w, dtype=dtype, opt=opt,
                                 pairs=tuple((k, side) for k in names)))
    return tuple(rows)


RECT_ROWS = _rect_rows()


def pairs_of(row):
    """the row's (kernel, (map height, map width)) pairs with the names of its dtype"""
    if row["dtype"] != "fp16":
        return row["pairs"]
    return tuple((k.replace("bf16", "f16"), m) for k, m in row["pairs"])


def is_tiny(m):
    return min(m) <= 2


def plan_pairs(kernels, maps, keep=is_tiny):
    """{(kernel, input map)} of a plan's ops, the ops fused into their predecessor left out; ``keep`` selects the maps"""
    return {(k, tuple(m)) for k, m in zip(kernels, maps) if not k.startswith("(fused") and keep(tuple(m))}


def planner_pairs(row, batch, keep=is_tiny):
    """what the CPU planner gives the row at ``batch`` (uint8 frames, as ``Darknet.forward_frames`` feeds them)"""
    ch = kc.plan_choice(row["model"], row["h"], row["dtype"], batch, "u8", OPTIONS[row["opt"]], width=row["w"])
    return plan_pairs(ch["kernel"], ch["map"], keep)


def net_pairs(net, keep=is_tiny):
    """the same of the plan a ``Darknet`` last ran"""
    cp = net._last_plan
    report = net.plan_report()
    return plan_pairs([r["kernel"] for r in report], [(cp.ops[i].in_h, cp.ops[i].in_w) for i in range(cp.n_ops)], keep)
