"""ctypes binding of libyolov3_hip.so (C ABI: include/yolov3_hip.h).

The library is hand-written HIP for gfx950 and is the ONLY compute backend of this
package: if it cannot be loaded, or no MI355X is visible, the entry points raise --
there is deliberately no CPU or PyTorch fallback.

``torch`` is imported first on purpose: PyTorch-ROCm ships its own libamdhip64.so.7
and must be the HIP runtime of the process, so that tensor ``data_ptr()`` addresses
and ``torch.cuda`` streams are valid inside this library (same runtime instance).
"""
import ctypes
import os

import torch  # noqa: F401,E402  (must be loaded before libyolov3_hip.so, see above)


_RUNTIME_DEFAULT_QUEUES = 4       # what HIP uses when the environment does not say


def hw_queues():
    """(hardware queues the HIP runtime maps this process's streams onto, whether that is certain).  HIP reads
    GPU_MAX_HW_QUEUES from the environment when it initialises; two streams that share a queue run one after the
    other (yolov3/pipeline.py warns, bench.py records it).  The package leaves the variable to the caller's environment: the
    hardware queues of a card are shared by every process on it."""
    try:
        return int(os.environ.get("GPU_MAX_HW_QUEUES") or _RUNTIME_DEFAULT_QUEUES), True
    except ValueError:
        return _RUNTIME_DEFAULT_QUEUES, False

_HERE = os.path.dirname(os.path.abspath(__file__))
# Y3_HIP_LIB: developer override (e.g. the diagnostic build with in-kernel phase stamps)
LIB_PATH = os.environ.get("Y3_HIP_LIB") or os.path.join(_HERE, "..", "lib", "libyolov3_hip.so")

Y3_F32, Y3_BF16, Y3_F16, Y3_F64 = 0, 1, 2, 3
OP_CONV, OP_MAXPOOL, OP_UPSAMPLE, OP_ADD, OP_COPY, OP_YOLO, OP_REORG = 1, 2, 3, 4, 5, 6, 7
OP_AVGPOOL, OP_SCALE_CHANNELS, OP_SAM = 8, 9, 10
F_LEAKY, F_RESIDUAL, F_OUT_F32, F_IN_NCHW_F32, F_IN_NHWC_U8BGR, F_PLAN_INPUT, F_FUSE_NEXT = 1, 2, 4, 8, 16, 32, 64
F_MISH, F_LOGISTIC, F_NEW_COORDS, F_POOL_DARKNET, F_SCORES_DARKNET, F_REORG_3D = 128, 256, 512, 1024, 2048, 4096
# y3_capabilities() bits: what the loaded library computes beyond ABI 6 as first released
CAP_MISH, CAP_SCALE_X_Y, CAP_LOGISTIC, CAP_NEW_COORDS, CAP_LETTERBOX, CAP_POOL_DARKNET = 1, 2, 4, 8, 16, 32
CAP_NMS_DARKNET, CAP_SCORES_DARKNET, CAP_MULTI_LABEL, CAP_PREPROCESS_DARKNET, CAP_REORG = 64, 128, 256, 512, 1024
CAP_LAUNCH_LOG = 2048
CAP_PLAN_OP_DIMS = 4096
CAP_TILES = 8192
CAP_GROUPED_CONV = 16384
CAP_ATTENTION = 32768
CAP_TILE_MERGE = 65536
# Darknet's suppression measures (include/yolov3_hip.h: Y3_NMS_*), by the cfg's spelling of `nms_kind`
NMS_IOU, NMS_GREEDY, NMS_DIOU = 0, 1, 2
NMS_KINDS = {"iou": NMS_IOU, "greedynms": NMS_GREEDY, "diounms": NMS_DIOU}
PATH_IGEMM, PATH_STEM, PATH_DIRECT, PATH_STEM_MFMA, PATH_GROUPED, PATH_DWISE = 0, 1, 2, 3, 4, 5


class _Y3OpGroups(ctypes.Union):
    """``groups`` of a conv op shares the four bytes of ``n_anchor``, which only YOLO ops read."""
    _fields_ = [("n_anchor", ctypes.c_int32), ("groups", ctypes.c_int32)]

    # four bytes with two names: compared by value, like the plain int32 field it replaces (code that walks Y3Op._fields_)
    def __eq__(self, other):
        return isinstance(other, _Y3OpGroups) and self.n_anchor == other.n_anchor

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash(self.n_anchor)

    def __repr__(self):
        return "n_anchor/groups={}".format(self.n_anchor)


class Y3Op(ctypes.Structure):
    """Mirror of ``struct y3_op`` (include/yolov3_hip.h)."""
    _anonymous_ = ("_groups",)
    _fields_ = [
        ("kind", ctypes.c_int32), ("dtype", ctypes.c_int32), ("flags", ctypes.c_uint32),
        ("batch", ctypes.c_int32),
        ("in_h", ctypes.c_int32), ("in_w", ctypes.c_int32), ("in_c", ctypes.c_int32), ("in_ld", ctypes.c_int32),
        ("out_h", ctypes.c_int32), ("out_w", ctypes.c_int32), ("out_c", ctypes.c_int32), ("out_ld", ctypes.c_int32),
        ("ksize", ctypes.c_int32), ("stride", ctypes.c_int32), ("pad", ctypes.c_int32),
        ("res_ld", ctypes.c_int32), ("k_ld", ctypes.c_int32), ("cout_pad", ctypes.c_int32),
        ("d_in", ctypes.c_void_p), ("d_out", ctypes.c_void_p), ("d_res", ctypes.c_void_p),
        ("d_weight", ctypes.c_void_p), ("d_scale", ctypes.c_void_p), ("d_bias", ctypes.c_void_p),
        ("_groups", _Y3OpGroups), ("n_attr", ctypes.c_int32),
        ("anchor_w", ctypes.c_float * 8), ("anchor_h", ctypes.c_float * 8),
        ("row_offset", ctypes.c_int32), ("rows_total", ctypes.c_int32),
        ("net_w", ctypes.c_float), ("net_h", ctypes.c_float),
        ("d_bbox", ctypes.c_void_p), ("d_prob", ctypes.c_void_p), ("d_cls", ctypes.c_void_p),
        ("block_idx", ctypes.c_int32), ("scale_x_y", ctypes.c_float),
        ("d_weight_frag", ctypes.c_void_p),
    ]


class Y3LetterboxFrame(ctypes.Structure):
    """Mirror of ``y3_letterbox_frame`` (include/yolov3_hip.h): one frame of a ``y3_letterbox_u8`` batch."""
    _fields_ = [("d_src", ctypes.c_void_p), ("src_h", ctypes.c_int32), ("src_w", ctypes.c_int32),
                ("d_ytab", ctypes.c_void_p), ("d_xtab", ctypes.c_void_p)]


class Y3Tile(ctypes.Structure):
    """Mirror of ``y3_tile`` (include/yolov3_hip.h): one net-sized window of a frame, for ``y3_tiles_u8``."""
    _fields_ = [("d_src", ctypes.c_void_p), ("src_h", ctypes.c_int32), ("src_w", ctypes.c_int32),
                ("y0", ctypes.c_int32), ("x0", ctypes.c_int32)]


class Y3TileGeom(ctypes.Structure):
    """Mirror of ``y3_tile_geom`` (include/yolov3_hip.h): scale and origin of one tile's boxes, for ``y3_detect_tiled``."""
    _fields_ = [("sx", ctypes.c_float), ("sy", ctypes.c_float), ("ox", ctypes.c_int32), ("oy", ctypes.c_int32)]


class Y3DarknetFrame(ctypes.Structure):
    """Mirror of ``y3_darknet_frame`` (include/yolov3_hip.h): one frame of a ``y3_preprocess_darknet_f32`` batch."""
    _fields_ = [("d_src", ctypes.c_void_p), ("src_h", ctypes.c_int32), ("src_w", ctypes.c_int32)]


class Y3HeadView(ctypes.Structure):
    """Mirror of ``y3_head_view`` (include/yolov3_hip.h): one detection head's float32 conv output as ``y3_expand_labels``
    reads it."""
    _fields_ = [("d_head", ctypes.c_void_p)] + [(name, ctypes.c_int32) for name in (
        "h", "w", "ld", "n_anchor", "n_attr", "row_offset", "new_coords")]


class Y3Options(ctypes.Structure):
    """Mirror of ``struct y3_options`` (include/yolov3_hip.h): kernel-selection options of one plan."""
    _fields_ = [(name, ctypes.c_int32) for name in (
        "auto_mask", "unused0", "igemm_version", "igemm_ns", "igemm_bm", "use_graph", "fuse_stem", "fuse_head",
        "fuse_spp", "decode_lanes", "fuse_block")] + [("reserved", ctypes.c_int32 * 5)]


# y3_options.auto_mask bits (include/yolov3_hip.h: Y3_AM_*)
AM_HALO_WIDE, AM_IGEMM3_MID, AM_HALO_NARROW, AM_IGEMM3_1X1_DEEP = 0x0001, 0x0002, 0x0004, 0x0008
AM_HALO_MID, AM_IGEMM3_NARROW, AM_IGEMM3_1X1_BM64, AM_PATCH_WIDE = 0x0010, 0x0020, 0x0040, 0x0080
AM_HALO_TILE256, AM_NO_BN_SHRINK, AM_NO_SMALL_GRID, AM_NO_WRES, AM_WRES_ALWAYS = 0x0200, 0x0400, 0x0800, 0x1000, 0x2000
AM_HALO_DW, AM_HALO_DW_ALWAYS = 0x4000, 0x8000                       # direct-weights strip kernel: where it pays / wherever it fits
AM_1X1_DW = 0x10000                                                  # direct-weights 1x1 kernel (short-K bottleneck layers, one tile per CU)
AM_SMALL_DW_ALWAYS = 0x40000                                         # tests / A-B: the small-grid kernel wherever its shape constraints hold
AM_SMALL_DW = 0x20000                                                # small-grid direct-weights kernel (48-pixel tiles, 1x1 and 3x3: one frame at a time)
AM_SMALL_DW_WIDE = 0x80000                                           # ... on grids a little over one round as well (3x3: 1.5 rounds; 1x1 with one channel tile: 8)
AM_DEFAULT = (AM_HALO_WIDE | AM_HALO_NARROW | AM_IGEMM3_1X1_DEEP | AM_HALO_MID | AM_PATCH_WIDE | AM_HALO_DW | AM_1X1_DW | AM_SMALL_DW |
              AM_SMALL_DW_WIDE)
AM_IGEMM_ONLY = 0
AM_HALO_ALL = AM_HALO_WIDE | AM_HALO_NARROW | AM_HALO_MID          # conv_bench: the halo kernel wherever it fits

ABI_VERSION = 6
_lib = None

# name -> (restype, argtypes); every symbol include/yolov3_hip.h declares
PROTOTYPES = {
    "y3_abi_version": (ctypes.c_int, []),
    "y3_capabilities": (ctypes.c_uint32, []),
    "y3_last_error": (ctypes.c_char_p, []),
    "y3_device_count": (ctypes.c_int, []),
    "y3_plan_create": (ctypes.c_int, [ctypes.POINTER(Y3Op), ctypes.c_int, ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_void_p)]),
    "y3_plan_create_ex": (ctypes.c_int, [ctypes.POINTER(Y3Op), ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(Y3Options),
                                         ctypes.POINTER(ctypes.c_void_p)]),
    "y3_options_default": (None, [ctypes.POINTER(Y3Options)]),
    "y3_plan_destroy": (None, [ctypes.c_void_p]),
    "y3_plan_run": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "y3_plan_run_timed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.POINTER(ctypes.c_float)]),
    "y3_plan_run_profiled": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_float)]),
    "y3_plan_op_kernel": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_int]),
    "y3_plan_op_dims": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]),
    "y3_plan_op_flops": (ctypes.c_double, [ctypes.c_void_p, ctypes.c_int]),
    "y3_plan_op_bytes": (ctypes.c_double, [ctypes.c_void_p, ctypes.c_int]),
    "y3_conv_path": (ctypes.c_int, [ctypes.POINTER(Y3Op)]),
    "y3_conv_fragment_weight_bytes": (ctypes.c_size_t, [ctypes.POINTER(Y3Op), ctypes.POINTER(Y3Options)]),
    "y3_conv_make_fragment_weights": (ctypes.c_int, [ctypes.POINTER(Y3Op), ctypes.c_void_p, ctypes.c_void_p]),
    "y3_set_tuning": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int]),
    "y3_debug_launch_log_begin": (ctypes.c_int, []),
    "y3_debug_launch_log_end": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
    "y3_op_run": (ctypes.c_int, [ctypes.POINTER(Y3Op), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "y3_detect_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "y3_detect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                 ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                                 ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "y3_detect_letterbox": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                                           ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "y3_detect_tiled_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "y3_detect_tiled": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p]),
    "y3_merge_tiled_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "y3_merge_tiled": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "y3_detect_darknet_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int]),
    "y3_detect_darknet": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_float, ctypes.c_double, ctypes.c_void_p,
                                         ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                         ctypes.c_float, ctypes.c_void_p]),
    "y3_nms_darknet_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "y3_nms_darknet": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_float,
                                      ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "y3_expand_labels_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "y3_expand_labels": (ctypes.c_int, [ctypes.POINTER(Y3HeadView), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_float, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "y3_nms_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "y3_nms": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                              ctypes.c_void_p]),
    "y3_cxywh_to_tlbr": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                        ctypes.c_void_p]),
    "y3_nms_float_workspace_bytes": (ctypes.c_size_t, [ctypes.c_int]),
    "y3_nms_float": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double,
                                    ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "y3_cxywh_to_tlbr_float": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                              ctypes.c_void_p]),
    "y3_resize_bilinear_u8": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                             ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "y3_letterbox_geometry": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int32)]),
    "y3_letterbox_u8": (ctypes.c_int, [ctypes.POINTER(Y3LetterboxFrame), ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "y3_tiles_u8": (ctypes.c_int, [ctypes.POINTER(Y3Tile), ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_void_p]),
    "y3_preprocess_darknet_f32": (ctypes.c_int, [ctypes.POINTER(Y3DarknetFrame), ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                                 ctypes.c_int, ctypes.c_int, ctypes.c_void_p]),
    "y3_copy_bytes": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "y3_pack_records": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
}


# symbols a library of ABI 6 built before they were added lacks: asked for through capabilities()
_OPTIONAL = ("y3_capabilities", "y3_detect_letterbox", "y3_letterbox_geometry", "y3_letterbox_u8",
             "y3_detect_darknet_workspace_bytes", "y3_detect_darknet", "y3_nms_darknet_workspace_bytes", "y3_nms_darknet",
             "y3_expand_labels_workspace_bytes", "y3_expand_labels", "y3_preprocess_darknet_f32",
             "y3_debug_launch_log_begin", "y3_debug_launch_log_end", "y3_plan_op_dims",
             "y3_tiles_u8", "y3_detect_tiled_workspace_bytes", "y3_detect_tiled",
             "y3_merge_tiled_workspace_bytes", "y3_merge_tiled")


class HipLibraryError(RuntimeError):
    pass


def lib():
    """Load (once) and return the shared library; raise if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.path.abspath(LIB_PATH)
    if not os.path.exists(path):
        raise HipLibraryError(
            "libyolov3_hip.so not found at {} -- build it with "
            "`make -C pytorch-yolov3_amd/csrc` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
            "This package has no CPU fallback.".format(path))
    try:
        handle = ctypes.CDLL(path)
    except OSError as exc:
        raise HipLibraryError("cannot load {}: {}".format(path, exc))
    for name, (restype, argtypes) in PROTOTYPES.items():
        if name in _OPTIONAL and not hasattr(handle, name):
            continue
        fn = getattr(handle, name)
        fn.restype = restype
        fn.argtypes = argtypes
    if handle.y3_abi_version() != ABI_VERSION:
        raise HipLibraryError("libyolov3_hip.so ABI version {} != {} (rebuild: make -C pytorch-yolov3_amd/csrc)".format(
            handle.y3_abi_version(), ABI_VERSION))
    _lib = handle
    return _lib


def capabilities():
    """CAP_* bits of the loaded library (0 from a library older than y3_capabilities)."""
    handle = lib()
    return int(handle.y3_capabilities()) if hasattr(handle, "y3_capabilities") else 0


def require_capabilities(needs, what):
    """Refuse a plan that needs a computation the loaded library does not report: a stale library would run mish as
    linear, ignore scale_x_y, run a logistic head as linear, decode new_coords heads the YOLOv3 way, stretch frames
    that were to be letterboxed, pool the reference's way where Darknet's rule was asked for, suppress by the
    reference's rule where Darknet's was asked for, score boxes by the reference's soft-max where Darknet's logistic scores
    were asked for, lack the multi-label expansion, lack Darknet's float preprocessing, reject a [reorg] op as of unknown kind,
    lack the tile cutter and the tiled detection tail, run a grouped conv as a dense one, or reject an [avgpool], [scale_channels]
    or [sam] op as of unknown kind, or lack the seam merge of tiled inference."""
    missing = needs & ~capabilities()
    if missing:
        names = [n for n, b in (("mish", CAP_MISH), ("scale_x_y", CAP_SCALE_X_Y), ("logistic", CAP_LOGISTIC),
                                ("new_coords", CAP_NEW_COORDS), ("letterbox", CAP_LETTERBOX),
                                ("Darknet max-pooling", CAP_POOL_DARKNET), ("Darknet NMS", CAP_NMS_DARKNET),
                                ("Darknet class scores", CAP_SCORES_DARKNET),
                                ("multi-label detections", CAP_MULTI_LABEL),
                                ("Darknet preprocessing", CAP_PREPROCESS_DARKNET), ("reorg", CAP_REORG),
                                ("tiled inference", CAP_TILES), ("grouped convolution", CAP_GROUPED_CONV),
                                ("attention blocks", CAP_ATTENTION), ("tile seam merging", CAP_TILE_MERGE)) if missing & b]
        raise HipLibraryError("{}: the loaded libyolov3_hip.so cannot compute {} (rebuild: make -C pytorch-yolov3_amd/csrc)"
                              .format(what, ", ".join(names)))


SCORE_MODES = ("reference", "darknet")


def check_scores_mode(scores):
    """``scores`` of ``Darknet(...)``: "reference" (soft-max over the class logits, the reference's) or "darknet" (an
    independent logistic per class, what Darknet computes); ValueError for anything else.  Needs no GPU."""
    if scores not in SCORE_MODES:
        raise ValueError("scores {!r}: this package computes {}".format(scores, " and ".join(repr(m) for m in SCORE_MODES)))
    return scores


PREPROCESS_MODES = (None, "darknet")


def check_preprocess_mode(preprocess):
    """``preprocess`` of the detection entry points: None (uint8 frames resized with OpenCV's 8-bit bilinear, the default) or
    "darknet" (Darknet's float ``resize_image`` / ``letterbox_image``: ``y3_preprocess_darknet_f32``); ValueError for
    anything else.  Needs no GPU."""
    if preprocess is not None and not (isinstance(preprocess, str) and preprocess == "darknet"):
        raise ValueError("preprocess {!r}: this package computes None (the default 8-bit resize) and 'darknet'".format(preprocess))
    return preprocess


def nms_mode(nms_kind, beta_nms=0.6):
    """(Y3_NMS_* code, beta as a float32-exact Python float) of a Darknet suppression mode, or None for ``nms_kind=None``
    (the reference's rule).  ValueError for a kind this package does not compute (``cornersnms`` ...) or a ``beta_nms``
    that is not finite and > 0.  Needs no GPU."""
    if nms_kind is None:
        return None
    if not isinstance(nms_kind, str) or nms_kind not in NMS_KINDS:
        raise ValueError("nms_kind {!r}: this package computes {} (None = the reference's rule on integer pixel boxes)".format(
            nms_kind, ", ".join(sorted(NMS_KINDS))))
    beta = ctypes.c_float(float(beta_nms)).value
    if not (beta > 0.0 and beta != float("inf")):
        raise ValueError("beta_nms must be finite and > 0 (as float32), got {!r}".format(beta_nms))
    return NMS_KINDS[nms_kind], beta


class launch_log:
    """``with launch_log() as log:`` records the code-object symbol name of every kernel this thread launches through the
    library inside the block (``y3_debug_launch_log_begin`` / ``_end``); afterwards ``log.names`` is the list in launch order
    and ``log.symbols`` the sorted set.  Tests and tools only."""

    def __init__(self):
        self.names, self.symbols = [], []

    def __enter__(self):
        if not capabilities() & CAP_LAUNCH_LOG:
            raise HipLibraryError("the loaded libyolov3_hip.so has no launch log (rebuild: make -C pytorch-yolov3_amd/csrc)")
        check(lib().y3_debug_launch_log_begin())
        return self

    def __exit__(self, *exc):
        handle = lib()
        need = ctypes.c_size_t(0)
        handle.y3_debug_launch_log_end(None, 0, ctypes.byref(need))          # the size query: fails by design, fills `need`
        buf = ctypes.create_string_buffer(need.value)
        rc = handle.y3_debug_launch_log_end(buf, need.value, None)
        self.names = buf.value.decode().split()
        self.symbols = sorted(set(self.names))
        if exc[0] is None:
            check(rc)
        return False


class device_cus:
    """``with device_cus(n):`` every plan created inside the block is made for a device of ``n`` compute units
    (``y3_set_tuning("device_cus", n)``: the plans a DPX / QPX / CPX compute partition of 128 / 64 / 32 CUs gets), whatever the
    device reports; the key is back at 0 -- ask the device -- when the block ends, an exception included.  A plan keeps what it
    was created with; ``Darknet`` caches plans by shape, so a network built outside the block is not re-planned inside it.
    Tests and tools only."""

    def __init__(self, n):
        self.n = int(n)

    def __enter__(self):
        if not capabilities() & CAP_PLAN_OP_DIMS:
            raise HipLibraryError("the loaded libyolov3_hip.so has no device_cus key (rebuild: make -C pytorch-yolov3_amd/csrc)")
        check(lib().y3_set_tuning(b"device_cus", self.n))
        return self

    def __exit__(self, *exc):
        lib().y3_set_tuning(b"device_cus", 0)
        return False


class grouped_generic:
    """``with grouped_generic():`` every grouped conv laid out and planned inside the block runs ``conv_grouped_*``
    (``y3_set_tuning("grouped_generic", 1)``: ``y3_conv_path`` answers 4 for it), the depthwise ones included; the key is back at
    what it was before when the block ends.  Weights are laid out by the path the library answers, so a network must compile its plans inside
    the block it is to run under.  Same bits either way: tests and A/B runs only."""

    current = 0          # the key's value as this class last set it (the library has no getter; nothing else in the package sets it)

    def __init__(self, on=True):
        self.on = int(bool(on))

    def __enter__(self):
        if not capabilities() & CAP_GROUPED_CONV:
            raise HipLibraryError("the loaded libyolov3_hip.so has no grouped convolution (rebuild: make -C pytorch-yolov3_amd/csrc)")
        self.before = grouped_generic.current
        check(lib().y3_set_tuning(b"grouped_generic", self.on))
        grouped_generic.current = self.on
        return self

    def __exit__(self, *exc):
        lib().y3_set_tuning(b"grouped_generic", self.before)      # (what it was: a nested block leaves the outer one's value)
        grouped_generic.current = self.before
        return False


def plan_op_dims(handle, op_index):
    """(workgroups, threads per workgroup, dynamic LDS bytes) that op ``op_index`` of plan ``handle`` launches, as recorded at plan
    creation; (0, 0, 0) for an op that an earlier step launches."""
    out = (ctypes.c_int64 * 3)()
    check(lib().y3_plan_op_dims(handle, op_index, out))
    return int(out[0]), int(out[1]), int(out[2])


def options(**overrides):
    """The library's default plan options (as modified by ``y3_set_tuning``) with ``overrides`` applied."""
    opt = Y3Options()
    lib().y3_options_default(ctypes.byref(opt))
    for key, val in overrides.items():
        if key not in dict(Y3Options._fields_) or key in ("reserved", "unused0"):
            raise KeyError("unknown plan option {!r}".format(key))
        setattr(opt, key, int(val))
    return opt


def check(rc):
    if rc != 0:
        msg = lib().y3_last_error()
        raise RuntimeError("libyolov3_hip: {} (code {})".format(msg.decode() if msg else "unknown error", rc))


def require_gpu():
    """Raise unless a gfx950 GPU is usable by both torch and the library."""
    if not torch.cuda.is_available():
        raise RuntimeError(
            "no HIP device visible to torch: this package runs its hot path only on MI355X (gfx950); "
            "there is no CPU fallback")
    if lib().y3_device_count() < 1:
        raise RuntimeError("libyolov3_hip: no gfx950 device found")


def stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(s.cuda_stream)
