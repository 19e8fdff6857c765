"""A plan description (yolov3/plan.py: ``build_plan``) as the C ABI's ``y3_op`` structs (include/yolov3_hip.h).

``fill_ops`` is the one translation: shapes, flags, padded weight sizes, anchors, ``scale_x_y`` and the library capabilities
the ops rely on.  It touches no device: every address comes from the ``mem`` object the caller hands it.  ``Darknet`` passes
one backed by tensors, the host tests one that deals fake addresses, so what the tests plan is what the product runs.
"""
import ctypes

from . import _hip

# storage modes: name -> (C ABI element type, bytes per element)
STORAGE = {"float32": (_hip.Y3_F32, 4), "bf16": (_hip.Y3_BF16, 2), "fp16": (_hip.Y3_F16, 2)}


# plan op kinds of the attention blocks -> C ABI op kinds
ATTENTION_OPS = {"avgpool": _hip.OP_AVGPOOL, "scale_channels": _hip.OP_SCALE_CHANNELS, "sam": _hip.OP_SAM}


def _round_up(v, m):
    return (v + m - 1) // m * m


def padded_weight_dims(path, cout, cin, k, es, groups=1):
    """``(cout_pad, k_ld)`` of a conv's device weights in the layout of kernel family ``path`` (``y3_conv_path``), elements of
    ``es`` bytes: the 32 x 32 block of the MFMA stem, the stem's [K][cout rounded to 8], or rows of K rounded to 128 bytes
    under cout rounded to 128.  A grouped conv (``cin`` input channels in all, ``groups`` of them): rows of the group's
    K = k * k * cin / groups rounded to 8 elements under cout rounded to 8; a depthwise one k * k rows of cout rounded to 8."""
    if path == _hip.PATH_DWISE:
        return _round_up(cout, 8), _round_up(cout, 8)
    if path == _hip.PATH_GROUPED:
        return _round_up(cout, 8), _round_up(k * k * (cin // groups), 8)
    if path == _hip.PATH_STEM_MFMA:
        return 32, 32
    if path == _hip.PATH_STEM:
        return _round_up(cout, 8), _round_up(cout, 8)
    return _round_up(cout, 128), _round_up(k * k * cin, 128 // es)


def multi_label_options(options, multi_label):
    """The plan options (a dict or None) a network compiles with: a multi-label one with ``fuse_head=0``, because the head
    convs' float32 outputs must reach memory and the fused head kernels keep them in LDS."""
    return dict(options or {}, fuse_head=0) if multi_label else options


def fill_maxpool_op(op, od):
    """Kind, size, stride and pooling rule of a plan's maxpool op dict into the C ABI's ``y3_op``; returns the library
    capabilities the op relies on.  Darknet's rule (``od["pool"] == "darknet"``) travels as Y3_F_POOL_DARKNET with the
    cfg's ``padding`` in ``pad``; the default sets neither."""
    op.kind = _hip.OP_MAXPOOL
    op.ksize, op.stride = od["ksize"], od["stride"]
    if od.get("pool") == "darknet":
        op.flags |= _hip.F_POOL_DARKNET
        op.pad = od["pad"]
        return _hip.CAP_POOL_DARKNET
    return 0


def yolo_decode_flags(od, scores):
    """(y3_op.flags bits, library capabilities) of a plan's yolo op dict under the class scoring ``scores``.  A new_coords
    head scores the Darknet way already, so it is the same op in both modes; any other head carries Y3_F_SCORES_DARKNET
    under "darknet".  A [region] head (YOLOv2, softmax=1) is the default decode in both modes as well."""
    if od.get("new_coords"):
        return _hip.F_NEW_COORDS, _hip.CAP_NEW_COORDS
    if od.get("region"):
        return 0, 0          # a [region] head with softmax=1: Darknet's rule for it IS the soft-max, in both modes
    if scores == "darknet":
        return _hip.F_SCORES_DARKNET, _hip.CAP_SCORES_DARKNET
    return 0, 0


def fill_ops(desc, net_info, convs, dtype, batch, input_mode, scores, opt, mem):
    """The ops of the plan description ``desc`` (``build_plan`` of the same ``batch`` and of ``dtype``'s element size) for a
    network whose conv layout is ``convs`` (weights.conv_layout), fed ``input_mode`` ("u8" frames or "f32" tensors), scoring
    classes by ``scores``, under the plan options ``opt`` (a ``Y3Options`` or None for the library's defaults).

    ``mem`` gives every address, and nothing else is asked for one:
        ``arena(nbytes) -> base address`` of the activations;
        ``conv(slot, path) -> (d_weight, d_scale, d_bias)`` of conv ``slot`` in the layout of kernel family ``path``;
        ``fragment(slot, op, nbytes) -> address`` of its fragment-order weights (``op`` is complete but for that address);
        ``outputs(batch, rows_total) -> (d_bbox, d_prob, d_cls)``, shared by every YOLO op.

    Returns (the ``y3_op`` array, the ``y3_capabilities`` bits the plan needs, per op the fragment-weight bytes of a conv and
    None for any other op)."""
    lib = _hip.lib()
    c_dtype, es = STORAGE[dtype]
    base = mem.arena(desc["arena_bytes"])
    bbox, prob, cls = mem.outputs(batch, desc["rows_total"])
    p_opt = ctypes.byref(opt) if opt is not None else None

    def addr(t, elem):
        return base + desc["offsets"][t.buf] + t.off * elem

    ops = (_hip.Y3Op * len(desc["ops"]))()
    needs = _hip.CAP_MULTI_LABEL if desc["keep_heads"] else 0
    frag = []
    for op, od in zip(ops, desc["ops"]):
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
            if od.get("mish"):
                op.flags |= _hip.F_MISH
                needs |= _hip.CAP_MISH
            if od.get("logistic"):
                op.flags |= _hip.F_LOGISTIC
                needs |= _hip.CAP_LOGISTIC
            if od.get("fuse_next"):
                op.flags |= _hip.F_FUSE_NEXT
            if res is not None:
                op.flags |= _hip.F_RESIDUAL
            c = convs[od["slot"]]
            groups = int(od.get("groups", 1))
            if groups > 1:
                op.groups = groups
                needs |= _hip.CAP_GROUPED_CONV
            # provisional padded sizes so that y3_conv_path can judge the shape
            op.cout_pad, op.k_ld = padded_weight_dims(_hip.PATH_IGEMM, c["cout"], c["cin"], c["k"], es)
            path = lib.y3_conv_path(ctypes.byref(op))     # (does not depend on the plan options)
            op.cout_pad, op.k_ld = padded_weight_dims(path, c["cout"], c["cin"], c["k"], es, groups)
            op.d_weight, op.d_scale, op.d_bias = mem.conv(od["slot"], path)
            nfrag = int(lib.y3_conv_fragment_weight_bytes(ctypes.byref(op), p_opt))
            if nfrag:
                op.d_weight_frag = mem.fragment(od["slot"], op, nfrag)
        elif kind == "maxpool":
            needs |= fill_maxpool_op(op, od)
        elif kind == "upsample":
            op.kind = _hip.OP_UPSAMPLE
            op.ksize, op.stride = 1, od["stride"]
        elif kind in ("add", "copy"):
            op.kind = _hip.OP_ADD if kind == "add" else _hip.OP_COPY
            op.ksize = op.stride = 1
        elif kind == "reorg":
            op.kind = _hip.OP_REORG
            op.ksize, op.stride = 1, od["stride"]
            if od.get("form3d"):
                op.flags |= _hip.F_REORG_3D
            needs |= _hip.CAP_REORG
        elif kind in ATTENTION_OPS:
            # prev in d_in / in_*, src in d_res / res_ld (filled above), no flags; a stale library would not know the kinds
            op.kind = ATTENTION_OPS[kind]
            op.ksize = op.stride = 1
            needs |= _hip.CAP_ATTENTION
        elif kind == "yolo":
            op.kind = _hip.OP_YOLO
            op.n_anchor = len(od["anchors"])
            op.n_attr = od["n_attr"]
            for a, (aw, ah) in enumerate(od["anchors"]):
                op.anchor_w[a] = float(aw)
                op.anchor_h[a] = float(ah)
            op.row_offset, op.rows_total = od["row_offset"], od["rows_total"]
            op.net_w, op.net_h = float(net_info["width"]), float(net_info["height"])
            if "scale_x_y" in od:
                op.scale_x_y = od["scale_x_y"]
                needs |= _hip.CAP_SCALE_X_Y
            flags, caps = yolo_decode_flags(od, scores)
            op.flags |= flags
            needs |= caps
            # persistent output buffers: every head's decode kernel writes its row range in place
            op.d_bbox, op.d_prob, op.d_cls = bbox, prob, cls
        else:
            raise AssertionError(kind)
        frag.append(nfrag)
    return ops, needs, frag


def head_views(ops):
    """The detection heads' float32 conv outputs, as filled ``ops`` address them: a ``y3_head_view`` array in YOLO-op order
    for ``y3_expand_labels``.  Meaningful for a plan built with ``keep_heads`` only; others reuse those tensors."""
    yolo = [op for op in ops if op.kind == _hip.OP_YOLO]
    heads = (_hip.Y3HeadView * len(yolo))()
    for view, op in zip(heads, yolo):
        view.d_head, view.h, view.w, view.ld = op.d_in, op.in_h, op.in_w, op.in_ld
        view.n_anchor, view.n_attr, view.row_offset = op.n_anchor, op.n_attr, op.row_offset
        view.new_coords = int(bool(op.flags & _hip.F_NEW_COORDS))
    return heads
