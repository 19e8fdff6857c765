"""Layer-plan compiler: Darknet blocks -> flat list of device ops + buffer arena.

Replaces the reference's ``blocks2modules`` / ``forward`` dispatch
(/root/reference/yolov3/darknet.py:218-315, :351-405).  The reference executes
one nn.Module per block and materialises every route (``torch.cat``) and
shortcut (``+``) as a new tensor.  Here the graph is resolved once, on the host:

* shortcut   -> residual input of the preceding conv's epilogue (no add pass);
* route [a]  -> alias of block a's tensor (no copy);
* route [a,b,..] -> one concat buffer; producers a, b, .. write straight into
  their channel slice (pixel stride = total channels), so no concat pass;
* yolo heads -> decode kernels write into row ranges of the final (B, M, .)
  outputs, so no head concat and no w,h rescale pass;
* every other tensor lives in an arena whose slots are reused as soon as their
  last reader has run (keeps the working set small enough to stay in the
  256 MiB Infinity Cache for the deeper stages).

Pure Python, no GPU needed: unit-tested on CPU.
"""
import ctypes

ALIGN = 256          # bytes, arena slot alignment
CH_ALIGN = 8         # channel-slice / pixel-stride granularity (elements): 16 B for bf16


def _round_up(v, m):
    return (v + m - 1) // m * m


class Tensor(object):
    """A (B,H,W,C) NHWC view: channels [off, off+c) of buffer `buf` with pixel stride `ld`."""
    __slots__ = ("buf", "off", "ld", "c", "h", "w", "f32")

    def __init__(self, buf, off, ld, c, h, w, f32=False):
        self.buf, self.off, self.ld, self.c, self.h, self.w, self.f32 = buf, off, ld, c, h, w, f32

    def __repr__(self):
        return "T(buf={} off={} ld={} c={} {}x{}{})".format(
            self.buf, self.off, self.ld, self.c, self.h, self.w, " f32" if self.f32 else "")


ACTIVATIONS = ("leaky", "linear", "mish", "logistic")
# max-pool semantics: "reference" (stride 1: window [y, y+k), out-of-range taps count as 0.0; else unpadded) or "darknet"
# (window origin o * stride - padding / 2, out-of-range taps ignored: ``maxpool_geometry``)
POOL_MODES = ("reference", "darknet")


def check_pool_mode(pool):
    if pool not in POOL_MODES:
        raise ValueError("pool={!r}: expected one of {}".format(pool, ", ".join(repr(m) for m in POOL_MODES)))
    return pool


def maxpool_geometry(i, blk, h, w, pool):
    """(out_h, out_w, padding) of [maxpool] block ``i`` on an (h, w) map.  "reference": stride 1 keeps the size, other strides
    pool unpadded, floor mode; padding is 0 (unused).  "darknet": padding = the cfg's ``padding`` key (Darknet's default:
    size - 1), out = (in + padding - size) // stride + 1; a block one of whose windows would hold no tap is refused."""
    k, s = blk["size"], blk["stride"]
    if pool != "darknet":
        if k > 1 and s == 1:
            return h, w, 0
        return (h - k) // s + 1, (w - k) // s + 1, 0
    p = int(blk.get("padding", k - 1))
    if p < 0 or h + p < k or w + p < k:
        raise ValueError("maxpool block {}: size={} padding={} does not fit a {}x{} map".format(i, k, p, h, w))
    oh, ow = (h + p - k) // s + 1, (w + p - k) // s + 1
    # the first window ends at k - 1 - p // 2, the last one starts at (out - 1) * s - p // 2
    if p // 2 >= k or (oh - 1) * s - p // 2 >= h or (ow - 1) * s - p // 2 >= w:
        raise ValueError("maxpool block {}: padding={} leaves a window of size={} without a tap inside the {}x{} map".format(
            i, p, k, h, w))
    return oh, ow, p


def route_groups(blk):
    """(groups, group_id) of a [route] block: Darknet's grouped route takes channel group `group_id` of `groups` equal
    parts of its input (yolov4-tiny's CSP blocks)."""
    return int(blk.get("groups", 1)), int(blk.get("group_id", 0))


REORG_KINDS = ("reorg", "reorg3d")
HEAD_KINDS = ("yolo", "region")
# Darknet's attention blocks.  [avgpool]: global average pool, (C, H, W) -> (C, 1, 1).  [scale_channels] from=J: block J's output
# times the (C, 1, 1) output of the block in front, channel by channel (a squeeze-and-excite unit's last step).  [sam] from=J: block
# J's output times the output of the block in front, element by element.  `from` is read as a [shortcut]'s is: relative to the block.
ATTENTION_KINDS = ("avgpool", "scale_channels", "sam")
MAX_ANCHORS = 8      # y3_op.anchor_w[8]


def _f32(v):
    """the float32 nearest to ``v`` (one rounding), as a Python float"""
    return ctypes.c_float(v).value


def region_anchors(blk, net_info, grid_h, grid_w):
    """The pixel anchors of a [region] block's decode on a grid_h x grid_w map.  Region anchors are in grid cells; the decode op
    takes pixels of the cfg's net size and divides by it again, so ``a * net_w / grid_w`` (float64, rounded once to float32)
    makes its ``exp(tw) * anchor / net_w`` Darknet's ``exp(tw) * a / grid_w``."""
    num = int(blk.get("num", 1))
    return [(_f32(float(aw) * net_info["width"] / grid_w), _f32(float(ah) * net_info["height"] / grid_h))
            for aw, ah in blk["anchors"][:num]]


def check_region(blocks, i):
    """Refuse, naming block and key, a [region] head the decode kernels would not score as Darknet does."""
    blk = blocks[i]
    for key in ("softmax_tree", "tree"):
        if key in blk:
            raise ValueError("region block {}: {} (a class hierarchy, YOLO9000) is not supported".format(i, key))
    if int(blk.get("softmax", 0)) != 1:
        raise ValueError("region block {}: softmax={} is not supported (softmax=1 only: sigmoid(obj) * softmax(classes))".format(
            i, blk.get("softmax", 0)))
    if int(blk.get("coords", 4)) != 4:
        raise ValueError("region block {}: coords={} is not supported (4 only)".format(i, blk["coords"]))
    num, classes = int(blk.get("num", 1)), int(blk.get("classes", 20))
    if not 1 <= num <= MAX_ANCHORS:
        raise ValueError("region block {}: num={} anchors per cell (1..{} only)".format(i, num, MAX_ANCHORS))
    if classes < 1:
        raise ValueError("region block {}: classes={}".format(i, classes))
    anchors = blk.get("anchors")
    if not isinstance(anchors, list) or len(anchors) < num or any(not isinstance(a, list) or len(a) != 2 for a in anchors[:num]):
        raise ValueError("region block {}: anchors does not hold num={} (w, h) pairs".format(i, num))
    head = blocks[i - 1] if i > 0 else {}
    if head.get("type") != "convolutional" or head.get("filters") != num * (5 + classes):
        raise ValueError("region block {}: the conv before it must have filters = num * (5 + classes) = {} (block {} is {} "
                         "filters={})".format(i, num * (5 + classes), i - 1, head.get("type"), head.get("filters")))


def check_grouped_conv(blocks, i, cin):
    """Refuse, naming block and numbers, a ``groups=`` on conv block ``i`` (``cin`` input channels) that the grouped kernels do
    not compute.  Called where the channel count is known: by ``infer_shapes`` for every plan and by ``Darknet`` on the
    descriptors of ``weights.conv_layout``."""
    blk = blocks[i]
    groups = int(blk.get("groups", 1))
    if groups == 1:
        return
    if groups < 1:
        raise ValueError("conv block {}: grouped convolution with groups={} (at least 1)".format(i, groups))
    if i == 0:
        raise ValueError("conv block {}: grouped convolution (groups={}) is not supported on the conv that reads the network "
                         "input".format(i, groups))
    filters = int(blk["filters"])
    if cin % groups or filters % groups:
        raise ValueError("conv block {}: grouped convolution: groups={} does not divide {} input channels and filters={}".format(
            i, groups, cin, filters))
    if i + 1 < len(blocks) and blocks[i + 1]["type"] in HEAD_KINDS:
        raise ValueError("conv block {}: grouped convolution (groups={}) is not supported directly in front of {} block {} (a "
                         "detection-head conv)".format(i, groups, blocks[i + 1]["type"], i + 1))


def check_blocks(blocks):
    """Refuse, naming the block, what the kernels cannot compute: any of it would otherwise run with different semantics
    and return wrong boxes without an error."""
    for i, blk in enumerate(blocks):
        kind = blk["type"]
        if kind == "convolutional":
            act = blk.get("activation")
            if act not in ACTIVATIONS:
                raise ValueError("conv block {}: activation {!r} is not supported (only {})".format(
                    i, act, ", ".join(ACTIVATIONS)))
            if int(blk.get("dilation", 1)) != 1:
                raise ValueError("conv block {}: dilated convolution (dilation={}) is not supported".format(
                    i, blk["dilation"]))
        elif kind == "maxpool":
            # Darknet's other pools; the kernels compute the spatial k x k pool with one stride only
            if int(blk.get("maxpool_depth", 0)) != 0:
                raise ValueError("maxpool block {}: maxpool_depth={} (pooling over channels) is not supported".format(
                    i, blk["maxpool_depth"]))
            if int(blk.get("antialiasing", 0)) != 0:
                raise ValueError("maxpool block {}: antialiasing={} is not supported".format(i, blk["antialiasing"]))
            for key in ("stride_x", "stride_y"):
                if key in blk and blk[key] != blk.get("stride", 1):
                    raise ValueError("maxpool block {}: {}={} differs from stride={} (one stride for both axes only)".format(
                        i, key, blk[key], blk.get("stride", 1)))
        elif kind == "route":
            groups, gid = route_groups(blk)
            if groups != 1 and len(blk["layers"]) != 1:
                raise ValueError("route block {}: groups={} is supported on single-layer routes only".format(i, groups))
            if groups < 1 or not 0 <= gid < groups:
                raise ValueError("route block {}: group_id={} out of range for groups={}".format(i, gid, groups))
        elif kind == "yolo":
            if int(blk.get("new_coords", 0)) != 0:
                # Darknet's new_coords decode reads probabilities (no exp, no sigmoid): the conv in front of the block must
                # end in a sigmoid, or the boxes would come out up to 4 * anchor * t^2 wide without an error
                head = blocks[i - 1] if i > 0 else {}
                if head.get("type") != "convolutional" or head.get("activation") != "logistic":
                    raise ValueError("yolo block {}: new_coords=1 is supported only behind a conv with activation=logistic "
                                     "(block {} is {} {!r})".format(i, i - 1, head.get("type"), head.get("activation")))
        elif kind in REORG_KINDS:
            # [reorg] is Darknet's original (flat) layer, [reorg3d] the space-to-depth of later Darknet; the kernels compute
            # the forward direction of either only
            if int(blk.get("reverse", 0)) != 0:
                raise ValueError("{} block {}: reverse={} is not supported".format(kind, i, blk["reverse"]))
            for key in ("flatten", "extra"):
                if int(blk.get(key, 0)) != 0:
                    raise ValueError("{} block {}: {}={} is not supported".format(kind, i, key, blk[key]))
            if int(blk.get("stride", 1)) < 1:
                raise ValueError("{} block {}: stride={}".format(kind, i, blk["stride"]))
        elif kind == "region":
            check_region(blocks, i)
        elif kind == "shortcut":
            if "weights_type" in blk:
                raise ValueError("shortcut block {}: weighted shortcuts (weights_type) are not supported".format(i))
            if blk.get("activation", "linear") != "linear":
                raise ValueError("shortcut block {}: activation {!r} is not supported (linear only)".format(
                    i, blk["activation"]))
        elif kind in ATTENTION_KINDS:
            if i == 0:
                raise ValueError("{} block 0: only a conv reads the network input (the first block must be "
                                 "[convolutional])".format(kind))
            if kind == "avgpool":
                continue                           # (it takes no parameters)
            if int(blk.get("scale_wh", 0)) != 0:
                raise ValueError("{} block {}: scale_wh={} is not supported".format(kind, i, blk["scale_wh"]))
            if blk.get("activation", "linear") != "linear":
                raise ValueError("{} block {}: activation {!r} is not supported (linear only)".format(
                    kind, i, blk["activation"]))
            if not isinstance(blk.get("from"), int) or not 0 <= i + blk["from"] < i:
                raise ValueError("{} block {}: from={!r} does not name an earlier block".format(kind, i, blk.get("from")))


def check_head_readers(blocks, readers, elem_size):
    """Refuse, naming both blocks, a graph that reads a detection head in a form nothing here computes.  ``readers[i]``: the
    (consumer block, role) pairs of block i's output.

    * Any reader of a [yolo] / [region] block's output, in every storage mode: in Darknet that is the activated tensor; the
      decode kernels write boxes only, and the planner's alias of the block would hand the reader the raw logits.
    * In the 16-bit modes (``elem_size != 4``) the logits of a head conv are float32 and, with the head fused into the decode
      kernel, never reach memory; every other tensor is 16-bit.  So a second reader of a head conv (a route, a shortcut's
      ``from``) would misread them, and a head behind anything but a conv would decode 16-bit elements as float32, past the
      end of their buffer."""
    kinds = [b["type"] for b in blocks]
    for i, kind in enumerate(kinds):
        if kind not in HEAD_KINDS:
            continue
        for r, _ in readers[i]:
            raise ValueError("{} block {}: block {} ({}) reads its output: the activated output of a detection head is not "
                             "computed (only its boxes are)".format(kind, i, r, kinds[r]))
        if elem_size == 4 or i == 0:
            continue
        if kinds[i - 1] != "convolutional":
            raise ValueError("{} block {}: block {} in front of it is a [{}], not a conv: in the 16-bit modes the decode reads "
                             "float32 logits, which only a conv directly in front of the head stores (float32 runs this "
                             "graph)".format(kind, i, i - 1, kinds[i - 1]))
        for r, _ in readers[i - 1]:
            if r != i:
                raise ValueError("conv block {}: block {} ({}) reads the logits of the head conv of {} block {}: in the 16-bit "
                                 "modes they are float32 and may never reach memory (float32 runs this graph)".format(
                                     i - 1, r, kinds[r], kind, i))


def infer_shapes(blocks, net_info, height, width, pool="reference"):
    """(C,H,W) of every block output for an input of size (height,width); conv arithmetic
    as torch.nn.Conv2d / MaxPool2d / Upsample compute it, max-pools by Darknet's size formula with ``pool="darknet"``."""
    check_blocks(blocks)
    check_pool_mode(pool)
    shapes = []
    c, h, w = net_info["channels"], height, width
    for i, blk in enumerate(blocks):
        kind = blk["type"]
        if kind == "convolutional":
            check_grouped_conv(blocks, i, c)       # (groups= against the input channel count, known here)
            k, s = blk["size"], blk["stride"]
            pad = (k - 1) // 2 if "pad" in blk else 0
            h = (h + 2 * pad - k) // s + 1
            w = (w + 2 * pad - k) // s + 1
            c = blk["filters"]
        elif kind == "maxpool":
            h, w, _ = maxpool_geometry(i, blk, h, w, pool)
        elif kind == "upsample":
            h, w = h * blk["stride"], w * blk["stride"]
        elif kind == "route":
            srcs = [shapes[j] for j in blk["layers"]]
            if any((s_[1], s_[2]) != (srcs[0][1], srcs[0][2]) for s_ in srcs):
                raise ValueError("route block {} joins tensors of different sizes: {}".format(i, srcs))
            c, h, w = sum(s_[0] for s_ in srcs), srcs[0][1], srcs[0][2]
            groups = route_groups(blk)[0]
            if c % groups:
                raise ValueError("route block {}: {} channels do not split into {} groups".format(i, c, groups))
            c //= groups
        elif kind == "shortcut":
            a, b = shapes[i - 1], shapes[i + blk["from"]]
            if a != b:
                raise ValueError("shortcut block {} adds {} and {}".format(i, a, b))
            c, h, w = a
        elif kind in REORG_KINDS:
            s = int(blk.get("stride", 1))
            if h % s or w % s:
                raise ValueError("{} block {}: stride={} does not divide the {}x{} map".format(kind, i, s, h, w))
            if kind == "reorg" and c % (s * s):
                raise ValueError("reorg block {}: {} channels are not a multiple of stride*stride = {}".format(i, c, s * s))
            c, h, w = c * s * s, h // s, w // s
        elif kind == "avgpool":
            h, w = 1, 1
        elif kind in ("scale_channels", "sam"):
            prev, src = shapes[i - 1], shapes[i + blk["from"]]
            if kind == "scale_channels" and prev != (src[0], 1, 1):
                raise ValueError("scale_channels block {} scales {} by {}: the scales must be ({}, 1, 1)".format(
                    i, src, prev, src[0]))
            if kind == "sam" and prev != src:
                raise ValueError("sam block {} multiplies {} by {}".format(i, src, prev))
            c, h, w = src
        elif kind in HEAD_KINDS or kind == "dropout":
            pass                                   # ([dropout]: Darknet skips it at inference; its keys are read and ignored)
        else:
            raise ValueError("unsupported block type {!r} (block {})".format(kind, i))
        if h <= 0 or w <= 0:
            raise ValueError("block {} produces an empty tensor".format(i))
        shapes.append((c, h, w))
    return shapes


def build_plan(blocks, net_info, batch, height, width, elem_size, reuse=True, fuse=None, pool="reference", keep_heads=False):
    """Resolve the graph.  ``blocks`` must already carry absolute route indices.

    Returns dict(ops=[...], buffers={id: nbytes}, offsets={id: arena offset}, arena_bytes,
    rows_total, shapes, keep_heads).  Each op is a dict; tensors are :class:`Tensor`.
    ``fuse`` (default: same as ``reuse``): mark conv pairs the executor may run as one kernel; with
    ``reuse=False, fuse=True`` (per-block parity tests) the intermediate tensor of a fused pair keeps
    its arena slot but is never written.
    ``pool``: "reference" [default] or "darknet" max-pool semantics for every [maxpool] block; under "darknet" each maxpool op
    carries ``pool="darknet"`` and ``pad`` (Darknet's ``padding``), under the default neither key.
    ``keep_heads``: the float32 outputs of the detection-head convs stay alive to the end of the plan (their arena slots are
    not reused), for a caller that reads them after the forward (multi-label detections); the ops themselves do not change.
    """
    if fuse is None:
        fuse = reuse
    n = len(blocks)
    shapes = infer_shapes(blocks, net_info, height, width, pool)
    kinds = [b["type"] for b in blocks]

    # ---- consumers of every block output -------------------------------------------------
    readers = [[] for _ in range(n)]      # (consumer block, role)
    for i, blk in enumerate(blocks):
        kind = kinds[i]
        if kind in ("convolutional", "maxpool", "upsample", "avgpool") + REORG_KINDS + HEAD_KINDS:
            if i > 0:
                readers[i - 1].append((i, "in"))
        elif kind == "route":
            for j in blk["layers"]:
                readers[j].append((i, "route"))
        elif kind == "dropout":
            if i > 0:
                readers[i - 1].append((i, "route"))   # an alias of its input, as a single-layer route of -1 is
        elif kind in ("shortcut", "scale_channels", "sam"):
            # (an attention block's two inputs under a shortcut's roles: the head rules below cover them, and a conv is fused
            # with what follows it only when that is its one reader, so no fusion swallows a tensor an attention block reads)
            readers[i - 1].append((i, "sc_prev"))
            readers[i + blk["from"]].append((i, "sc_from"))

    check_head_readers(blocks, readers, elem_size)

    # ---- shortcut fusion: conv (i-1) + shortcut (i) when nobody else reads conv i-1 -------
    fused_into = {}      # shortcut block -> conv block
    for i, blk in enumerate(blocks):
        if kinds[i] == "shortcut" and kinds[i - 1] == "convolutional" and i + blk["from"] != i - 1:
            if [r for r in readers[i - 1] if r != (i, "sc_prev")] == []:
                fused_into[i] = i - 1
    conv_fused = {v: k for k, v in fused_into.items()}

    # ---- concat placement ------------------------------------------------------------------
    def resolve(j):
        """follow single-source routes (and [dropout] blocks) down to the block that really produces the data"""
        while j > 0 and (kinds[j] == "dropout" or
                         (kinds[j] == "route" and len(blocks[j]["layers"]) == 1 and route_groups(blocks[j])[0] == 1)):
            j = j - 1 if kinds[j] == "dropout" else blocks[j]["layers"][0]
        return j

    buffers = {}            # id -> dict(bytes, first, last)
    tensor_of = [None] * n
    placed = {}             # producing block -> Tensor inside a concat buffer
    copies = {}             # route block -> list of (src block, Tensor dst) needing a copy op
    head_of = {}            # conv block feeding a yolo block
    for i in range(n):
        if kinds[i] in HEAD_KINDS and kinds[i - 1] == "convolutional":
            head_of[i - 1] = i

    for i, blk in enumerate(blocks):
        if kinds[i] == "route" and len(blk["layers"]) > 1:
            c_tot, h, w = shapes[i]
            ld = _round_up(c_tot, CH_ALIGN)
            buf = "cat%d" % i
            buffers[buf] = dict(elems=batch * h * w * ld, es=elem_size)
            tensor_of[i] = Tensor(buf, 0, ld, c_tot, h, w)
            off = 0
            copies[i] = []
            for j in blk["layers"]:
                src = resolve(j)
                # the data of block `src` is produced by conv src-1... if src is a fused shortcut
                cj = shapes[j][0]
                dst = Tensor(buf, off, ld, cj, h, w)
                ok = (src not in placed and off % CH_ALIGN == 0 and src < i
                      and kinds[src] in ("convolutional", "maxpool", "upsample", "shortcut") + REORG_KINDS + ATTENTION_KINDS
                      and src not in head_of and kinds[src] != "route")
                if ok:
                    placed[src] = dst
                else:
                    copies[i].append((j, dst))
                off += cj

    def own_tensor(i, f32=False):
        c, h, w = shapes[i]
        ld = _round_up(c, CH_ALIGN)
        buf = "t%d" % i
        buffers[buf] = dict(elems=batch * h * w * ld, es=4 if f32 else elem_size)
        return Tensor(buf, 0, ld, c, h, w, f32)

    # ---- emit ops ---------------------------------------------------------------------------
    ops = []
    def mask_of(blk):
        m = blk["mask"]
        return m if isinstance(m, list) else [m]      # "mask=0" parses to a bare int

    def n_anchors(blk):
        return int(blk.get("num", 1)) if blk["type"] == "region" else len(mask_of(blk))

    rows_total = sum(n_anchors(blocks[i]) * shapes[i][1] * shapes[i][2] for i in range(n) if kinds[i] in HEAD_KINDS)
    row_offset = 0
    conv_slot = 0
    in_tensor = Tensor("input", 0, net_info["channels"], net_info["channels"], height, width)

    def prev_tensor(i):
        return in_tensor if i == 0 else tensor_of[i - 1]

    for i, blk in enumerate(blocks):
        kind = kinds[i]
        if kind == "convolutional":
            k, s = blk["size"], blk["stride"]
            target = conv_fused.get(i, i)          # block whose tensor this conv produces
            if target in placed:
                out = placed[target]
            else:
                out = own_tensor(target, f32=(i in head_of))
            res = None
            if i in conv_fused:
                sc = conv_fused[i]
                res = tensor_of[sc + blocks[sc]["from"]]
            op = dict(kind="conv", block=i, inp=prev_tensor(i), out=out, res=res, ksize=k, stride=s,
                            pad=(k - 1) // 2 if "pad" in blk else 0, leaky=blk["activation"] == "leaky",
                            slot=conv_slot, bn=bool(blk.get("batch_normalize", 0)), net_input=(i == 0),
                            # hint for the executor: the next op is a conv and the ONLY reader of this conv's
                            # output, so the pair may run as one kernel that never writes this tensor (stem + stride-2
                            # conv, 1x1 + 3x3 of a residual block); needs arena reuse semantics, i.e. not the
                            # keep-every-tensor debugging mode.  Whether a fused kernel exists is the executor's call.
                            fuse_next=bool(fuse and i not in conv_fused and i + 1 < n and
                                           kinds[i + 1] == "convolutional" and readers[i] == [(i + 1, "in")]))
            if int(blk.get("groups", 1)) > 1:
                op["groups"] = int(blk["groups"])      # (ordinary convs carry no key: their op dicts are what they were)
            if blk["activation"] == "mish":
                op["mish"] = True
            elif blk["activation"] == "logistic":
                op["logistic"] = True
            ops.append(op)
            conv_slot += 1
            if i in conv_fused:
                tensor_of[i] = None                # never materialised
                tensor_of[conv_fused[i]] = out
            else:
                tensor_of[i] = out
        elif kind in ("maxpool", "upsample"):
            out = placed[i] if i in placed else own_tensor(i)
            op = dict(kind=kind, block=i, inp=prev_tensor(i), out=out, ksize=blk.get("size", 1), stride=blk["stride"])
            if kind == "maxpool" and pool == "darknet":
                op["pool"] = "darknet"
                op["pad"] = maxpool_geometry(i, blk, op["inp"].h, op["inp"].w, pool)[2]
            ops.append(op)
            tensor_of[i] = out
        elif kind in REORG_KINDS:
            out = placed[i] if i in placed else own_tensor(i)
            op = dict(kind="reorg", block=i, inp=prev_tensor(i), out=out, stride=int(blk.get("stride", 1)))
            if kind == "reorg3d":
                op["form3d"] = True                # the space-to-depth form (default: Darknet's original flat form)
            ops.append(op)
            tensor_of[i] = out
        elif kind in ATTENTION_KINDS:
            # handled as an unfused [shortcut] is: an op of its own that reads the block in front (and `from`'s block) and writes
            # a tensor of its own or its slice of a route's buffer; both inputs stay alive until it has run (liveness below)
            out = placed[i] if i in placed else own_tensor(i)
            op = dict(kind=kind, block=i, inp=tensor_of[i - 1], out=out)
            if kind != "avgpool":
                op["res"] = tensor_of[i + blk["from"]]
            ops.append(op)
            tensor_of[i] = out
        elif kind == "dropout":
            tensor_of[i] = prev_tensor(i)          # no op, no buffer
        elif kind == "shortcut":
            if i in fused_into:
                pass                               # produced by the conv's epilogue
            else:
                out = placed[i] if i in placed else own_tensor(i)
                ops.append(dict(kind="add", block=i, inp=tensor_of[i - 1], res=tensor_of[i + blk["from"]], out=out))
                tensor_of[i] = out
        elif kind == "route":
            groups, gid = route_groups(blk)
            if len(blk["layers"]) == 1 and groups == 1:
                tensor_of[i] = tensor_of[blk["layers"][0]]
            elif len(blk["layers"]) == 1:
                # grouped route: channel group `gid` of the source, an alias at the same pixel stride (no copy) unless
                # the slice breaks the channel-slice granularity
                src = tensor_of[blk["layers"][0]]
                c = src.c // groups
                off = src.off + gid * c
                if off % CH_ALIGN == 0 and c % CH_ALIGN == 0:
                    tensor_of[i] = Tensor(src.buf, off, src.ld, c, src.h, src.w, src.f32)
                else:
                    out = own_tensor(i)
                    ops.append(dict(kind="copy", block=i, inp=Tensor(src.buf, off, src.ld, c, src.h, src.w, src.f32),
                                    out=out))
                    tensor_of[i] = out
            else:
                for j, dst in copies[i]:
                    ops.append(dict(kind="copy", block=i, inp=tensor_of[j], out=dst))
        elif kind in HEAD_KINDS:
            src = tensor_of[i - 1]
            c, h, w = shapes[i]
            na = n_anchors(blk)
            if c % na != 0 or c // na <= 5:
                raise ValueError("{} block {}: {} channels do not split into {} anchors".format(kind, i, c, na))
            if kind == "region":
                # the default decode over all `num` anchors (no mask): centres, objectness and the soft-max score are what
                # a [region] head with softmax=1 computes; its anchors, in grid cells, become pixels of the cfg's net size
                anchors = region_anchors(blk, net_info, h, w)
            else:
                anchors = [blk["anchors"][m] for m in mask_of(blk)]
            op = dict(kind="yolo", block=i, inp=src, anchors=anchors, n_attr=c // na,
                      row_offset=row_offset, rows_total=rows_total)
            if kind == "region":
                op["region"] = True
            if float(blk.get("scale_x_y", 1)) != 1.0:
                op["scale_x_y"] = float(blk["scale_x_y"])     # Darknet's centre stretch (default 1: the YOLOv3 decode)
            if int(blk.get("new_coords", 0)) != 0:
                op["new_coords"] = True                       # Darknet's decode of a logistic head (check_blocks)
            ops.append(op)
            row_offset += na * h * w
            tensor_of[i] = src
        if tensor_of[i] is None and kind != "convolutional":
            raise AssertionError("block {} has no tensor".format(i))

    # ---- liveness + arena ---------------------------------------------------------------------
    first, last = {}, {}
    for t, op in enumerate(ops):
        for key in ("inp", "res"):
            tt = op.get(key)
            if tt is not None and tt.buf != "input":
                last[tt.buf] = t
                first.setdefault(tt.buf, t)     # read before written would be a planner bug
        tt = op.get("out")
        if tt is not None:
            first.setdefault(tt.buf, t)
            last[tt.buf] = max(last.get(tt.buf, t), t)
    for buf in buffers:
        if buf not in first:
            raise AssertionError("buffer {} never produced".format(buf))
    if keep_heads:
        for op in ops:
            if op["kind"] == "yolo":
                last[op["inp"].buf] = len(ops) - 1

    nbytes = {buf: _round_up(d["elems"] * d["es"], ALIGN) for buf, d in buffers.items()}
    offsets = {}
    free = []          # (offset, size) sorted by offset
    top = 0

    def alloc(size):
        nonlocal top
        best = None
        for idx, (o, s) in enumerate(free):
            if s >= size and (best is None or s < free[best][1]):
                best = idx
        if best is not None:
            o, s = free.pop(best)
            if s > size:
                free.append((o + size, s - size))
                free.sort()
            return o
        o = top
        top += size
        return o

    def release(o, size):
        free.append((o, size))
        free.sort()
        merged = []
        for fo, fs in free:
            if merged and merged[-1][0] + merged[-1][1] == fo:
                merged[-1] = (merged[-1][0], merged[-1][1] + fs)
            else:
                merged.append((fo, fs))
        free[:] = merged

    by_first = {}
    by_last = {}
    for buf in buffers:
        by_first.setdefault(first[buf], []).append(buf)
        by_last.setdefault(last[buf], []).append(buf)
    for t in range(len(ops)):
        for buf in by_first.get(t, []):
            offsets[buf] = alloc(nbytes[buf])
        if reuse:
            for buf in by_last.get(t, []):
                release(offsets[buf], nbytes[buf])

    return dict(ops=ops, buffers=nbytes, offsets=offsets, arena_bytes=max(top, ALIGN),
                rows_total=rows_total, shapes=shapes, n_convs=conv_slot, live=(first, last),
                tensor_of=tensor_of, keep_heads=bool(keep_heads))
