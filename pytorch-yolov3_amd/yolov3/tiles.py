"""Tiled inference: a frame much larger than the network input is looked at through net-sized windows at full resolution
instead of being squeezed into one input.  Not in the reference, which resizes every frame to the network.

This module is the host side and needs no GPU: where the windows lie (:func:`tile_grid`), what each one's boxes need to get back
into the frame (:func:`tile_geometry`), which options tiling refuses (:func:`check_options`), and a numpy statement of the
cutter (:func:`cut_tiles_u8`).  The device side is ``y3_tiles_u8`` (the letterbox kernel's copy form) and ``y3_detect_tiled``
(the detection tail over the union of a frame's tiles); ``inference(..., tile_overlap=f)`` puts them together.

An object cut by a tile border yields partial boxes, and IoU suppression does not merge a part with the whole, unless
``tile_merge`` (``--tile-merge``) is given: otherwise the overlap
between neighbouring windows is what guards against that (an object smaller than the overlap lies whole in one window), along
with the overview -- the whole frame stretched to the network by the default 8-bit resize -- for objects larger than a window.

Seam merging (``inference(..., tile_overlap=f, tile_merge=t)``, ``y3_merge_tiled`` on the device) is an opt-in second pass over
a frame's detections: boxes of one class from DIFFERENT tiles whose intersection over the smaller area exceeds ``t`` are merged
into their union box, greedily in the canonical order, always matching on original boxes.  :func:`check_merge` checks the
threshold and :func:`merge_detections` states the rule in numpy (include/yolov3_hip.h states it in full).  Within one tile the
network saw both boxes at once and the IoU suppression has ruled, so same-tile pairs are left alone.  0.5 is a reasonable first
threshold; its effect on accuracy has not been measured here.
"""
import numpy as np

MAX_OVERLAP = 0.9


def check_overlap(overlap):
    """The overlap fraction as a float; ValueError unless 0 <= overlap <= 0.9."""
    try:
        f = float(overlap)
    except (TypeError, ValueError):
        raise ValueError("tile_overlap must be a fraction in [0, {}], got {!r}".format(MAX_OVERLAP, overlap))
    if not 0.0 <= f <= MAX_OVERLAP:                          # (NaN fails both comparisons)
        raise ValueError("tile_overlap must be a fraction in [0, {}], got {!r}".format(MAX_OVERLAP, overlap))
    return f


def check_merge(thr):
    """The seam-merge threshold as a float; ValueError for anything that is not a number in [0, 1] (NaN included)."""
    try:
        if isinstance(thr, (bool, str, bytes)):
            raise TypeError
        f = float(thr)
    except (TypeError, ValueError):
        raise ValueError("tile_merge must be a number in [0, 1], got {!r}".format(thr))
    if not 0.0 <= f <= 1.0:                                  # (NaN fails both comparisons)
        raise ValueError("tile_merge must be a number in [0, 1], got {!r}".format(thr))
    return f


def axis_origins(length, net, overlap):
    """Origins of the windows of ``net`` pixels along an axis of ``length`` pixels, in integers: one window at 0 when the axis
    fits (it is padded); otherwise ``n = ceil((length - ov) / (net - ov))`` windows with ``ov = int(overlap * net)``, spread
    evenly from 0 to ``length - net``, so that neighbours share at least ``ov`` pixels."""
    length, net = int(length), int(net)
    if length <= 0 or net <= 0:
        raise ValueError("axis_origins: sizes must be positive, got {}".format((length, net)))
    ov = int(check_overlap(overlap) * net)
    if length <= net:
        return [0]
    step = net - ov
    n = (length - ov + step - 1) // step
    return [(i * (length - net)) // (n - 1) for i in range(n)]


def tile_grid(src_h, src_w, net_h, net_w, overlap):
    """``[(y0, x0), ...]``: the origins of the net-sized windows that cover a (src_h, src_w) frame, row-major (y outer)."""
    xs = axis_origins(src_w, net_w, overlap)
    return [(y0, x0) for y0 in axis_origins(src_h, net_h, overlap) for x0 in xs]


def tile_geometry(src_h, src_w, net_h, net_w, grid, overview):
    """``[(sx, sy, ox, oy), ...]`` of ``y3_tile_geom`` for the windows of ``grid`` and, when ``overview``, the stretched whole
    frame after them: a window cut 1:1 at (y0, x0) scales its relative boxes by the network size and moves them by its
    origin, the overview scales by the frame size as an untiled frame does."""
    geom = [(float(net_w), float(net_h), int(x0), int(y0)) for y0, x0 in grid]
    if overview:
        geom.append((float(src_w), float(src_h), 0, 0))
    return geom


def cut_tiles_u8(img, net_h, net_w, grid, fill=128):
    """uint8 (H, W, 3) -> uint8 (len(grid), net_h, net_w, 3): what ``y3_tiles_u8`` computes, in numpy."""
    img = np.asarray(img)
    out = np.full((len(grid), net_h, net_w, 3), fill, dtype=np.uint8)
    for i, (y0, x0) in enumerate(grid):
        part = img[y0:y0 + net_h, x0:x0 + net_w]
        out[i, :part.shape[0], :part.shape[1]] = part
    return out


def check_options(overlap, letterbox=False, preprocess=None, resize=True, nms_kind=None, multi_label=False):
    """The overlap as a float, after refusing (ValueError, each by name) what tiling does not combine with: the tiled detection
    tail has no letterbox correction, no Darknet suppression kinds and no multi-label virtual rows, and the windows are uint8
    crops, which leaves nothing for Darknet's float preprocessing or ``resize=False`` to mean."""
    f = check_overlap(overlap)
    if letterbox:
        raise ValueError("tile_overlap cannot be combined with letterbox=True: tiles are cut 1:1 and the tiled detection tail "
                         "has no letterbox correction")
    if preprocess is not None:
        raise ValueError("tile_overlap cannot be combined with preprocess={!r}: tiles are cut from the uint8 frame".format(preprocess))
    if not resize:
        raise ValueError("tile_overlap cannot be combined with resize=False: a frame larger than the network is what tiling is for")
    if nms_kind is not None:
        raise ValueError("tile_overlap cannot be combined with nms_kind={!r}: the tiled detection tail computes the reference's "
                         "suppression only".format(nms_kind))
    if multi_label:
        raise ValueError("tile_overlap cannot be combined with a multi_label network: the tiled detection tail takes no "
                         "multi-label virtual rows")
    return f


def merge_detections(tlbr, prob, cls, rows, tile_rows, thr):
    """What ``y3_merge_tiled`` computes for one frame, in numpy: ``(tlbr, prob, cls, rows, members)`` of the keepers.

    The inputs are a frame's detections in canonical order (class ascending, score descending, row descending): int64 corners
    (n, 4), scores, classes and combined rows; a detection's tile is ``row // tile_rows``.  Areas and intersections are int64 with
    the +1 pixel convention, a box with ``w <= 0`` or ``h <= 0`` neither matches nor is matched, and ``a`` matches ``b`` iff
    ``inter / min(area_a, area_b) > thr`` in float64.  In order, a detection that nothing has absorbed is a keeper and absorbs
    every later, not yet absorbed detection of its class from another tile that its original box matches; a keeper's box
    becomes the union of its own and its members' original boxes, everything else it carries stays its own."""
    thr = check_merge(thr)
    tile_rows = int(tile_rows)
    if tile_rows < 1:
        raise ValueError("merge_detections: tile_rows must be positive, got {}".format(tile_rows))
    box = np.asarray(tlbr, dtype=np.int64).reshape(-1, 4)
    prob, cls, rows = np.asarray(prob), np.asarray(cls), np.asarray(rows)
    n = len(box)
    w, h = box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1
    area = w * h
    ok = (w > 0) & (h > 0)
    tile = rows.astype(np.int64) // tile_rows
    out = box.copy()
    members = np.ones(n, dtype=np.int32)
    free = np.ones(n, dtype=bool)          # not absorbed
    for i in range(n):
        if not (free[i] and ok[i]):
            continue
        later = slice(i + 1, n)
        iw = np.maximum(np.minimum(box[i, 2], box[later, 2]) - np.maximum(box[i, 0], box[later, 0]) + 1, 0)
        ih = np.maximum(np.minimum(box[i, 3], box[later, 3]) - np.maximum(box[i, 1], box[later, 1]) + 1, 0)
        small = np.minimum(area[i], area[later])
        cand = free[later] & ok[later] & (cls[later] == cls[i]) & (tile[later] != tile[i])
        ios = np.zeros(n - i - 1, dtype=np.float64)
        ios[cand] = (iw * ih)[cand].astype(np.float64) / small[cand].astype(np.float64)
        take = np.flatnonzero(cand & (ios > thr)) + i + 1
        if len(take):
            free[take] = False
            members[i] += len(take)
            out[i, :2] = np.minimum(out[i, :2], box[take, :2].min(axis=0))
            out[i, 2:] = np.maximum(out[i, 2:], box[take, 2:].max(axis=0))
    return out[free], prob[free], cls[free], rows[free], members[free]
