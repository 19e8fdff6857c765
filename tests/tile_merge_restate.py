"""The seam-merge rule of ``y3_merge_tiled`` (include/yolov3_hip.h), restated with plain Python loops over Python ints.  It shares
no code with ``yolov3.tiles.merge_detections``.  ``merge(..., wrong=...)`` is the same loop with ONE rule bent, one switch per
wrong rule: the tests use them to show that the case table tells the right rule from each of them.

    "ge"         a pair at exactly the threshold matches (>= instead of >)
    "iou"        intersection over union instead of intersection over the smaller area
    "same_tile"  pairs from one tile may match
    "absorbing"  an absorbed detection goes on absorbing (what it takes goes to its keeper)
    "grown"      a keeper matches with its grown (union) box instead of its original one
"""
WRONG_RULES = ("ge", "iou", "same_tile", "absorbing", "grown")


def measures(box):
    """(w, h, area) of (x1, y1, x2, y2) with the +1 pixel convention."""
    w = box[2] - box[0] + 1
    h = box[3] - box[1] + 1
    return w, h, w * h


def degenerate(box):
    w, h, _ = measures(box)
    return w <= 0 or h <= 0


def intersection(a, b):
    iw = min(a[2], b[2]) - max(a[0], b[0]) + 1
    ih = min(a[3], b[3]) - max(a[1], b[1]) + 1
    return max(iw, 0) * max(ih, 0)


def ios(a, b):
    """Intersection over the smaller area of two non-degenerate boxes: float64 division of the two integers as floats."""
    return float(intersection(a, b)) / float(min(measures(a)[2], measures(b)[2]))


def iou(a, b):
    inter = intersection(a, b)
    return float(inter) / float(measures(a)[2] + measures(b)[2] - inter)


def merge(boxes, scores, classes, rows, tile_rows, thr, wrong=None, owners=False):
    """One frame.  boxes: n sequences of four ints; scores, classes, rows: n values each, all in canonical order.
    -> (boxes, scores, classes, rows, members) of the keepers, as lists (boxes as tuples of ints); with ``owners`` instead the
    list that holds, per input detection, the index of the keeper that absorbed it (None for a keeper)."""
    assert wrong is None or wrong in WRONG_RULES, wrong
    n = len(boxes)
    orig = [tuple(int(v) for v in b) for b in boxes]
    cls = [int(c) for c in classes]
    assert cls == sorted(cls), "not in canonical order: classes must ascend"
    tile = [int(r) // int(tile_rows) for r in rows]
    keeper_of = [None] * n                  # None = not absorbed
    grown = [list(b) for b in orig]
    members = [1] * n
    for i in range(n):
        if keeper_of[i] is not None and wrong != "absorbing":
            continue
        k = i if keeper_of[i] is None else keeper_of[i]          # who gets what i takes
        if degenerate(orig[i]):
            continue
        for j in range(i + 1, n):
            if cls[j] != cls[i]:
                break                                                # classes ascend: the rest belongs to other classes
            if keeper_of[j] is not None or degenerate(orig[j]):
                continue
            if tile[j] == tile[i] and wrong != "same_tile":
                continue
            mine = tuple(grown[k]) if wrong == "grown" else orig[i]
            measure = iou(mine, orig[j]) if wrong == "iou" else ios(mine, orig[j])
            if measure > thr or (wrong == "ge" and measure == thr):
                keeper_of[j] = k
                members[k] += 1
                grown[k] = [min(grown[k][0], orig[j][0]), min(grown[k][1], orig[j][1]),
                            max(grown[k][2], orig[j][2]), max(grown[k][3], orig[j][3])]
    if owners:
        return keeper_of
    keep = [i for i in range(n) if keeper_of[i] is None]
    return ([tuple(grown[i]) for i in keep], [scores[i] for i in keep], [cls[i] for i in keep], [int(rows[i]) for i in keep],
            [members[i] for i in keep])
