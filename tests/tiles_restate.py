"""Tiled inference restated in numpy and the oracle, independent of yolov3/tiles.py and of the kernels: what a tile holds
(crop plus pad), and what the tiled detection tail keeps (per tile: threshold, float32 product, ``astype(int64)``, the tile's
offset, ``oracle.cxywh_to_tlbr``; then ``oracle.non_max_suppression`` on the union in (tile, row) order).  Also the planted
tensors the GPU tests of the tail share."""
import numpy as np

from oracle import darknet_oracle as orc

F = np.float32


def crop_pad(img, y0, x0, net_h, net_w, fill):
    """Pixel (y, x) of the tile is the frame's (y0 + y, x0 + x) where that lies inside the frame, else ``fill``."""
    out = np.full((net_h, net_w, 3), fill, dtype=np.uint8)
    part = img[y0:y0 + net_h, x0:x0 + net_w]
    out[:part.shape[0], :part.shape[1]] = part
    return out


def arange_frame(h, w, start=0):
    """uint8 (h, w, 3) whose bytes are ``(start + arange) % 251``: no two neighbouring rows, pixels or channels look alike."""
    return ((start + np.arange(h * w * 3, dtype=np.int64)) % 251).astype(np.uint8).reshape(h, w, 3)


def plain_geom(net_h, net_w, grid):
    return [(float(net_w), float(net_h), int(x0), int(y0)) for y0, x0 in grid]


def tiled_postprocess(box, prob, cls, geom, prob_thresh, iou):
    """One frame: box (T, rows, 4) f32, prob (T, rows) f32, cls (T, rows) i64, geom T x (sx, sy, ox, oy).
    -> [tlbr, prob, cls, combined rows] of the kept detections, and the number of candidates."""
    tiles, rows = prob.shape
    tl, pr, cl, rw = [], [], [], []
    for t in range(tiles):
        sx, sy, ox, oy = geom[t]
        mask = prob[t] >= F(prob_thresh)
        b = box[t, mask, :].astype(F).copy()
        b[:, [0, 2]] *= F(sx)                                # float32 products
        b[:, [1, 3]] *= F(sy)
        ib = b.astype(np.int64)                              # truncation toward zero
        ib[:, 0] += int(ox)                                  # ... and only then the tile's place in the frame
        ib[:, 1] += int(oy)
        tl.append(orc.cxywh_to_tlbr(ib))
        pr.append(prob[t, mask])
        cl.append(cls[t, mask])
        rw.append(t * rows + np.nonzero(mask)[0])
    tlbr, p, c, r = np.concatenate(tl), np.concatenate(pr), np.concatenate(cl), np.concatenate(rw).astype(np.int64)
    keep = [int(k) for k in orc.non_max_suppression(tlbr, p, class_idx=c, iou_thresh=iou)]
    return [tlbr[keep], p[keep], c[keep], r[keep]], len(p)


def unique_scores(rng, shape):
    """float32 scores in (0, 1), all different: the oracle's argsort leaves the order of ties open beyond 16 candidates."""
    n = int(np.prod(shape))
    return ((rng.permutation(n) + 1).astype(np.float64) / (n + 1)).astype(F).reshape(shape)


def random_outputs(seed, n_tiles, rows, n_cls, size=0.7):
    """Forward outputs of ``n_tiles`` tiles: centres a little outside [0, 1] too, sizes from 0.4 ``size`` to ``size`` of a tile --
    large enough that most candidates are suppressed, by boxes of their own tile and of its neighbours."""
    rng = np.random.default_rng(seed)
    box = np.empty((n_tiles, rows, 4), F)
    box[..., :2] = rng.uniform(-0.1, 1.1, size=(n_tiles, rows, 2))
    box[..., 2:] = rng.uniform(0.4 * size, size, size=(n_tiles, rows, 2))
    return box, unique_scores(rng, (n_tiles, rows)), rng.integers(0, n_cls, size=(n_tiles, rows)).astype(np.int64)


def grid_geom(n_y, n_x, net, step):
    """An n_y x n_x grid of 1:1 tiles of a square network ``net``, ``step`` pixels apart (step < net: they overlap)."""
    return [(float(net), float(net), x * step, y * step) for y in range(n_y) for x in range(n_x)]
