"""Float32 torch-CPU restatement of what Scaled-YOLOv4 (yolov4-csp) adds to the YOLOv4 cfgs: ``activation=logistic`` on a
conv and Darknet's ``[yolo] new_coords=1`` decode.  Builds on tests/yolov4_restate.py (mish, grouped routes, scale_x_y) by
importing it; no reference implementation of these two exists to pin it against, so tests/test_new_coords_host.py pins it
with hand-computed answers.

Darknet's definitions:
  logistic(x)  = 1 / (1 + e^-x)                                    (torch.sigmoid)
  new_coords   : the head conv ends in a logistic, so the decode reads probabilities t, with no exp and no soft-max:
                 centre = (sxy(t) + cell) / grid, sxy(v) = v * s - (s - 1) / 2 with the head's scale_x_y s
                 size   = ((t * t) * 4) * anchor / net
                 prob   = max_c t_c * t_obj, cls the first index of the largest stored t_c
  every operation rounded in float32 on its own.
"""
import torch

import yolov4_restate as R


def conv(x, p, blk, emulate=None):
    """conv -> BN -> activation of one [convolutional] block, logistic included (float32, not rounded to storage)."""
    y = R.conv(x, p, blk, emulate)            # linear for "logistic": the restatement below applies it
    if blk["activation"] == "logistic":
        y = torch.sigmoid(y)
    return y


def new_coords_decode(x, anchors, s=1.0):
    """(bbox with w, h in pixels, prob, cls) of a new_coords head from its probabilities x (B, A * n_attr, h, w)."""
    b, ch, h, w = x.shape
    na = len(anchors)
    t = x.reshape(b, na, ch // na, h, w)
    gx = torch.arange(w, dtype=torch.float32).reshape(1, 1, 1, w)
    gy = torch.arange(h, dtype=torch.float32).reshape(1, 1, h, 1)
    aw = torch.tensor([a[0] for a in anchors], dtype=torch.float32).reshape(1, na, 1, 1)
    ah = torch.tensor([a[1] for a in anchors], dtype=torch.float32).reshape(1, na, 1, 1)
    four = torch.tensor(4.0, dtype=torch.float32)
    bx = (R.scale_xy(t[:, :, 0], s) + gx) / w
    by = (R.scale_xy(t[:, :, 1], s) + gy) / h
    bw = ((t[:, :, 2] * t[:, :, 2]) * four) * aw
    bh = ((t[:, :, 3] * t[:, :, 3]) * four) * ah
    best, idx = torch.max(t[:, :, 5:], dim=2)           # first index of the maximum on ties
    bbox = torch.stack((bx, by, bw, bh), dim=-1).reshape(b, na * h * w, 4)
    return bbox, (best * t[:, :, 4]).reshape(b, -1), idx.reshape(b, -1)


class Restatement(R.Restatement):
    def conv(self, i, x, emulate=None):
        return conv(x, self.params[self.slot[i]], self.blocks[i], emulate)

    def decode(self, i, x):
        """(bbox with w, h / net size, prob, cls) of yolo block i from its head conv's float32 output."""
        blk = self.blocks[i]
        if int(blk.get("new_coords", 0)) == 0:
            return R.Restatement.decode(self, i, x)
        box, prob, idx = new_coords_decode(x, [blk["anchors"][m] for m in R.mask_of(blk)], float(blk.get("scale_x_y", 1)))
        box[:, :, 2] /= self.net_info["width"]
        box[:, :, 3] /= self.net_info["height"]
        return box, prob, idx
