"""Float32 torch-CPU restatement of Darknet's max-pool rule, independent of the package, stated twice.

For a [maxpool] block with ``size=k``, ``stride=s`` and ``padding=p`` (Darknet's default when the key is absent: k - 1) on an
H x W map:
  out_h = (H + p - k) / s + 1,  out_w = (W + p - k) / s + 1                      (integer division)
  out[i][j] = max over n, m in [0, k) of in[i * s + n - p / 2][j * s + m - p / 2]  (integer p / 2), taps inside the image only.

``pool_loop`` is that rule as written; ``pool`` is torch's max-pool on a tensor padded with -inf by p / 2 on the left / top and
p - p / 2 on the right / bottom, cropped to Darknet's output size.  tests/test_darknet_pool_host.py pins one against the other.
Max of stored values is exact, so both are exact for float32, and for bf16 / fp16 values held in float32.

``DarknetPools`` turns a whole-network restatement (tests/yolov4_restate.py, tests/new_coords_restate.py) into one that pools
this way.
"""
import torch
import torch.nn.functional as F

from oracle import darknet_oracle as orc

import new_coords_restate as NR
import yolov4_restate as R


def out_size(n, k, s, p):
    return (n + p - k) // s + 1


def padding_of(blk):
    return int(blk.get("padding", blk["size"] - 1))


def pool_loop(x, k, s, p=None):
    """The rule, tap by tap.  x: (B, C, H, W) float32.  For small tensors."""
    p = k - 1 if p is None else p
    b, c, h, w = x.shape
    oh, ow = out_size(h, k, s, p), out_size(w, k, s, p)
    out = torch.full((b, c, oh, ow), float("-inf"), dtype=x.dtype)
    for i in range(oh):
        for j in range(ow):
            for n in range(k):
                for m in range(k):
                    y, xx = i * s + n - p // 2, j * s + m - p // 2
                    if 0 <= y < h and 0 <= xx < w:
                        out[:, :, i, j] = torch.maximum(out[:, :, i, j], x[:, :, y, xx])
    return out


def pool(x, k, s, p=None):
    """The rule through torch.nn.functional.max_pool2d on a -inf padded tensor."""
    p = k - 1 if p is None else p
    h, w = x.shape[2], x.shape[3]
    lo, hi = p // 2, p - p // 2
    padded = F.pad(x, (lo, hi, lo, hi), value=float("-inf"))
    return F.max_pool2d(padded, k, s)[:, :, :out_size(h, k, s, p), :out_size(w, k, s, p)].contiguous()


class DarknetPools(object):
    """Mix-in in front of a ``Restatement``: the same forward, with ``pool`` where theirs calls the oracle's max-pool."""

    def forward(self, x, emulate=None):
        rnd = orc.storage_round(emulate)
        rounds = self.rounding_points()
        outs, heads = [], []
        with torch.no_grad():
            if rnd is not None:
                x = rnd(x)
            for i, blk in enumerate(self.blocks):
                kind = blk["type"]
                if kind == "convolutional":
                    x = self.conv(i, x, emulate)
                    if rnd is not None and rounds[i]:
                        x = rnd(x)
                elif kind == "maxpool":
                    x = pool(x, blk["size"], blk["stride"], padding_of(blk))
                elif kind == "upsample":
                    x = orc.upsample(x, blk["stride"])
                elif kind == "route":
                    x = R.route(outs, blk)
                elif kind == "shortcut":
                    x = outs[i - 1] + outs[i + blk["from"]]
                    if rnd is not None:
                        x = rnd(x)
                elif kind == "yolo":
                    heads.append(self.decode(i, x))
                outs.append(x)
        return {"bbox_xywh": torch.cat([h[0] for h in heads], 1), "class_prob": torch.cat([h[1] for h in heads], 1),
                "class_idx": torch.cat([h[2] for h in heads], 1)}


class Restatement(DarknetPools, R.Restatement):
    """yolov3-spp, yolov3-tiny (leaky / linear only), yolov4, yolov4-tiny"""


class NewCoordsRestatement(DarknetPools, NR.Restatement):
    """yolov4-csp"""
