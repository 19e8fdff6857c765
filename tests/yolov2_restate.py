"""Float32 restatement of what the YOLOv2 cfgs add to the Darknet layers the other families use: the two forms of the
pass-through layer (``[reorg]``, ``[reorg3d]``) and the ``[region]`` head.  Independent of the package: it reads the cfg with
``oracle.ref_io``, states the reorgs as Darknet's literal loops in numpy on NCHW arrays and the decode from Darknet's formulas in
torch; for conv + BN, LeakyReLU, max-pools and the 16-bit storage rounding of the bf16 / fp16 modes it reuses
``oracle.darknet_oracle``, as tests/yolov4_restate.py does.

Darknet's definitions, input (C, H, W) per frame, stride s, output (C*s*s, H/s, W/s):
  [reorg]    with oc = C / (s*s), for k < C, j < H, i < W:
                 c2 = k % oc, off = k / oc, w2 = i*s + off % s, h2 = j*s + off / s
                 out_flat[i + W*(j + H*k)] = in_flat[w2 + (W*s)*(h2 + (H*s)*c2)]
             on the frame's flat arrays of C*H*W values; out_flat is then read as (C*s*s, H/s, W/s)
  [reorg3d]  for k < C*s*s, j < H/s, i < W/s, g = k / C:  out[k, j, i] = in[k % C, j*s + g / s, i*s + g % s]
  [region]   softmax=1, coords=4, anchors (a_w, a_h) in grid cells, cell (i, j) of a w x h grid:
                 box = ((i + sigmoid(tx)) / w, (j + sigmoid(ty)) / h, exp(tw) * a_w / w, exp(th) * a_h / h)
                 score = sigmoid(to) * max_c softmax(classes)_c,  class = the first index of that maximum
"""
import numpy as np
import torch

from oracle import darknet_oracle as orc
from oracle import ref_io


def reorg_flat(x, s):
    """Darknet's original [reorg] on one batch (B, C, H, W): the literal loop, every element moved on its own."""
    x = np.ascontiguousarray(x)
    b_, c_, h_, w_ = x.shape
    assert h_ % s == 0 and w_ % s == 0 and c_ % (s * s) == 0
    oc = c_ // (s * s)
    out = np.empty_like(x).reshape(b_, -1)
    flat = x.reshape(b_, -1)
    for k in range(c_):
        c2, off = k % oc, k // oc
        for j in range(h_):
            h2 = j * s + off // s
            for i in range(w_):
                w2 = i * s + off % s
                out[:, i + w_ * (j + h_ * k)] = flat[:, w2 + (w_ * s) * (h2 + (h_ * s) * c2)]
    return out.reshape(b_, c_ * s * s, h_ // s, w_ // s)


def reorg_3d(x, s):
    """[reorg3d], the space-to-depth of later Darknet, as the literal loop."""
    x = np.ascontiguousarray(x)
    b_, c_, h_, w_ = x.shape
    assert h_ % s == 0 and w_ % s == 0
    out = np.empty((b_, c_ * s * s, h_ // s, w_ // s), dtype=x.dtype)
    for k in range(c_ * s * s):
        g = k // c_
        for j in range(h_ // s):
            for i in range(w_ // s):
                out[:, k, j, i] = x[:, k % c_, j * s + g // s, i * s + g % s]
    return out


def reorg(x, s, form3d=False):
    return reorg_3d(x, s) if form3d else reorg_flat(x, s)


def reorg_block(x, blk):
    """a [reorg] / [reorg3d] block on a torch tensor"""
    return torch.from_numpy(reorg(x.numpy(), int(blk.get("stride", 1)), blk["type"] == "reorg3d"))


def region_decode(x, anchors):
    """x: (B, num * (5 + classes), h, w) float32 logits; anchors: ``num`` (a_w, a_h) pairs in grid cells.  Returns
    (bbox (B, num*h*w, 4), prob, cls) with row = anchor * h * w + y * w + x, every operation in float32."""
    b, ch, h, w = x.shape
    na = len(anchors)
    t = x.reshape(b, na, ch // na, h, w)
    gx = torch.arange(w, dtype=torch.float32).reshape(1, 1, 1, w)
    gy = torch.arange(h, dtype=torch.float32).reshape(1, 1, h, 1)
    aw = torch.tensor([a[0] for a in anchors], dtype=torch.float32).reshape(1, na, 1, 1)
    ah = torch.tensor([a[1] for a in anchors], dtype=torch.float32).reshape(1, na, 1, 1)
    bx = (gx + torch.sigmoid(t[:, :, 0])) / w
    by = (gy + torch.sigmoid(t[:, :, 1])) / h
    bw = torch.exp(t[:, :, 2]) * aw / w
    bh = torch.exp(t[:, :, 3]) * ah / h
    best, idx = torch.max(torch.softmax(t[:, :, 5:], dim=2), dim=2)
    prob = torch.sigmoid(t[:, :, 4]) * best
    bbox = torch.stack((bx, by, bw, bh), dim=-1).reshape(b, na * h * w, 4)
    return bbox, prob.reshape(b, -1), idx.reshape(b, -1)


class Restatement(object):
    """Walks a cfg of [convolutional] / [maxpool] / [route] / [reorg] / [reorg3d] / [region] blocks."""

    def __init__(self, cfg, params):
        self.blocks, self.net_info = ref_io.read_cfg(cfg)
        for i, blk in enumerate(self.blocks):
            if blk["type"] == "route":
                blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
        convs = [i for i, blk in enumerate(self.blocks) if blk["type"] == "convolutional"]
        self.slot = {bi: n for n, bi in enumerate(convs)}
        self.params = params

    def rounding_points(self):
        """Block outputs the 16-bit modes store rounded: every conv but the head conv (float32 logits)."""
        n = len(self.blocks)
        return [not (blk["type"] == "convolutional" and i + 1 < n and self.blocks[i + 1]["type"] == "region")
                for i, blk in enumerate(self.blocks)]

    def conv(self, i, x, emulate=None):
        blk = self.blocks[i]
        k = blk["size"]
        assert blk["activation"] in ("leaky", "linear")
        return orc.conv_block(x, self.params[self.slot[i]], blk["stride"], (k - 1) // 2 if "pad" in blk else 0,
                              blk["activation"] == "leaky", round_weights=emulate)

    def anchors(self, i):
        blk = self.blocks[i]
        return [tuple(a) for a in blk["anchors"][:int(blk["num"])]]

    def decode(self, i, logits):
        """(bbox, prob, cls) of region block i from its float32 logits"""
        return region_decode(logits, self.anchors(i))

    def forward(self, x, emulate=None):
        """x: (B,3,H,W) float32 in [0,1].  Returns the forward dict; ``emulate`` "bf16" / "f16": 16-bit storage."""
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
                    x = orc.maxpool(x, blk["size"], blk["stride"])
                elif kind == "route":
                    x = torch.cat([outs[j] for j in blk["layers"]], dim=1)
                elif kind in ("reorg", "reorg3d"):
                    x = reorg_block(x, blk)
                elif kind == "region":
                    heads.append(self.decode(i, x))
                else:
                    raise AssertionError("block %d: %s" % (i, kind))
                outs.append(x)
        return {"bbox_xywh": torch.cat([h[0] for h in heads], 1), "class_prob": torch.cat([h[1] for h in heads], 1),
                "class_idx": torch.cat([h[2] for h in heads], 1)}


def frames_to_input(frames):
    return torch.from_numpy(orc.frames_to_input(frames))
