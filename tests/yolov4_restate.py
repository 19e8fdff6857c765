"""Float32 torch-CPU restatement of the semantics the YOLOv4 cfgs add to Darknet-53's: ``activation=mish``, grouped
routes (``[route] groups=G group_id=g``) and ``[yolo] scale_x_y``.  Independent of the package: it reads the cfg with
``oracle.ref_io`` and runs torch ops; for what YOLOv3 already has (conv + BN, LeakyReLU, pools, upsample, the 16-bit storage
rounding of the bf16 / fp16 modes) it reuses ``oracle.darknet_oracle``.

Darknet's definitions:
  mish(x)      = x * tanh(softplus(x))                             (torch.nn.functional.mish)
  grouped route: channels [g * C / G, (g + 1) * C / G) of the single source tensor
  scale_x_y s  : box centre = (sigmoid(t) * s - (s - 1) / 2 + cell) / grid, every operation rounded in float32
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import darknet_oracle as orc
from oracle import ref_io


def conv(x, p, blk, emulate=None):
    """conv -> BN -> activation of one [convolutional] block (float32, not rounded to storage)."""
    k = blk["size"]
    pad = (k - 1) // 2 if "pad" in blk else 0
    act = blk["activation"]
    y = orc.conv_block(x, p, blk["stride"], pad, act == "leaky", round_weights=emulate)
    if act == "mish":
        y = F.mish(y)
    return y


def route(outs, blk):
    x = torch.cat([outs[j] for j in blk["layers"]], dim=1)
    groups, gid = int(blk.get("groups", 1)), int(blk.get("group_id", 0))
    if groups != 1:
        c = x.shape[1] // groups
        x = x[:, gid * c:(gid + 1) * c]
    return x


def scale_xy(sig, s):
    """sigmoid(t) * s - (s - 1) / 2 as t = sig * s + (-0.5 (s - 1)), float32 op by op."""
    s = torch.tensor(float(s), dtype=torch.float32)
    return sig * s + torch.tensor(-0.5, dtype=torch.float32) * (s - torch.tensor(1.0, dtype=torch.float32))


def yolo_decode(x, anchors, s=1.0):
    """oracle.darknet_oracle.yolo_decode with Darknet's scale_x_y on the centre offsets."""
    b, ch, h, w = x.shape
    na = len(anchors)
    t = x.reshape(b, na, ch // na, h, w)
    gx = torch.arange(w, dtype=torch.float32).reshape(1, 1, 1, w)
    gy = torch.arange(h, dtype=torch.float32).reshape(1, 1, h, 1)
    aw = torch.tensor([a[0] for a in anchors], dtype=torch.float32).reshape(1, na, 1, 1)
    ah = torch.tensor([a[1] for a in anchors], dtype=torch.float32).reshape(1, na, 1, 1)
    bx = (scale_xy(torch.sigmoid(t[:, :, 0]), s) + gx) / w
    by = (scale_xy(torch.sigmoid(t[:, :, 1]), s) + gy) / h
    bw = torch.exp(t[:, :, 2]) * aw
    bh = torch.exp(t[:, :, 3]) * ah
    obj = torch.sigmoid(t[:, :, 4])
    best, idx = torch.max(torch.softmax(t[:, :, 5:], dim=2), dim=2)
    bbox = torch.stack((bx, by, bw, bh), dim=-1).reshape(b, na * h * w, 4)
    return bbox, (best * obj).reshape(b, -1), idx.reshape(b, -1)


def mask_of(blk):
    m = blk["mask"]
    return m if isinstance(m, list) else [m]


class Restatement(object):
    def __init__(self, cfg, params):
        self.blocks, self.net_info = ref_io.read_cfg(cfg)
        for i, blk in enumerate(self.blocks):
            if blk["type"] == "route":
                blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
        convs = [i for i, blk in enumerate(self.blocks) if blk["type"] == "convolutional"]
        self.slot = {bi: n for n, bi in enumerate(convs)}
        self.params = params

    def rounding_points(self):
        """Block outputs the 16-bit modes store rounded (as oracle.OracleDarknet.bf16_rounding_points): not the head convs
        (float32 logits) nor a conv whose only reader is the shortcut after it (one rounding of the sum)."""
        n = len(self.blocks)
        readers = [0] * n
        for i, blk in enumerate(self.blocks):
            if blk["type"] in ("convolutional", "maxpool", "upsample", "yolo") and i > 0:
                readers[i - 1] += 1
            elif blk["type"] == "route":
                for j in blk["layers"]:
                    readers[j] += 1
            elif blk["type"] == "shortcut":
                readers[i - 1] += 1
                readers[i + blk["from"]] += 1
        rounds = [True] * n
        for i, blk in enumerate(self.blocks):
            if blk["type"] != "convolutional":
                continue
            nxt = self.blocks[i + 1]["type"] if i + 1 < n else None
            if nxt == "yolo" or (nxt == "shortcut" and readers[i] == 1 and i + 1 + self.blocks[i + 1]["from"] != i):
                rounds[i] = False
        return rounds

    def conv(self, i, x, emulate=None):
        return conv(x, self.params[self.slot[i]], self.blocks[i], emulate)

    def decode(self, i, logits):
        """(bbox with w, h / net size, prob, cls) of yolo block i from its float32 logits."""
        blk = self.blocks[i]
        box, prob, idx = yolo_decode(logits, [blk["anchors"][m] for m in mask_of(blk)], float(blk.get("scale_x_y", 1)))
        box[:, :, 2] /= self.net_info["width"]
        box[:, :, 3] /= self.net_info["height"]
        return box, prob, idx

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
                elif kind == "upsample":
                    x = orc.upsample(x, blk["stride"])
                elif kind == "route":
                    x = route(outs, blk)
                elif kind == "shortcut":
                    x = outs[i - 1] + outs[i + blk["from"]]
                    if rnd is not None:
                        x = rnd(x)
                elif kind == "yolo":
                    heads.append(self.decode(i, x))
                outs.append(x)
        return {"bbox_xywh": torch.cat([h[0] for h in heads], 1), "class_prob": torch.cat([h[1] for h in heads], 1),
                "class_idx": torch.cat([h[2] for h in heads], 1)}


def frames_to_input(frames):
    return torch.from_numpy(orc.frames_to_input(frames))


def f32_ulp(a):
    return np.spacing(np.abs(np.asarray(a, dtype=np.float32)))
