"""Torch-CPU restatement of Darknet's attention blocks -- ``[avgpool]``, ``[scale_channels]``, ``[sam]`` -- in float64 and in
float32, and of a cfg that holds them, walked by block index.  TEST INFRASTRUCTURE, independent of the package: the cfg is read
with ``oracle.ref_io``; what YOLOv3 / YOLOv4 already have comes from ``oracle.darknet_oracle`` and ``yolov4_restate``.

Darknet's definitions, for block i whose previous block's output is ``prev``:
  [avgpool]                out[c]       = mean over the H * W pixels of prev[c]                  (C, H, W) -> (C, 1, 1)
  [scale_channels] from=J  out[c][y][x] = src[c][y][x] * prev[c]       src = block i + J's output, prev (C, 1, 1)
  [sam] from=J             out          = src * prev, element by element, both of one shape
and ``activation=logistic`` on a conv is 1 / (1 + e^-x).  ``from`` is relative to the block, as a [shortcut]'s."""
import torch

from oracle import darknet_oracle as orc

import yolov4_restate as R4

KINDS = ("avgpool", "scale_channels", "sam")


def avgpool(x, dtype=torch.float64):
    """x (B, C, H, W) -> (B, C, 1, 1): the sum in ``dtype`` divided by H * W in ``dtype``"""
    p = x.shape[2] * x.shape[3]
    return x.to(dtype).sum(dim=(2, 3), keepdim=True) / torch.tensor(float(p), dtype=dtype)


def scale_channels(src, prev, dtype=torch.float64):
    assert prev.shape == (src.shape[0], src.shape[1], 1, 1), (tuple(src.shape), tuple(prev.shape))
    b, c, h, w = src.shape
    return src.to(dtype) * prev.to(dtype).expand(b, c, h, w)


def sam(src, prev, dtype=torch.float64):
    assert prev.shape == src.shape, (tuple(src.shape), tuple(prev.shape))
    return src.to(dtype) * prev.to(dtype)


def attention_block(blk, prev, src, dtype=torch.float32):
    """one block of KINDS as a float32 tensor (computed in ``dtype``, not rounded to storage)"""
    if blk["type"] == "avgpool":
        return avgpool(prev, dtype).float()
    return (scale_channels if blk["type"] == "scale_channels" else sam)(src, prev, dtype).float()


def conv(x, p, blk, emulate=None):
    """yolov4_restate.conv with ``activation=logistic``"""
    y = R4.conv(x, p, blk, emulate)
    return torch.sigmoid(y) if blk["activation"] == "logistic" else y


class Restatement(R4.Restatement):
    def conv(self, i, x, emulate=None):
        return conv(x, self.params[self.slot[i]], self.blocks[i], emulate)

    def src_of(self, i):
        return i + self.blocks[i]["from"]

    def rounding_points(self):
        """yolov4_restate's rule with the attention blocks among the readers: a conv is stored unrounded only in front of a
        [yolo] or as the sole operand of the shortcut directly after it"""
        n = len(self.blocks)
        readers = [0] * n
        for i, blk in enumerate(self.blocks):
            kind = blk["type"]
            if kind in ("convolutional", "maxpool", "upsample", "yolo", "avgpool") and i > 0:
                readers[i - 1] += 1
            elif kind == "route":
                for j in blk["layers"]:
                    readers[j] += 1
            elif kind in ("shortcut", "scale_channels", "sam"):
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

    def blocks_forward(self, x, emulate=None, dtype=torch.float32):
        """[block output] of every block, float32 tensors; ``emulate`` "bf16" / "f16": 16-bit storage; ``dtype``: what the
        attention blocks compute in.  A [yolo] block's entry is its input, the logits."""
        rnd = orc.storage_round(emulate)
        rounds = self.rounding_points()
        outs = []
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
                    x = R4.route(outs, blk)
                elif kind == "shortcut":
                    x = outs[i - 1] + outs[i + blk["from"]]
                    if rnd is not None:
                        x = rnd(x)
                elif kind in KINDS:
                    x = attention_block(blk, outs[i - 1], None if kind == "avgpool" else outs[self.src_of(i)], dtype)
                    if rnd is not None:
                        x = rnd(x)
                elif kind != "yolo":
                    raise AssertionError("block %d: %s" % (i, kind))
                outs.append(x)
        return outs

    def forward(self, x, emulate=None):
        outs = self.blocks_forward(x, emulate)
        heads = [self.decode(i, outs[i]) for i, blk in enumerate(self.blocks) if blk["type"] == "yolo"]
        return {"bbox_xywh": torch.cat([h[0] for h in heads], 1), "class_prob": torch.cat([h[1] for h in heads], 1),
                "class_idx": torch.cat([h[2] for h in heads], 1)}
