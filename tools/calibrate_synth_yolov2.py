"""Per-BN-layer output statistics of procedural weights for the YOLOv2 cfgs (the synth_calibration.json entries "yolov2" and
"yolov2-tiny"; `python tools/calibrate_synth_yolov2.py yolov2-tiny` redoes one of them).

The same procedure as tools/calibrate_synth_yolov4.py, walking the cfg with the float32 CPU restatement of the reorg layer
(tests/yolov2_restate.py): before a BN conv is evaluated its conv output (pre-BN) mean / variance over the same seeded batch is
measured, rounded to 6 significant digits and installed as that layer's running statistics (yolov3.weights.synth_params'
formula).  Merges the entries into pytorch-yolov3_amd/yolov3/synth_calibration.json; prints the rms of every block.
"""
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
from yolov3 import weights as W  # noqa: E402
import yolov2_restate as R  # noqa: E402

CFG_DIR = os.path.join(ROOT, "pytorch-yolov3_amd", "models")
OUT = os.path.join(ROOT, "pytorch-yolov3_amd", "yolov3", "synth_calibration.json")


def calibrate(model, dim, seed=0):
    cfg = os.path.join(CFG_DIR, model + ".cfg")
    blocks, net_info = R.ref_io.read_cfg(cfg)
    params = W.synth_params(blocks, net_info, seed=seed)          # weights do not depend on the calibration
    net = R.Restatement(cfg, params)
    rs = np.random.RandomState(1234)
    frames = rs.randint(0, 256, size=(2, dim, dim, 3), dtype=np.uint8)
    x = R.frames_to_input(frames)
    calib, outs = [], []
    with torch.no_grad():
        for i, blk in enumerate(net.blocks):
            t = blk["type"]
            if t == "convolutional":
                li = net.slot[i]
                p = params[li]
                if "bn_gamma" in p:
                    k = blk["size"]
                    y = torch.nn.functional.conv2d(x, torch.from_numpy(p["weight"]), None, stride=blk["stride"],
                                                   padding=(k - 1) // 2 if "pad" in blk else 0)
                    m = float("%.6g" % float(y.mean()))
                    v = float("%.6g" % float(y.var(unbiased=False)))
                    calib.append([m, v])
                    base, co, sd = li * 8, p["bn_gamma"].shape[0], math.sqrt(v)      # synth_params' running statistics
                    p["bn_mean"] = (m + sd * (0.2 * W.hash_uniform(seed, base + 3, co) - 0.1)).astype(np.float32)
                    p["bn_var"] = (v * (0.9 + 0.2 * W.hash_uniform(seed, base + 4, co))).astype(np.float32)
                x = net.conv(i, x)
            elif t == "maxpool":
                x = R.orc.maxpool(x, blk["size"], blk["stride"])
            elif t == "route":
                x = torch.cat([outs[j] for j in blk["layers"]], dim=1)
            elif t in ("reorg", "reorg3d"):
                x = R.reorg_block(x, blk)
            outs.append(x)
            print(model, i, t, "rms %.3f" % float(x.pow(2).mean().sqrt()), flush=True)
    # the table reproduces the parameters measured with
    again = W.synth_params(blocks, net_info, seed=seed, calib=calib)
    for a, b in zip(again, params):
        if "bn_mean" in a:
            assert np.array_equal(a["bn_mean"], b["bn_mean"]) and np.array_equal(a["bn_var"], b["bn_var"])
    return calib


if __name__ == "__main__":
    with open(OUT) as fh:
        table = json.load(fh)
    dims = {"yolov2-tiny": 416, "yolov2": 608}
    for model in sys.argv[1:] or list(dims):
        table[model] = calibrate(model, dims[model])
    with open(OUT, "w") as fh:
        json.dump(table, fh, indent=0)
