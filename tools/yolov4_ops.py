"""Per-op kernel times of YOLOv4 (bf16, batch 16, 608) with its mish backbone, next to the same network with every mish
replaced by leaky (same parameters, same shapes: what mish costs per layer), plus forward frames/s and achieved TFLOP/s
(plan_report() flops over kernel time) of yolov4 and yolov4-tiny.  Procedural weights, calibrated like bench.py's.

    python tools/yolov4_ops.py [--batch 16] [--passes 10] [--out FILE]
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
import yolov3  # noqa: E402
from yolov3 import weights as W  # noqa: E402
from yolov3.synthdata import synth_frames  # noqa: E402

MODELS = os.path.join(ROOT, "pytorch-yolov3_amd", "models")


def op_times(cfg, params, frames, dtype, passes):
    net = yolov3.Darknet(cfg, device="cuda", dtype=dtype).set_params(params)
    x = torch.from_numpy(frames).cuda()
    for _ in range(3):
        net.forward_frames(x, fresh=False)
    per = []
    for _ in range(passes):
        net._run(x, "u8", timed="kernel")
        per.append(net.last_op_ms)
    ms = np.median(np.array(per), axis=0)
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 20
    start.record()
    for _ in range(n):
        net.forward_frames(x, fresh=False)
    stop.record()
    torch.cuda.synchronize()
    fps = n * len(frames) / (start.elapsed_time(stop) / 1e3)
    return net.plan_report(), ms, fps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--passes", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []
    for model, dim in (("yolov4", 608), ("yolov4-tiny", 416)):
        cfg = os.path.join(MODELS, model + ".cfg")
        net0 = yolov3.Darknet(cfg)
        params = W.synth_params(net0.blocks, net0.net_info, seed=0, obj_bias=-5.0, calib=W.load_calibration(model))
        frames = synth_frames(5, args.batch, dim, dim)
        rep, ms, fps = op_times(cfg, params, frames, args.dtype, args.passes)
        flops = sum(r["flops"] for r in rep)
        lines.append("%s %dx%d %s batch %d: forward %.1f frames/s; kernels %.3f ms per batch, %.1f GFLOP per frame, %.1f TFLOP/s"
                     % (model, dim, dim, args.dtype, args.batch, fps, ms.sum(), flops / args.batch / 1e9,
                        flops / (ms.sum() * 1e-3) / 1e12))
        if model != "yolov4":
            continue
        text = open(cfg).read().replace("activation=mish", "activation=leaky")
        with tempfile.NamedTemporaryFile("w", suffix=".cfg", delete=False) as fh:
            fh.write(text)
        rep_l, ms_l, fps_l = op_times(fh.name, params, frames, args.dtype, args.passes)
        os.unlink(fh.name)
        lines.append("yolov4 with leaky in place of mish: forward %.1f frames/s; kernels %.3f ms per batch" % (fps_l, ms_l.sum()))
        mish_blocks = {i for i, b in enumerate(net0.blocks) if b["type"] == "convolutional" and b.get("activation") == "mish"}
        lines.append("%4s %5s %-36s %9s %-36s %9s %8s %7s" % ("op", "block", "kernel (mish)", "us", "kernel (leaky)", "us",
                                                              "mish/lk", "TF/s"))
        tm = tl = 0.0
        for k, (a, b) in enumerate(zip(rep, rep_l)):
            mark = "*" if a["block"] in mish_blocks else " "
            if mark == "*":
                tm += ms[k]
                tl += ms_l[k]
            tf = a["flops"] / (ms[k] * 1e-3) / 1e12 if ms[k] > 0 else 0.0
            lines.append("%4d %4d%s %-36s %9.1f %-36s %9.1f %8.3f %7.1f" % (
                k, a["block"], mark, a["kernel"][:36], ms[k] * 1e3, b["kernel"][:36], ms_l[k] * 1e3,
                ms[k] / ms_l[k] if ms_l[k] > 0 else 0.0, tf))
        lines.append("mish layers (*): %.3f ms as mish, %.3f ms as leaky (%+.2f %%)" % (tm, tl, 100 * (tm / tl - 1)))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
