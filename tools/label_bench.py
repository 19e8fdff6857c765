"""Time the multi-label expansion (y3_expand_labels: two launches) alone on the head outputs of the bench workload -- yolov3 at
608 x 608, procedural weights -- at Darknet's threshold 0.25 and at 0.001: per line, the median of --passes passes of --iters
calls each, after --load seconds of sustained calls.  With --frames-rate it also measures detect_in_frames on net-sized frames
for the reference scores, scores="darknet" and multi_label=True."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
import yolov3  # noqa: E402
from yolov3 import _hip  # noqa: E402
from yolov3 import weights as W  # noqa: E402
from yolov3.synthdata import synth_frames  # noqa: E402

CFG = os.path.join(ROOT, "pytorch-yolov3_amd", "models", "yolov3.cfg")


def network(obj_bias, dtype="bf16", **kw):
    net = yolov3.Darknet(CFG, device="cuda:0", dtype=dtype, **kw).eval()
    return net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=obj_bias, calib=W.load_calibration("yolov3")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj-bias", type=float, nargs="+", default=[-5.0, 0.0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--thresh", type=float, nargs="+", default=[0.25, 0.001])
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--load", type=float, default=1.0, help="seconds of calls before the timed passes of each line")
    ap.add_argument("--once", action="store_true", help="one call per threshold and nothing else (for a kernel trace)")
    ap.add_argument("--frames-rate", type=int, default=0, metavar="N", help="also time detect_in_frames over N net-sized frames")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    lib = _hip.lib()
    for ob in args.obj_bias:
        net = network(ob, scores="darknet", multi_label=True)
        frames = torch.from_numpy(synth_frames(123, args.batch, 608, 608)).to(dev)
        out = net.forward_frames(frames, fresh=False)
        heads = net.label_heads()
        rows = out["class_prob"].shape[1]
        head_mb = sum(args.batch * v.h * v.w * v.ld * 4 for v in heads) / 1e6
        cap = rows
        nws = lib.y3_expand_labels_workspace_bytes(args.batch, rows, cap)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        vbbox = torch.empty((args.batch, cap, 4), dtype=torch.float32, device=dev)
        vprob = torch.empty((args.batch, cap), dtype=torch.float32, device=dev)
        vcls = torch.empty((args.batch, cap), dtype=torch.int64, device=dev)
        vrow = torch.empty((args.batch, cap), dtype=torch.int32, device=dev)
        vcount = torch.zeros(args.batch, dtype=torch.int32, device=dev)
        for thresh in args.thresh:
            def launch():
                _hip.check(lib.y3_expand_labels(heads, len(heads), out["bbox_xywh"].data_ptr(), args.batch, rows,
                                                ctypes.c_float(thresh), cap, ws.data_ptr(), nws, vbbox.data_ptr(), vprob.data_ptr(),
                                                vcls.data_ptr(), vrow.data_ptr(), vcount.data_ptr(), _hip.stream_ptr()))
            launch()
            torch.cuda.synchronize()
            if args.once:
                continue
            t_end = time.time() + args.load
            while time.time() < t_end:
                for _ in range(args.iters):
                    launch()
                torch.cuda.synchronize()
            ms = []
            for _ in range(args.passes):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / args.iters)
            labels = vcount.float().mean().item()
            print("obj_bias %.1f thresh %g: %.1f labels/frame (capacity %d), head tensors %.1f MB, expand median %.4f ms "
                  "(min %.4f max %.4f, %d passes x %d) per batch of %d" % (
                      ob, thresh, labels, cap, head_mb, statistics.median(ms), min(ms), max(ms), args.passes, args.iters,
                      args.batch), flush=True)
        del net
    if args.frames_rate:
        frames = synth_frames(7, args.batch, 608, 608)
        stream = [frames[i % args.batch] for i in range(args.frames_rate)]
        for name, kw in (("scores=reference", {}), ("scores=darknet", dict(scores="darknet")),
                         ("multi_label", dict(scores="darknet", multi_label=True))):
            net = network(-5.0, **kw)
            rates = []
            for _ in range(3):
                t0 = time.time()
                n = sum(len(r[1]) for r in yolov3.detect_in_frames(net, stream, batch_size=args.batch, prob_thresh=0.25,
                                                                   nms_iou_thresh=0.45))
                rates.append(len(stream) / (time.time() - t0))
            print("detect_in_frames %s, bf16, thresh 0.25, %d frames: %.0f frames/s (best of 3: %s), %d detections" % (
                name, len(stream), max(rates), ", ".join("%.0f" % r for r in rates), n), flush=True)
            del net


if __name__ == "__main__":
    main()
