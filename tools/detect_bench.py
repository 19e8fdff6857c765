"""Time the fused detection tail (y3_detect; with --nms-kind, y3_detect_darknet) alone on the forward outputs of the bench
workload: per regime, the median of --passes passes of --iters launches each, after --load seconds of sustained launches."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
import yolov3  # noqa: E402
from yolov3 import weights as W  # noqa: E402
from yolov3.inference import Detector  # noqa: E402
from yolov3.synthdata import synth_frames  # noqa: E402


def telemetry(dev):
    """bench.py's sclk sampler (plain reads of the card's hwmon files) for the device the tail runs on."""
    sys.path.insert(0, ROOT)
    import bench
    pr = torch.cuda.get_device_properties(dev)
    return bench.GpuTelemetry("%04x:%02x:%02x.0" % (pr.pci_domain_id, pr.pci_bus_id, pr.pci_device_id), interval=0.005)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obj-bias", type=float, nargs="+", default=[-8.5, -5.0, -3.0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--nms-kind", nargs="+", default=["none"], choices=["none", "iou", "greedynms", "diounms"],
                    help="suppression rules to time: none = the reference's (y3_detect), else Darknet's (y3_detect_darknet)")
    ap.add_argument("--beta-nms", type=float, default=0.6)
    ap.add_argument("--prob-thresh", type=float, default=0.05)
    ap.add_argument("--iou-thresh", type=float, default=0.3)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--load", type=float, default=1.0, help="seconds of launches before the timed passes of each line")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    tel = telemetry(dev)
    cfg = os.path.join(ROOT, "pytorch-yolov3_amd", "models", "yolov3.cfg")
    for ob in args.obj_bias:
        net = yolov3.Darknet(cfg, device="cuda:0", dtype="bf16").eval()
        net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=ob, calib=W.load_calibration("yolov3")))
        frames = torch.from_numpy(synth_frames(123, args.batch, 608, 608)).to(dev)
        out = net.forward_frames(frames, fresh=False)
        rows = out["class_prob"].shape[1]
        det = Detector(args.batch, rows, dev)
        hw = torch.tensor([[608, 608]] * args.batch, dtype=torch.int32, device=dev)
        cand = int((out["class_prob"] >= args.prob_thresh).sum()) / args.batch
        for kind in args.nms_kind:
            kw = {} if kind == "none" else {"nms_kind": kind, "beta_nms": args.beta_nms}

            def launch():
                det.run(out, hw, args.prob_thresh, args.iou_thresh, **kw)

            t_end = time.time() + args.load
            while time.time() < t_end:
                for _ in range(args.iters):
                    launch()
                torch.cuda.synchronize()
            ms = []
            with tel:
                for _ in range(args.passes):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.iters):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1) / args.iters)
            kept = float(det.count.float().mean())
            print("obj_bias %.1f nms_kind %s: %.1f candidates/frame, %.1f kept/frame, detect median %.4f ms (min %.4f max %.4f, "
                  "%d passes x %d) per batch of %d, sclk %s MHz" % (ob, kind, cand, kept, statistics.median(ms), min(ms), max(ms),
                                                               args.passes, args.iters, args.batch, tel.summary().get("sclk_mhz")), flush=True)


if __name__ == "__main__":
    main()
