#!/usr/bin/env python3
"""Kernel time of the two batched preprocessing launches on one MI355X: ``y3_letterbox_u8`` (uint8 canvas) and
``y3_preprocess_darknet_f32`` (Darknet's float resize / letterbox), same frames, same network size.

    rocprofv3 --kernel-trace --output-format csv -d <dir> -- python tools/preprocess_bench.py
    python tools/preprocess_bench.py --summarize <dir>

The first form launches each kernel ``--runs`` times after ``--warmup`` (the frames are random bytes already on the device) and
prints the shader clock sampled while the launches are queued; the second reads the kernel trace the profiler wrote -- begin and
end of every dispatch -- and prints the median, minimum and maximum per kernel."""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))

KERNELS = ("letterbox_u8_kernel", "preprocess_darknet_kernel")


def sclk_mhz():
    for path in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*/freq1_input")):
        try:
            with open(path) as fh:
                return int(fh.read()) / 1e6
        except (OSError, ValueError):
            continue
    return float("nan")


def summarize(directory):
    times = {k: [] for k in KERNELS}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                for k in KERNELS:
                    if k in row["Kernel_Name"]:
                        times[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for k in KERNELS:
        t = times[k]
        if not t:
            raise SystemExit("no dispatch of %s in the trace under %s" % (k, directory))
        print("%-28s %3d dispatches   median %8.2f us   min %8.2f   max %8.2f" % (k, len(t), statistics.median(t), min(t), max(t)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarize", metavar="DIR")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--frame", type=int, nargs=2, default=(1080, 1920), metavar=("H", "W"))
    ap.add_argument("--net", type=int, nargs=2, default=(608, 608), metavar=("H", "W"))
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import torch
    from yolov3 import _hip
    from yolov3.preprocess import darknet_frames_device, letterbox_frames_device
    _hip.require_gpu()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    frames = [torch.randint(0, 256, (args.frame[0], args.frame[1], 3), dtype=torch.uint8, generator=gen).to(dev)
              for _ in range(args.batch)]
    clocks = []
    for name, run in (("y3_letterbox_u8", lambda: letterbox_frames_device(frames, args.net[0], args.net[1], dev)),
                      ("y3_preprocess_darknet_f32", lambda: darknet_frames_device(frames, args.net[0], args.net[1], dev, True))):
        for _ in range(args.warmup):
            run()
        torch.cuda.synchronize()
        for _ in range(args.runs):
            run()
            clocks.append(sclk_mhz())
        torch.cuda.synchronize()
        print("%s: %d launches of %d frames %d x %d -> %d x %d" % ((name, args.runs, args.batch) + tuple(args.frame) + tuple(args.net)))
    print("sclk while queued: median %.0f MHz (min %.0f, max %.0f)" % (statistics.median(clocks), min(clocks), max(clocks)))


if __name__ == "__main__":
    main()
