#!/usr/bin/env python3
"""The attention kernels (csrc/attention.hip) next to their yardsticks, add_<dtype> and copy_<dtype> of the main library, on tensors
of the same byte count (runs on an MI355X).  One-op plans through the C ABI on dense tensors; kernel time from event pairs bound to
the dispatch (y3_plan_run_profiled); the kernels alternate inside every round, the figure of a round is the median of its
repeats, and the line gives the median, the least and the greatest round -- the spread the ratios have to be read against.

sam moves add's bytes (two tensors in, one out); scale_channels moves copy's plus the (C, 1, 1) scales; avgpool reads what copy
reads and writes almost nothing, so its figure is the read rate, next to copy's read rate (half of copy's bytes).
Usage: python tools/attention_bench.py [--batch 16] [--iters 30] [--rounds 7] [--dtype bf16]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from yolov3 import _hip  # noqa: E402

SHAPES = [("76x76x256", 76, 76, 256), ("19x19x1024", 19, 19, 1024)]
KINDS = (("avgpool", _hip.OP_AVGPOOL), ("scale_channels", _hip.OP_SCALE_CHANNELS), ("sam", _hip.OP_SAM), ("add", _hip.OP_ADD),
         ("copy", _hip.OP_COPY))
DT = {"bf16": (_hip.Y3_BF16, torch.bfloat16), "fp16": (_hip.Y3_F16, torch.float16), "float32": (_hip.Y3_F32, torch.float32)}


def clocks():
    try:
        return "sclk %d MHz" % torch.cuda.clock_rate()
    except Exception as exc:          # (no SMI library next to torch)
        return "clocks not available (%s)" % type(exc).__name__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--dtype", default="bf16")
    args = ap.parse_args()
    lib = _hip.lib()
    _hip.require_gpu()
    dev = torch.device("cuda:0")
    code, tdt = DT[args.dtype]
    es = torch.empty(0, dtype=tdt).element_size()
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    B = args.batch
    for name, h, w, c in SHAPES:
        g = torch.Generator().manual_seed(c)
        full = [torch.randn((B, h, w, c), generator=g).to(tdt).to(dev) for _ in range(2)]
        gate = torch.rand((B, 1, 1, c), generator=g).to(tdt).to(dev)
        out = torch.zeros((B, h, w, c), dtype=tdt, device=dev)
        pooled = torch.zeros((B, 1, 1, c), dtype=tdt, device=dev)
        plans = []
        for label, kind in KINDS:
            op = _hip.Y3Op()
            op.kind, op.dtype, op.batch, op.ksize, op.stride = kind, code, B, 1, 1
            op.in_h, op.in_w, op.in_c, op.in_ld = h, w, c, c
            op.out_h, op.out_w, op.out_c, op.out_ld = h, w, c, c
            op.d_in, op.d_out = full[0].data_ptr(), out.data_ptr()
            if label == "avgpool":
                op.out_h = op.out_w = 1
                op.d_out = pooled.data_ptr()
            elif label == "scale_channels":
                op.in_h = op.in_w = 1
                op.d_in, op.d_res, op.res_ld = gate.data_ptr(), full[1].data_ptr(), c
            elif label in ("sam", "add"):
                op.d_res, op.res_ld = full[1].data_ptr(), c
            arr = (_hip.Y3Op * 1)(op)
            handle = ctypes.c_void_p()
            _hip.check(lib.y3_plan_create_ex(arr, 1, zero.data_ptr(), None, ctypes.byref(handle)))
            plans.append((label, handle, arr))
        ms = (ctypes.c_float * 1)()
        rounds = {label: [] for label, _ in KINDS}
        for _ in range(args.rounds):
            for label, handle, _ in plans:
                for _ in range(3):
                    _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
                reps = []
                for _ in range(args.iters):
                    _hip.check(lib.y3_plan_run_profiled(handle, None, _hip.stream_ptr(), ms))
                    reps.append(ms[0] * 1e3)
                rounds[label].append(statistics.median(reps))
        tensor = B * h * w * c * es
        moved = {"avgpool": tensor, "scale_channels": 2 * tensor, "sam": 3 * tensor, "add": 3 * tensor, "copy": 2 * tensor}
        med = {label: statistics.median(v) for label, v in rounds.items()}
        print("%s batch %d %s (%.1f MiB a tensor; %s)" % (name, B, args.dtype, tensor / 2.0 ** 20, clocks()))
        for label, handle, _ in plans:
            v = rounds[label]
            grid = _hip.plan_op_dims(handle, 0)[0]
            print("  %-15s %-20s median %7.2f us  (rounds %7.2f .. %7.2f)  %6.0f GB/s of %5.1f MiB  %6d workgroups" % (
                label, lib.y3_plan_op_kernel(handle, 0).decode(), med[label], min(v), max(v), moved[label] / med[label] / 1e3,
                moved[label] / 2.0 ** 20, grid), flush=True)
        spread = {label: (max(v) - min(v)) / statistics.median(v) for label, v in rounds.items()}
        print("  sam / add time %.3f (spread of rounds: sam %.1f %%, add %.1f %%);  scale_channels / copy time %.3f (spread %.1f %%, %.1f %%)" % (
            med["sam"] / med["add"], 100 * spread["sam"], 100 * spread["add"], med["scale_channels"] / med["copy"],
            100 * spread["scale_channels"], 100 * spread["copy"]))
        print("  avgpool read rate / copy read rate %.3f (avgpool %.0f GB/s read, copy %.0f GB/s read; spread %.1f %%, %.1f %%)" % (
            (tensor / med["avgpool"]) / (tensor / med["copy"]), tensor / med["avgpool"] / 1e3, tensor / med["copy"] / 1e3,
            100 * spread["avgpool"], 100 * spread["copy"]), flush=True)
        for _, handle, _ in plans:
            lib.y3_plan_destroy(handle)


if __name__ == "__main__":
    main()
