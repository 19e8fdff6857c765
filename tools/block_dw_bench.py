#!/usr/bin/env python3
"""A/B of the direct-weights fused block kernel (csrc/conv_block_dw.hip, fuse_block = 3) against the two separate launches
(fuse_block = 0) and the old fused kernel (csrc/conv_block.hip, fuse_block = 1) on the 76^2 pairs of yolov3@608 (runs on an
MI355X).  For every shape: three two-op plans through the C ABI on the same operands, bit-equality of the outputs, HIP-event
time per plan run (interleaved rounds, best of and median).
Usage: python tools/block_dw_bench.py [--batch 16] [--iters 50] [--rounds 5] [--stamps]
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

import block_dw_util as BU  # noqa: E402
from yolov3 import _hip  # noqa: E402

# name, Cin, Cout, shortcut
SHAPES = [("s76_256-128-256_res", 256, 256, True), ("s76_384-128-256", 384, 256, False), ("s76_256-128-256", 256, 256, False)]
MODES = (("two launches", 0), ("block_fused", 1), ("block_dw", 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--stamps", action="store_true", help="library built with `make stamps` (Y3_HIP_LIB): phase cycles of block_dw")
    args = ap.parse_args()
    lib = _hip.lib()
    _hip.require_gpu()
    dev = torch.device("cuda:0")
    stream = _hip.stream_ptr()
    B, h = args.batch, 76
    for name, cin, cout, res in SHAPES:
        t, ops, _, _ = BU.random_pair(dev, args.dtype, B, h, h, cin, cout, res, seed=cin + cout)
        outs = [torch.zeros((B, h, h, cout), dtype=t["x"].dtype, device=dev) for _ in MODES]
        plans = [BU.make_plan(ops, t["zero"], o, fuse_block=m) for o, (_, m) in zip(outs, MODES)]
        names = [[lib.y3_plan_op_kernel(pl, i).decode() for i in range(2)] for pl in plans]
        times = [[] for _ in MODES]
        for _ in range(args.rounds):
            for vi, pl in enumerate(plans):
                for _ in range(3):
                    _hip.check(lib.y3_plan_run(pl, None, stream))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    _hip.check(lib.y3_plan_run(pl, None, stream))
                e1.record()
                torch.cuda.synchronize()
                times[vi].append(e0.elapsed_time(e1) / args.iters * 1e3)
                if args.stamps and MODES[vi][1] == 3:
                    buf = (ctypes.c_ulonglong * 8)()
                    lib.y3_debug_stamps_block_dw(buf)
                    n = float(buf[7]) or 1.0
                    print("    [stamps] workgroups %.0f  cycles/workgroup: wait+barrier-A %.0f  mma-A %.0f  mid-write %.0f  mid-barrier %.0f  "
                          "K loops-B %.0f  write-out %.0f" % (n, buf[0] / n, buf[1] / n, buf[2] / n, buf[3] / n, buf[5] / n, buf[6] / n))
        flops = 2.0 * (cin * 128 + 9 * 128 * cout) * h * h * B
        print("%-22s b%d %s" % (name, B, args.dtype))
        for vi, (label, _) in enumerate(MODES):
            best, med = min(times[vi]), statistics.median(times[vi])
            print("  %-12s best %6.1f us  median %6.1f us  %6.0f TFLOP/s  [%s]  bit-identical to two launches: %s" % (
                label, best, med, flops / best / 1e6, " + ".join(n for n in names[vi] if not n.startswith("(")),
                torch.equal(outs[vi], outs[0])), flush=True)
        for pl in plans:
            lib.y3_plan_destroy(pl)


if __name__ == "__main__":
    main()
