#!/usr/bin/env python3
"""Micro-benchmark of the depthwise kernel on MobileNetV2-style 3x3 layers (runs on an MI355X).

For every layer shape, at batch 1 and batch 16 in bf16, the op is planned twice -- as the library chooses (``conv_dwise_*``) and
under ``y3_set_tuning("grouped_generic", 1)`` (``conv_grouped_*``, the baseline: no earlier version of the library runs these
ops at all) -- and timed with ``y3_plan_run_profiled`` (events bound to the dispatch: the kernel's own begin -> end), the two
alternating in one process after a warm-up.  Two regimes per shape:

  warm   one set of buffers, run again and again: whatever fits stays in the L2s (4 MiB per XCD, 32 MiB in all) or the Infinity
         Cache (256 MiB), so small maps read ABOVE the HBM roof;
  cold   the plans rotate over enough buffer sets (up to 64) that the bytes between two uses of a set exceed the Infinity
         Cache where the shape allows it: the HBM-bound figure.  The rotating working set is printed; below 256 MiB the
         figure is still a cache figure and is marked so.

GB/s = algorithmic bytes (input + output + weights, each once) / median kernel time; the roof is the 6.3 TB/s achievable HBM
bandwidth of the MI355X.  The outputs of the two kernels are compared bit for bit.
Usage: python tools/grouped_bench.py [--iters 20] [--rounds 3] [--dtype bf16] [--out FILE]
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from yolov3 import _hip  # noqa: E402
from yolov3.darknet import grouped_weight_layout  # noqa: E402
from yolov3.plan_ops import padded_weight_dims  # noqa: E402

# (input map side, channels, stride): the depthwise layers of MobileNetV2 at a 416 x 416 input
LAYERS = [(208, 96, 2), (104, 144, 1), (104, 144, 2), (52, 192, 1), (52, 192, 2), (26, 384, 1), (26, 576, 1), (26, 576, 2),
          (13, 960, 1)]
HBM_ROOF_GBS = 6300.0
L2_BYTES, MALL_BYTES = 32 << 20, 256 << 20
TORCH_DT = {"bf16": torch.bfloat16, "fp16": torch.float16, "float32": torch.float32}
DT_CODE = {"bf16": _hip.Y3_BF16, "fp16": _hip.Y3_F16, "float32": _hip.Y3_F32}


class OnePlan(object):
    """a one-op plan of a depthwise 3x3 conv on buffers of its own"""

    def __init__(self, side, c, stride, batch, dtype, generic, shared):
        lib = _hip.lib()
        dev = torch.device("cuda:0")
        tdt = TORCH_DT[dtype]
        es = torch.empty(0, dtype=tdt).element_size()
        out_side = (side + 2 - 3) // stride + 1
        self.x = (torch.rand((batch, side, side, c), device=dev) - 0.5).to(tdt)
        self.out = torch.empty((batch, out_side, out_side, c), dtype=tdt, device=dev)
        ops = (_hip.Y3Op * 1)()
        op = ops[0]
        op.kind, op.dtype, op.batch, op.flags, op.block_idx = _hip.OP_CONV, DT_CODE[dtype], batch, _hip.F_LEAKY, 1
        op.in_h = op.in_w = side
        op.out_h = op.out_w = out_side
        op.in_c = op.in_ld = op.out_c = op.out_ld = op.groups = c
        op.ksize, op.stride, op.pad = 3, stride, 1
        op.d_in, op.d_out = self.x.data_ptr(), self.out.data_ptr()
        with _hip.grouped_generic(generic):
            op.cout_pad, op.k_ld = 128, 1 << 20
            path = lib.y3_conv_path(ctypes.byref(op))
            key = ("w", path)
            if key not in shared:          # (weights, scale and bias are shared by every buffer set: they are read each time anyway)
                cp, k_ld = padded_weight_dims(path, c, c, 3, es, c)
                host = grouped_weight_layout(path, shared["w"], c, cp, k_ld)
                shared[key] = (torch.from_numpy(host).to(tdt).to(dev), torch.ones(cp, device=dev), torch.zeros(cp, device=dev), cp, k_ld)
            w, sc, bi, op.cout_pad, op.k_ld = shared[key]
            op.d_weight, op.d_scale, op.d_bias = w.data_ptr(), sc.data_ptr(), bi.data_ptr()
            self.handle = ctypes.c_void_p()
            _hip.check(lib.y3_plan_create(ops, 1, shared["zero"].data_ptr(), ctypes.byref(self.handle)))
        self.ops = ops
        self.kernel = lib.y3_plan_op_kernel(self.handle, 0).decode()
        self.bytes = lib.y3_plan_op_bytes(self.handle, 0)
        self.set_bytes = (self.x.numel() + self.out.numel()) * es

    def run(self):
        ms = (ctypes.c_float * 1)()
        _hip.check(_hip.lib().y3_plan_run_profiled(self.handle, None, _hip.stream_ptr(), ms))
        return ms[0]

    def destroy(self):
        _hip.lib().y3_plan_destroy(self.handle)


def bound(nbytes):
    if nbytes <= L2_BYTES:
        return "L2"
    return "Infinity Cache" if nbytes <= MALL_BYTES else "HBM"


def measure(plans, iters, rounds, warmup):
    """plans: {variant: [OnePlan per buffer set]}; the variants alternate round by round; -> {variant: median ms}"""
    times = {v: [] for v in plans}
    for v in plans:
        for i in range(warmup):
            plans[v][i % len(plans[v])].run()
    for _ in range(rounds):
        for v in plans:
            for i in range(iters):
                times[v].append(plans[v][i % len(plans[v])].run())
    return {v: statistics.median(t) for v, t in times.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--batches", default="1,16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _hip.require_gpu()
    lines = ["# tools/grouped_bench.py: depthwise 3x3, %s, median kernel time of %d x %d runs per regime (y3_plan_run_profiled), "
             "variants alternating" % (args.dtype, args.rounds, args.iters),
             "# GB/s = (input + output + weights) / time; HBM roof %.0f GB/s; 'bound' = where the working set of the regime lives" % HBM_ROOF_GBS,
             "%-22s %5s %-6s %9s %-15s | %-22s %9s %8s %6s | %-22s %9s %8s | %7s" % (
                 "layer", "batch", "regime", "MiB", "bound", "kernel", "us", "GB/s", "%roof", "baseline kernel", "us", "GB/s", "speedup")]
    gen = torch.Generator().manual_seed(7)
    for side, c, stride in LAYERS:
        for batch in [int(b) for b in args.batches.split(",")]:
            shared = {"w": ((torch.rand((c, 1, 3, 3), generator=gen) - 0.5) * 0.5).numpy().astype(np.float32),
                      "zero": torch.zeros(4096, dtype=torch.uint8, device="cuda:0")}
            first = {"dwise": OnePlan(side, c, stride, batch, args.dtype, False, shared),
                     "generic": OnePlan(side, c, stride, batch, args.dtype, True, shared)}
            first["generic"].x.copy_(first["dwise"].x)
            first["dwise"].run()
            first["generic"].run()
            torch.cuda.synchronize()
            same = torch.equal(first["dwise"].out, first["generic"].out)
            n_sets = max(1, min(64, -(-2 * MALL_BYTES // first["dwise"].set_bytes)))
            sets = {v: [p] + [OnePlan(side, c, stride, batch, args.dtype, v == "generic", shared) for _ in range(n_sets - 1)]
                    for v, p in first.items()}
            name = "%dx%d c%d s%d" % (side, side, c, stride)
            for regime, plans in (("warm", {v: s[:1] for v, s in sets.items()}), ("cold", sets)):
                t = measure(plans, args.iters, args.rounds, args.warmup)
                ws = first["dwise"].set_bytes * len(plans["dwise"])
                algo = first["dwise"].bytes
                gbs = {v: algo / (t[v] * 1e-3) / 1e9 for v in t}
                lines.append("%-22s %5d %-6s %9.2f %-15s | %-22s %9.2f %8.0f %5.0f%% | %-22s %9.2f %8.0f | %6.2fx%s" % (
                    name, batch, regime, ws / 2.0 ** 20, bound(ws), first["dwise"].kernel, t["dwise"] * 1e3, gbs["dwise"],
                    100.0 * gbs["dwise"] / HBM_ROOF_GBS, first["generic"].kernel, t["generic"] * 1e3, gbs["generic"],
                    t["generic"] / t["dwise"], "" if same else "  OUTPUTS DIFFER"))
                print(lines[-1], flush=True)
            for s in sets.values():
                for p in s:
                    p.destroy()
            del sets, first
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    else:
        print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
