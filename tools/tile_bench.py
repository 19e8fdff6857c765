"""Time tiled inference on one large frame -- by default 3840 x 2160 through yolov3 at 608 x 608 in bf16, procedural weights,
overlap 0.2: 40 tiles and the overview -- piece by piece: the tile cutter (y3_tiles_u8) alone, the tiled detection tail
(y3_detect_tiled) alone at the candidate count the run produces, the forward of the same tiles in the chunks inference() uses,
and the whole inference() call from a host frame to host detections.  With --merge F also the seam merge (y3_merge_tiled) alone on
what that tail kept, and the whole call with tile_merge=F next to the call without.  Per line the median of --passes passes of --iters calls
each (device time between two events for the pieces, wall time for the call).

The detection tail is one workgroup per frame and greedy suppression is quadratic in the candidates of a class, so the
regime matters: the default objectness bias is bench.py's (-8.5, a few hundred candidates per tile); at -5.0 half of all rows are
candidates and one call takes seconds.  The candidate count is printed before the tail is timed, and a tail whose first call
takes more than --tail-limit-ms is reported from that one call."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
import yolov3  # noqa: E402
from yolov3 import _hip  # noqa: E402
from yolov3.inference import Detector, _MergeBuffers, cut_tiles_device, frame_tiles_device, tile_chunks, tile_geom_tensor  # noqa: E402
from yolov3 import tiles  # noqa: E402
from yolov3 import weights as W  # noqa: E402
from yolov3.synthdata import synth_frames  # noqa: E402


def device_ms(fn, passes, iters):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(passes):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return ms


def line(what, ms, passes, iters):
    print("%-58s median %8.4f ms (min %.4f max %.4f, %d passes x %d)" % (what, statistics.median(ms), min(ms), max(ms), passes, iters),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov3")
    ap.add_argument("--frame", type=int, nargs=2, default=[2160, 3840], metavar=("H", "W"))
    ap.add_argument("--overlap", type=float, default=0.2)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--obj-bias", type=float, default=-8.5)
    ap.add_argument("--tail-limit-ms", type=float, default=100.0)
    ap.add_argument("--thresh", type=float, default=0.05)
    ap.add_argument("--tile-batch", type=int, default=16)
    ap.add_argument("--merge", type=float, default=None, metavar="F", help="also time the seam merge at this threshold")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = os.path.join(ROOT, "pytorch-yolov3_amd", "models", args.model + ".cfg")
    net = yolov3.Darknet(cfg, device="cuda:0", dtype=args.dtype).eval()
    net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=args.obj_bias, calib=W.load_calibration(args.model)))
    net_h, net_w = net.net_info["height"], net.net_info["width"]
    h, w = args.frame
    # a frame of procedural content: net-sized synthetic frames side by side
    ny, nx = -(-h // net_h), -(-w // net_w)
    parts = synth_frames(5, ny * nx, net_h, net_w)
    frame = np.ascontiguousarray(np.concatenate([np.concatenate(list(parts[r * nx:(r + 1) * nx]), axis=1) for r in range(ny)])[:h, :w])
    grid = tiles.tile_grid(h, w, net_h, net_w, args.overlap)
    n_tiles = len(grid) + 1
    print("%s %dx%d %s, frame %d x %d, overlap %g: %d tiles + overview, chunks of %d" % (
        args.model, net_h, net_w, args.dtype, w, h, args.overlap, len(grid), args.tile_batch), flush=True)

    d_frame = torch.from_numpy(frame).to(dev)
    d_tiles = torch.empty((n_tiles, net_h, net_w, 3), dtype=torch.uint8, device=dev)
    line("y3_tiles_u8, %d tiles (two launches)" % len(grid),
         device_ms(lambda: cut_tiles_device(d_frame, net_h, net_w, grid, out=d_tiles[:len(grid)]), args.passes, args.iters),
         args.passes, args.iters)
    line("tiles + overview from a device frame",
         device_ms(lambda: frame_tiles_device(d_frame, net_h, net_w, dev, args.overlap, True, out=d_tiles), args.passes, args.iters),
         args.passes, args.iters)

    _, geom = frame_tiles_device(d_frame, net_h, net_w, dev, args.overlap, True, out=d_tiles)
    chunks = tile_chunks(n_tiles, args.tile_batch)
    outs = [net.forward_frames(d_tiles[a:b]) for a, b in chunks]
    union = {k: torch.cat([o[k] for o in outs]).contiguous() for k in outs[0]}
    rows = int(union["class_prob"].shape[1])

    def forward():
        for a, b in chunks:
            net.forward_frames(d_tiles[a:b], fresh=False)
    line("forward of the %d tiles in chunks %s" % (n_tiles, [b - a for a, b in chunks]), device_ms(forward, args.passes, args.iters),
         args.passes, args.iters)

    det = Detector(1, n_tiles * rows, dev)
    d_geom = tile_geom_tensor(geom, dev)
    thr = float(np.float32(args.thresh))
    mask = union["class_prob"] >= thr
    n_cand = int(mask.sum().item())
    per_class = int(torch.bincount(union["class_idx"][mask].clamp(min=0)).max().item()) if n_cand else 0
    print("candidates at %g: %d of %d rows, %d in the largest class" % (args.thresh, n_cand, n_tiles * rows, per_class), flush=True)
    first = device_ms(lambda: det.run_tiled(union, d_geom, n_tiles, thr, 0.3), 1, 1)
    if first[0] > args.tail_limit_ms:
        line("y3_detect_tiled, %d candidates, %d kept (one call)" % (n_cand, int(det.count[0].item())), first, 1, 1)
        print("the tail alone takes longer than --tail-limit-ms: the whole call is not timed in this regime", flush=True)
        return
    ms = device_ms(lambda: det.run_tiled(union, d_geom, n_tiles, thr, 0.3), args.passes, args.iters)
    line("y3_detect_tiled, %d rows, %d candidates, %d kept" % (n_tiles * rows, n_cand, int(det.count[0].item())), ms,
         args.passes, args.iters)

    if args.merge is not None:
        # the merge launch alone, on the detections the tail has just left in the Detector's buffers
        merge = tiles.check_merge(args.merge)
        mb = _MergeBuffers(1, n_tiles * rows, dev)

        def merge_launch():
            _hip.check(_hip.lib().y3_merge_tiled(
                det.count.data_ptr(), det.tlbr.data_ptr(), det.prob.data_ptr(), det.cls.data_ptr(), det.row.data_ptr(), 1,
                n_tiles * rows, rows, ctypes.c_double(merge), mb.ws.data_ptr(), mb.ws_bytes, mb.count.data_ptr(), mb.tlbr.data_ptr(),
                mb.prob.data_ptr(), mb.cls.data_ptr(), mb.row.data_ptr(), mb.members.data_ptr(), _hip.stream_ptr()))
        ms_merge = device_ms(merge_launch, args.passes, args.iters)
        kept_in, kept_out = int(det.count[0].item()), int(mb.count[0].item())
        per_class = int(torch.bincount(det.cls[0, :kept_in].clamp(min=0)).max().item()) if kept_in else 0
        line("y3_merge_tiled at %g, %d detections (%d in the largest class) -> %d, largest group %d" % (
            merge, kept_in, per_class, kept_out, int(mb.members[0, :kept_out].max().item()) if kept_out else 0), ms_merge,
            args.passes, args.iters)
        print("the merge launch takes %.2f of the y3_detect_tiled launch in front of it" % (
            statistics.median(ms_merge) / statistics.median(ms)), flush=True)

    def timed_call(merge):
        def call():
            return yolov3.inference(net, frame, device="cuda:0", prob_thresh=args.thresh, tile_overlap=args.overlap,
                                    tile_batch=args.tile_batch, **({} if merge is None else {"tile_merge": merge}))
        call()
        wall = []
        for _ in range(args.passes):
            t0 = time.perf_counter()
            for _ in range(args.iters):
                kept = len(call()[0][1])
            wall.append((time.perf_counter() - t0) / args.iters * 1e3)
        line("inference(tile_overlap=%g%s), host frame to host detections (%d)" % (
            args.overlap, "" if merge is None else ", tile_merge=%g" % merge, kept), wall, args.passes, args.iters)
    timed_call(None)
    if args.merge is not None:
        timed_call(args.merge)

    def plain():
        return yolov3.inference(net, frame, device="cuda:0", prob_thresh=args.thresh)
    plain()
    wall = []
    for _ in range(args.passes):
        t0 = time.perf_counter()
        for _ in range(args.iters):
            kept = len(plain()[0][1])
        wall.append((time.perf_counter() - t0) / args.iters * 1e3)
    line("inference() without tiling, the same frame (%d)" % kept, wall, args.passes, args.iters)


if __name__ == "__main__":
    main()
