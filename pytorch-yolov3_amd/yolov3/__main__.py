"""``python -m yolov3``: the reference's command line (/root/reference/yolov3/__main__.py:36-212)
over the HIP path -- same flags and meanings; frames are processed in batches
(``--batch-size``), detections can be dumped as COCO JSON (``--json``), and annotated frames
are written to ``--output`` (a directory of PNGs; an .mp4 needs OpenCV).  There is no window
output without OpenCV and no CPU mode: ``-d cpu`` is refused instead of silently running
something else than the GPU path.
"""
import argparse
import json
import os
import pathlib
import sys
import time


# (flags, keyword arguments) per option; the flag names and defaults are the reference CLI's -- they are the interface a
# user of `yolov3 ...` already knows -- the batching / dtype / json options are this build's additions
_SOURCE_OPTIONS = [
    (("-C", "--cam"), dict(metavar="cam_id", nargs="?", const=0,
                           help="live capture: device number (0 when given bare) or a stream path")),
    (("-I", "--image"), dict(type=pathlib.Path, metavar="<path>", help="one image, or a folder whose images are all run")),
    (("-V", "--video"), dict(type=pathlib.Path, metavar="<path>", help="a video file, or a folder of frames")),
]
_MODEL_OPTIONS = [
    (("-c", "--config"), dict(type=pathlib.Path, required=True, metavar="<path>", help="Darknet .cfg of the network (required)")),
    (("-w", "--weights"), dict(type=pathlib.Path, required=True, metavar="<path>", help="Darknet .weights file (required)")),
    (("-d", "--device"), dict(type=str, default="cuda", metavar="<device>", help="'cuda' or 'cuda:N' (default cuda)")),
    (("-p", "--prob-thresh"), dict(type=float, default=0.05, metavar="<prob>", help="keep detections scoring at least this (default 0.05)")),
    (("-i", "--iou-thresh"), dict(type=float, default=0.3, metavar="<iou>", help="NMS overlap above which the weaker box goes (default 0.3)")),
    (("-n", "--class-names"), dict(type=pathlib.Path, metavar="<path>", help="text file, one class name per line; labels show indices without it")),
    (("--dtype",), dict(default="float32", choices=["float32", "fp16", "bf16"], help="conv arithmetic: float32 (the reference's; default, boxes and scores within 1e-3 of its CPU path), fp16 or bf16 storage with float32 accumulation (about 7x the frames/s; scores within ~1e-3 / ~1e-2)")),
    (("-b", "--batch-size"), dict(type=int, default=16, metavar="<n>", help="frames per GPU batch for folders and videos (default 16)")),
    (("--letterbox",), dict(action="store_true", help="Darknet letterboxing: keep each frame's aspect ratio and fill the rest of the network input with grey (128) instead of stretching the frame; use it with yolov4-csp, which was trained that way")),
    (("--darknet-resize",), dict(action="store_true", help="prepare every frame the way Darknet itself does: byte / 255 first, then Darknet's float32 resize_image (align-corners geometry) instead of the 8-bit bilinear resize; with --letterbox its letterbox_image, padded with 0.5 instead of the byte 128")),
    (("--darknet-pool",), dict(action="store_true", help="Darknet max-pooling (centred windows, out-of-range taps ignored) instead of the reference's; use it with weights trained by Darknet for yolov3-spp, yolov4 and yolov4-csp (the latter together with --letterbox)")),
    (("--nms-kind",), dict(choices=["iou", "greedynms", "diounms"], default=None, help="suppress by Darknet's rule on the float32 boxes instead of the reference's on integer pixel corners: iou (a cfg without nms_kind), greedynms (yolov4.cfg) or diounms (yolov4-csp.cfg); -i is its threshold (Darknet's own defaults are -p 0.25 -i 0.45)")),
    (("--darknet-scores",), dict(action="store_true", help="score every class of a box by Darknet's independent logistic, sigmoid(obj) * sigmoid(class), instead of the reference's soft-max over the classes; use it with weights trained by Darknet for yolov3, yolov3-tiny, yolov3-spp, yolov4 and yolov4-tiny (yolov4-csp scores that way already)")),
    (("--multi-label",), dict(action="store_true", help="report every class of a box that scores above -p, as Darknet does, not the best class only (a box may then appear once per class); implies --darknet-scores")),
    (("--tile-overlap",), dict(type=float, default=None, metavar="<fraction>", help="tiled inference for images larger than the network (-I only): cut every image into network-sized tiles at full resolution whose neighbours share at least this fraction (0 .. 0.9) of the network size, run them all and suppress over their union; objects too small to survive the resize are found, objects cut by a tile border may come out as partial boxes unless --tile-merge is given")),
    (("--tile-merge",), dict(type=float, default=None, metavar="<threshold>", help="with --tile-overlap: merge detections of one class from different tiles whose intersection over the smaller box exceeds this threshold (0 .. 1; 0.5 is a reasonable start) into one detection with their union box, so that an object cut by a tile border is reported once")),
    (("--no-tile-overview",), dict(action="store_true", help="with --tile-overlap: leave out the extra tile that holds the whole image resized to the network (it finds objects larger than a tile)")),
    (("--beta-nms",), dict(type=float, default=0.6, metavar="<beta>", help="exponent of the distance penalty of --nms-kind diounms (default 0.6, the cfgs' beta_nms)")),
]
_OUTPUT_OPTIONS = [
    (("-o", "--output"), dict(type=pathlib.Path, metavar="<path>", help="annotated frames: a folder of PNGs, or an .mp4 when OpenCV is installed")),
    (("--json",), dict(type=pathlib.Path, metavar="<path>", help="dump every detection as COCO-format JSON")),
    (("--show-fps",), dict(action="store_true", help="overlay the frame rate (camera mode)")),
    (("-v", "--verbose"), dict(action="store_true", help="print device and throughput")),
]


def build_parser():
    parser = argparse.ArgumentParser(prog="yolov3", description="YOLOv3 detection on an MI355X (HIP path)")
    source = parser.add_argument_group(title="input (exactly one)").add_mutually_exclusive_group(required=True)
    for flags, kw in _SOURCE_OPTIONS:
        source.add_argument(*flags, **kw)
    model = parser.add_argument_group(title="model")
    for flags, kw in _MODEL_OPTIONS:
        model.add_argument(*flags, **kw)
    output = parser.add_argument_group(title="output")
    for flags, kw in _OUTPUT_OPTIONS:
        output.add_argument(*flags, **kw)
    return parser


def _abspath(p):
    return None if p is None else str(pathlib.Path(p).expanduser().absolute())


def _write_frames(frames, fps, path):
    """``-o``: .mp4 like the reference's write_mp4 (__main__.py:13-33) when OpenCV is there; .avi (Motion JPEG) / .y4m
    through this package's own writers; anything else is taken as a directory of PNG frames."""
    from .stream import _cv2
    cv2 = _cv2()
    if path.endswith(".mp4"):
        if cv2 is None:
            raise RuntimeError("writing .mp4 needs OpenCV (cv2), which is not installed; give a .avi (Motion JPEG) or "
                               ".y4m file name or a directory instead")
        h, w = frames[0].shape[:2]
        writer = cv2.VideoWriter(path, cv2.VideoWriter_fourcc(*"mp4v"), int(fps), (w, h))
        for frame in frames:
            writer.write(frame)
        writer.release()
        return
    if path.lower().endswith((".avi", ".y4m")):
        from .videoio import write_video
        write_video(path, frames, fps)
        return
    from PIL import Image
    os.makedirs(path, exist_ok=True)
    for i, frame in enumerate(frames):
        Image.fromarray(frame[:, :, ::-1]).save(os.path.join(path, "frame_%06d.png" % i))


def check_tiling(args):
    """``--tile-overlap`` (and ``--tile-merge``, which needs it) and what it does not combine with: SystemExit before anything is loaded.  args: the parsed options."""
    if args["tile_overlap"] is None:
        if args["no_tile_overview"]:
            raise SystemExit("yolov3: --no-tile-overview means nothing without --tile-overlap")
        if args["tile_merge"] is not None:
            raise SystemExit("yolov3: --tile-merge means nothing without --tile-overlap")
        return
    if not args["image"]:
        raise SystemExit("yolov3: --tile-overlap refused with video or camera input -- tiled inference runs on images (-I) only")
    from .tiles import check_options
    try:
        check_options(args["tile_overlap"], letterbox=args["letterbox"], preprocess="darknet" if args["darknet_resize"] else None,
                      nms_kind=args["nms_kind"], multi_label=args["multi_label"])
    except ValueError as exc:
        raise SystemExit("yolov3: --tile-overlap refused: %s" % exc)
    if args["tile_merge"] is not None:
        from .tiles import check_merge
        try:
            check_merge(args["tile_merge"])
        except ValueError as exc:
            raise SystemExit("yolov3: --tile-merge refused: %s" % exc)


def main(argv=None):
    args = vars(build_parser().parse_args(argv))
    check_tiling(args)
    for key in ("class_names", "config", "weights", "image", "video", "output", "json"):
        args[key] = _abspath(args[key])
    device = args["device"]
    if not device.startswith("cuda"):
        raise SystemExit("yolov3: device %r refused -- this build has no CPU path (the reference's `-d cpu` mode "
                         "is PyTorch-CPU; use the reference for that)" % device)

    import yolov3
    from yolov3 import stream

    net = yolov3.Darknet(args["config"], device=device, dtype=args["dtype"],
                         pool="darknet" if args["darknet_pool"] else "reference",
                         scores="darknet" if args["darknet_scores"] or args["multi_label"] else "reference",
                         multi_label=args["multi_label"])
    net.load_weights(args["weights"])
    net.eval()
    net.cuda(device=device)
    if args["verbose"]:
        import torch
        print("Running model on %s" % torch.cuda.get_device_name(net._torch_device()))

    class_names = None
    if args["class_names"] is not None and os.path.isfile(args["class_names"]):
        with open(args["class_names"], "r") as fh:
            class_names = [line.strip() for line in fh.readlines()]

    frames = [] if args["output"] else None
    preprocess = "darknet" if args["darknet_resize"] else None
    names, results, fps = None, None, 25.0
    t0 = time.time()
    if args["image"]:
        directory, names = stream.list_image_files(args["image"])
        images = [stream.load_image_bgr(os.path.join(directory, n)) for n in names]
        if args["tile_overlap"] is not None:
            results = [tuple(yolov3.inference(net, image, device=device, prob_thresh=args["prob_thresh"],
                                              nms_iou_thresh=args["iou_thresh"], tile_overlap=args["tile_overlap"],
                                              tile_overview=not args["no_tile_overview"], tile_batch=args["batch_size"],
                                              tile_merge=args["tile_merge"])[0])
                       for image in images]
        else:
            results = list(stream.detect_in_frames(net, images, batch_size=args["batch_size"],
                                                   prob_thresh=args["prob_thresh"], nms_iou_thresh=args["iou_thresh"],
                                                   letterbox=args["letterbox"], nms_kind=args["nms_kind"],
                                                   beta_nms=args["beta_nms"], preprocess=preprocess))
        if frames is not None:
            for image, (bbox_tlbr, class_prob, class_idx) in zip(images, results):
                stream.draw_boxes(image, bbox_tlbr, class_idx=class_idx, class_names=class_names)
                frames.append(image)
    elif args["video"]:
        fps = stream.video_fps(args["video"], fps)
        results = stream.detect_in_video(net, args["video"], device=device, prob_thresh=args["prob_thresh"],
                                         nms_iou_thresh=args["iou_thresh"], class_names=class_names,
                                         frames=frames, show_video=False, batch_size=args["batch_size"],
                                         letterbox=args["letterbox"], nms_kind=args["nms_kind"], beta_nms=args["beta_nms"],
                                         preprocess=preprocess)
        names = ["frame_%06d" % i for i in range(len(results))]
    else:
        cam = args["cam"]
        if isinstance(cam, str) and cam.isdigit():
            cam = int(cam)
        stream.detect_in_cam(net, cam_id=cam, device=device, prob_thresh=args["prob_thresh"],
                             nms_iou_thresh=args["iou_thresh"], class_names=class_names,
                             show_fps=args["show_fps"], frames=frames, letterbox=args["letterbox"],
                             nms_kind=args["nms_kind"], beta_nms=args["beta_nms"], preprocess=preprocess)
    elapsed = time.time() - t0
    if results is not None and args["verbose"]:
        kept = sum(len(r[1]) for r in results)
        print("%d frames, %d detections, %.1f frames/s (decode + upload + GPU + fetch)" % (
            len(results), kept, len(results) / max(elapsed, 1e-9)))
    if args["json"] and results is not None:
        categories = class_names
        if categories is None:
            top = max([int(r[2].max()) for r in results if len(r[2])] + [0])
            categories = [str(i) for i in range(top + 1)]
        with open(args["json"], "w") as fh:
            json.dump(stream.to_coco(names, results, categories), fh)
    if args["output"] and frames:
        _write_frames(frames, fps, args["output"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
