"""Post-processing entry points with the reference's signatures, computed on the GPU.

``cxywh_to_tlbr``, ``non_max_suppression`` and ``inference`` mirror
/root/reference/yolov3/inference.py:220-368.  Differences that callers can observe:

* kept indices / detections come out in a canonical order (class ascending, score
  descending, then higher index first) instead of the reference's Python-``set`` /
  ``argsort`` dependent order -- the *set* of kept boxes is identical;
* ``inference()`` runs threshold, scaling, integer truncation, corner conversion and
  per-class NMS in one device kernel per batch (libyolov3_hip ``y3_detect``) and copies
  only the surviving detections back to the host;
* frames that are not net-sized are resized on the GPU (``y3_resize_bilinear_u8``, bit-identical to
  ``preprocess.resize_bilinear_u8``; the reference uses ``cv2.resize``, see that module's docstring);
* ``letterbox=True`` (opt-in, not in the reference) letterboxes the frames the Darknet way instead of stretching them
  (``y3_letterbox_u8``, bit-identical to ``preprocess.letterbox_u8``) and corrects the boxes back to the frame
  (``y3_detect_letterbox``, the same as ``preprocess.correct_letterbox_boxes`` followed by the reference's tail);
* ``nms_kind="iou" | "greedynms" | "diounms"`` (opt-in, not in the reference) chooses the survivors by Darknet's rule on the
  float32 centre / size boxes (``y3_detect_darknet``; include/yolov3_hip.h states the rule) instead of the reference's on
  integer pixel corners; everything else about a detection stays.  ``non_max_suppression_darknet`` is that rule on
  caller-provided boxes;
* a network built with ``multi_label=True`` (opt-in, not in the reference) reports every class of a box whose Darknet score
  ``sigmoid(obj) * sigmoid(class_c)`` is ``>`` the threshold, not the arg-max class only: ``y3_expand_labels`` turns the
  head outputs into one candidate per (box, class) and the detection tail runs on those unchanged, so a box may appear once
  per class and a box's second class takes part in that class's suppression;
* ``preprocess="darknet"`` (opt-in, not in the reference) prepares the frames the way Darknet itself does: ``byte / 255`` first,
  then Darknet's float32 ``resize_image`` (or ``letterbox_image`` on a canvas of 0.5 with ``letterbox=True``) in one launch per
  batch (``y3_preprocess_darknet_f32``), and the network runs from that float input instead of the fused uint8 stem;
* ``tile_overlap=f`` (opt-in, not in the reference) looks at a frame larger than the network through net-sized windows at full
  resolution (``yolov3/tiles.py``): the windows are cut on the device (``y3_tiles_u8``), run through the network in chunks, and
  all their rows are one frame's candidates, each mapped back by its window's origin, before one suppression (``y3_detect_tiled``);
* ``tile_merge=t`` (opt-in, with ``tile_overlap`` only; not in the reference) adds the seam merge after that suppression
  (``y3_merge_tiled``, one more launch on the same stream): detections of one class from DIFFERENT tiles whose intersection over
  the smaller area exceeds ``t`` become one detection with their union box, so an object cut by a tile border is reported once.
  ``tiles.merge_detections`` is the same rule in numpy.

There is no CPU fallback: without the HIP library / a GPU these functions raise.
"""
import ctypes

import numpy as np
import torch

from . import _hip, tiles as _tiles
from .preprocess import _fill_byte, darknet_frames_device, letterbox_frames_device, prepare_frames_device, resize_on_device


def _device(device=None):
    _hip.require_gpu()
    if device is None or str(device) == "cuda":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _float_kind(dtype):
    """numpy float dtype -> (C ABI element type, numpy dtype the kernel computes in): float32 and float64 boxes are computed
    in their own type, step by step as numpy does.  float16 boxes are REFUSED: the reference would compute areas and IoU in
    float16 (a 300 x 300 box's area overflows to inf there), which the float32 kernel would silently not reproduce
    (ADVICE r05); wider floats (longdouble) go through float64."""
    if dtype == np.float16:
        raise TypeError("float16 boxes are not supported: numpy would compute areas and IoU in float16 (overflow above 255 x 255 "
                        "pixels); pass float32 / float64 or integer boxes")
    if dtype == np.float64 or dtype.itemsize > 8:
        return _hip.Y3_F64, np.float64
    return _hip.Y3_F32, np.float32


def _require_finite(arr, what):
    """NaN / inf coordinates: numpy's maximum / minimum propagate NaN and ``inf // 2`` is NaN there, the device kernels
    compare and floor instead -- refuse rather than return a different keep set."""
    if not np.isfinite(arr).all():
        raise ValueError("{} holds non-finite values (NaN / inf): not supported on float boxes".format(what))


def _run_nms(dev, ws_query, call, boxes, prob, cls):
    """The device side that the NMS wrappers share.  Uploads ``boxes``, ``prob`` and the optional ``cls`` (host arrays that the
    caller has validated) to ``dev``, makes the workspace that ``ws_query(n)`` asks for and the keep / count buffers, and runs
    ``call(d_boxes, d_prob, d_cls, n, tail)`` on ``dev``: device pointers (``d_cls`` may be None) and ``tail``, the arguments
    every NMS entry point ends with (workspace, its size, keep, count, stream).  Returns the kept indices as a list."""
    n = boxes.shape[0]
    d_box = torch.from_numpy(boxes).to(dev)
    d_prob = torch.from_numpy(prob).to(dev)
    d_cls = torch.from_numpy(cls).to(dev) if cls is not None else None
    ws_bytes = ws_query(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    keep = torch.empty(n, dtype=torch.int64, device=dev)
    count = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        tail = (ws.data_ptr(), ws_bytes, keep.data_ptr(), count.data_ptr(), _hip.stream_ptr())
        _hip.check(call(d_box.data_ptr(), d_prob.data_ptr(), d_cls.data_ptr() if d_cls is not None else None, n, tail))
        return keep[:int(count.cpu()[0])].cpu().numpy().tolist()


def cxywh_to_tlbr(bbox_xywh):
    """(n, >=4) array [cx, cy, w, h, ...] -> [x1, y1, x2, y2, ...] with ``x1 = cx - w//2`` etc. (floor division; extra
    columns pass through).  Integer pixel boxes (what ``inference()`` uses) and float32 / float64 boxes, like the reference
    (inference.py:269-283: ``//`` is numpy's floor division in the array's dtype)."""
    arr = np.asarray(bbox_xywh)
    if arr.ndim != 2 or arr.shape[1] < 4:
        raise ValueError("expected an (n, >=4) array")
    if np.issubdtype(arr.dtype, np.floating):
        if arr.shape[0] == 0:
            return arr.copy()
        code, work = _float_kind(arr.dtype)
        _require_finite(arr, "bbox_xywh")
        dev = _device()
        src = torch.from_numpy(np.ascontiguousarray(arr, dtype=work)).to(dev)
        dst = torch.empty_like(src)
        _hip.check(_hip.lib().y3_cxywh_to_tlbr_float(src.data_ptr(), dst.data_ptr(), arr.shape[0], arr.shape[1], code, _hip.stream_ptr()))
        return dst.cpu().numpy().astype(arr.dtype, copy=False)
    if not np.issubdtype(arr.dtype, np.integer):
        raise TypeError("cxywh_to_tlbr works on integer or floating-point boxes, got dtype {}".format(arr.dtype))
    if arr.shape[0] == 0:
        return arr.copy()
    dev = _device()
    src = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int64)).to(dev)
    dst = torch.empty_like(src)
    _hip.check(_hip.lib().y3_cxywh_to_tlbr(src.data_ptr(), dst.data_ptr(), arr.shape[0], arr.shape[1],
                                           _hip.stream_ptr()))
    return dst.cpu().numpy().astype(arr.dtype, copy=False)


def non_max_suppression(bbox_tlbr, class_prob, class_idx=None, iou_thresh=0.3):
    """Greedy NMS; per class when ``class_idx`` is given.  Returns a list of kept indices.

    Same decision rule as the reference (areas with +1, suppress iff IoU > iou_thresh, highest score first).  INTEGER pixel
    corners -- what ``inference()`` feeds it (inference.py:353-355) -- take the int64 device kernel (IoU = int / int in
    float64, like numpy); float32 / float64 boxes (normalised or sub-pixel coordinates: any caller of the public function)
    take ``y3_nms_float``, which computes every step in the array's dtype as numpy does (round 5).
    """
    barr = np.asarray(bbox_tlbr)
    if barr.size and np.issubdtype(barr.dtype, np.floating):
        return _nms_float(barr, class_prob, class_idx, iou_thresh)
    if barr.size and not np.issubdtype(barr.dtype, np.integer):
        raise TypeError("non_max_suppression works on integer or floating-point boxes, got dtype {}".format(barr.dtype))
    boxes = np.ascontiguousarray(np.asarray(bbox_tlbr)[:, :4] if np.asarray(bbox_tlbr).size else
                                 np.zeros((0, 4)), dtype=np.int64)
    prob = np.ascontiguousarray(class_prob, dtype=np.float32)
    n = boxes.shape[0]
    if prob.shape[0] != n:
        raise ValueError("bbox_tlbr and class_prob disagree on the number of boxes")
    if n == 0:
        return []
    dev = _device()
    lib = _hip.lib()
    cls = None
    if class_idx is not None:
        cls = np.ascontiguousarray(class_idx, dtype=np.int64)
        if cls.shape[0] != n:
            raise ValueError("class_idx has the wrong length")
    thr = float(iou_thresh)
    return _run_nms(dev, lib.y3_nms_workspace_bytes,
                    lambda box, score, cidx, n, tail: lib.y3_nms(box, score, cidx, n, thr, *tail), boxes, prob, cls)


def non_max_suppression_darknet(bbox_xywh, class_prob, class_idx=None, thresh=0.45, nms_kind="iou", beta_nms=0.6):
    """Greedy NMS by Darknet's rule on float32 centre / size boxes ``[x, y, w, h]``; per class when ``class_idx`` is given.
    Returns the kept indices in canonical order (class ascending, score descending, higher index first).

    ``nms_kind``: "iou" (what a cfg without ``nms_kind`` gets), "greedynms" (IoU minus the DIoU penalty d / c) or "diounms"
    (IoU - (d / c) ** beta_nms); a suppresses b iff the measure is > ``thresh`` in float32 (include/yolov3_hip.h,
    ``y3_detect_darknet``, states every operation).  The boxes must BE float32: float64 (and float16, and integers) are
    refused, not rounded, because the rule is defined on the float32 values.
    """
    mode = _hip.nms_mode(nms_kind, beta_nms)
    if mode is None:
        raise ValueError("nms_kind=None is the reference's rule: non_max_suppression() computes it")
    barr = np.asarray(bbox_xywh)
    if barr.dtype != np.float32:
        raise TypeError("non_max_suppression_darknet works on float32 boxes (Darknet's rule is float32 arithmetic), got dtype {}; "
                        "convert explicitly if rounding them is what you mean".format(barr.dtype))
    if barr.size == 0:
        barr = barr.reshape(0, 4)
    if barr.ndim != 2 or barr.shape[1] < 4:
        raise ValueError("expected an (n, >=4) array of [x, y, w, h] boxes")
    _require_finite(barr[:, :4], "bbox_xywh")
    boxes = np.ascontiguousarray(barr[:, :4])
    prob = np.ascontiguousarray(class_prob, dtype=np.float32)
    n = boxes.shape[0]
    if prob.ndim != 1 or prob.shape[0] != n:
        raise ValueError("bbox_xywh and class_prob disagree on the number of boxes")
    cls = None
    if class_idx is not None:
        cls = np.ascontiguousarray(class_idx, dtype=np.int64)
        if cls.ndim != 1 or cls.shape[0] != n:
            raise ValueError("class_idx has the wrong length")
    thresh = float(np.float32(thresh))
    if n == 0:
        return []
    dev = _device()
    _hip.require_capabilities(_hip.CAP_NMS_DARKNET, "non_max_suppression_darknet")
    lib = _hip.lib()
    return _run_nms(dev, lib.y3_nms_darknet_workspace_bytes,
                    lambda box, score, cidx, n, tail: lib.y3_nms_darknet(box, score, cidx, n, thresh, mode[0], mode[1], *tail),
                    boxes, prob, cls)


def _nms_float(barr, class_prob, class_idx, iou_thresh):
    code, work = _float_kind(barr.dtype)
    _require_finite(barr[:, :4], "bbox_tlbr")
    boxes = np.ascontiguousarray(barr[:, :4], dtype=work)
    prob = np.ascontiguousarray(class_prob, dtype=np.float64)
    n = boxes.shape[0]
    if prob.shape[0] != n:
        raise ValueError("bbox_tlbr and class_prob disagree on the number of boxes")
    dev = _device()
    lib = _hip.lib()
    cls = None
    if class_idx is not None:
        cls = np.ascontiguousarray(class_idx, dtype=np.int64)
        if cls.shape[0] != n:
            raise ValueError("class_idx has the wrong length")
    thr = float(iou_thresh)
    return _run_nms(dev, lib.y3_nms_float_workspace_bytes,
                    lambda box, score, cidx, n, tail: lib.y3_nms_float(box, code, score, cidx, n, thr, *tail), boxes, prob, cls)


class Detector(object):
    """Reusable device buffers for the detection tail of one (batch, rows) shape."""

    def __init__(self, batch, rows, device):
        lib = _hip.lib()
        self.batch, self.rows, self.device = batch, rows, device
        self.ws_bytes = lib.y3_detect_workspace_bytes(batch, rows)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.count = torch.zeros(batch, dtype=torch.int32, device=device)
        self.tlbr = torch.empty((batch, rows, 4), dtype=torch.int64, device=device)
        self.prob = torch.empty((batch, rows), dtype=torch.float32, device=device)
        self.cls = torch.empty((batch, rows), dtype=torch.int64, device=device)
        self.row = torch.empty((batch, rows), dtype=torch.int32, device=device)
        self.orig_hw = torch.empty((batch, 2), dtype=torch.int32, device=device)
        self._records = {}      # kmax -> (batch, kmax, 8) int32 staging buffer of fetch()
        self._ws_darknet = None  # (bytes, tensor): the larger workspace of y3_detect_darknet, made when first asked for
        self._labels = {}        # capacity -> _LabelBuffers of multi-label runs
        self._tail = self        # the Detector that holds the last run's detections (another one for a capacity != rows)
        self._label_run = None   # multi-label: the _LabelBuffers of the last run, whose true counts fetch() checks
        self._merge = None       # _MergeBuffers of run_tiled(merge=...), made when first asked for
        self._merge_run = None   # ... when the last run merged: what fetch() then reports

    def run(self, out, orig_hw, prob_thresh, iou_thresh, letterbox=None, nms_kind=None, beta_nms=0.6, labels=None,
            label_capacity=None):
        """out: Darknet.forward dict (device tensors).  orig_hw: (batch,2) int32 tensor/array.  letterbox: the
        (net_h, net_w) the frames were letterboxed into -- the boxes are then corrected back (``y3_detect_letterbox``).
        nms_kind: None = the reference's suppression rule; "iou" / "greedynms" / "diounms" = Darknet's, on the float32
        boxes (``y3_detect_darknet``; with ``letterbox``, on the corrected ones), ``beta_nms`` for "diounms".
        labels: None, or the ``y3_head_view`` array of the forward that made ``out`` (``Darknet.label_heads()``): Darknet's
        multi-label detections.  Every (box, class) whose score is > ``prob_thresh`` becomes a candidate
        (``y3_expand_labels``), at most ``label_capacity`` per frame (default: the number of prediction rows), and the
        tail chosen by the other arguments runs on those; the rows reported are the real prediction rows.  A frame with
        more labels than the capacity is an error raised by ``fetch`` (``check_label_capacity``), never a truncation."""
        mode = _hip.nms_mode(nms_kind, beta_nms)
        if labels is not None:
            return self._run_labels(out, orig_hw, prob_thresh, iou_thresh, letterbox, nms_kind, beta_nms, labels, label_capacity)
        self._tail, self._label_run, self._merge_run = self, None, None
        if not isinstance(orig_hw, torch.Tensor):
            orig_hw = torch.from_numpy(np.ascontiguousarray(orig_hw, dtype=np.int32))
        if (orig_hw.device == self.orig_hw.device and orig_hw.dtype == torch.int32 and orig_hw.is_contiguous()
                and tuple(orig_hw.shape) == (self.batch, 2)):
            hw = orig_hw                       # already resident: no staging copy on the launch path
        else:
            self.orig_hw.copy_(orig_hw, non_blocking=True)
            hw = self.orig_hw
        bbox, prob, cls = out["bbox_xywh"], out["class_prob"], out["class_idx"]
        lib = _hip.lib()
        if mode is not None:
            _hip.require_capabilities(_hip.CAP_NMS_DARKNET, "Detector.run(nms_kind=...)")
        if letterbox is not None:
            _hip.require_capabilities(_hip.CAP_LETTERBOX, "Detector.run(letterbox=...)")
        ws, ws_bytes = self.ws, self.ws_bytes
        if mode is not None:
            if self._ws_darknet is None:
                nbytes = lib.y3_detect_darknet_workspace_bytes(self.batch, self.rows)
                self._ws_darknet = (nbytes, torch.empty(nbytes, dtype=torch.uint8, device=self.device))
            ws_bytes, ws = self._ws_darknet
        args = [bbox.data_ptr(), prob.data_ptr(), cls.data_ptr(), self.batch, self.rows, hw.data_ptr(),
                ctypes.c_float(prob_thresh), ctypes.c_double(iou_thresh), ws.data_ptr(), ws_bytes,
                self.count.data_ptr(), self.tlbr.data_ptr(), self.prob.data_ptr(), self.cls.data_ptr(),
                self.row.data_ptr()]
        net_h, net_w = (int(v) for v in letterbox) if letterbox is not None else (0, 0)
        if mode is not None:
            _hip.check(lib.y3_detect_darknet(*args, net_h, net_w, mode[0], ctypes.c_float(mode[1]), _hip.stream_ptr()))
        elif letterbox is not None:
            _hip.check(lib.y3_detect_letterbox(*args, net_h, net_w, _hip.stream_ptr()))
        else:
            _hip.check(lib.y3_detect(*args, _hip.stream_ptr()))

    def run_tiled(self, out, geom, tiles, prob_thresh, iou_thresh, merge=None):
        """The detection tail over frames that were run as tiles (``y3_detect_tiled``).  out: forward outputs of
        ``batch * tiles`` tiles, frame by frame (device tensors).  geom: ``y3_tile_geom`` of every tile in that order -- a uint8
        device tensor of 16 bytes per tile, or a list of (sx, sy, ox, oy).  This Detector's ``rows`` is the capacity of a frame,
        ``tiles`` times the rows of a tile, and the rows ``fetch`` reports are combined rows, tile * rows of a tile + row.  The
        reference's suppression only: no letterbox correction, no Darknet kinds, no multi-label rows.
        merge: None, or the seam-merge threshold in [0, 1]: ``y3_merge_tiled`` then runs after the tail, on the same stream, into
        buffers of its own (made on first use); ``fetch`` reports the merged detections and ``members`` how many detections each
        one stands for.  The unmerged detections stay in ``count`` / ``tlbr`` / ``prob`` / ``cls`` / ``row``.  The merge buffers
        (outputs, members and workspace at full capacity, about 68 bytes per slot) stay with this Detector once made: a later
        ``merge=None`` run allocates nothing and launches nothing more, but does not free them either."""
        _hip.require_capabilities(_hip.CAP_TILES, "Detector.run_tiled")
        if merge is not None:
            merge = _tiles.check_merge(merge)
            _hip.require_capabilities(_hip.CAP_TILE_MERGE, "Detector.run_tiled(merge=...)")
        bbox, prob, cls = out["bbox_xywh"], out["class_prob"], out["class_idx"]
        tiles = int(tiles)
        if tiles < 1 or self.rows % tiles or tuple(prob.shape) != (self.batch * tiles, self.rows // tiles):
            raise ValueError("Detector of batch {} and {} rows given {} tiles a frame and outputs of shape {}".format(
                self.batch, self.rows, tiles, tuple(prob.shape)))
        if not (bbox.is_contiguous() and prob.is_contiguous() and cls.is_contiguous()):
            raise ValueError("Detector.run_tiled: the outputs must be contiguous")
        if not isinstance(geom, torch.Tensor):
            geom = tile_geom_tensor(geom, self.device)
        if geom.dtype != torch.uint8 or geom.numel() != 16 * self.batch * tiles or not geom.is_contiguous():
            raise ValueError("Detector.run_tiled: expected {} tile geometries of 16 bytes".format(self.batch * tiles))
        self._tail, self._label_run, self._merge_run = self, None, None
        self._geom = geom                                   # alive until the next run
        _hip.check(_hip.lib().y3_detect_tiled(
            bbox.data_ptr(), prob.data_ptr(), cls.data_ptr(), self.batch, tiles, self.rows // tiles, geom.data_ptr(),
            ctypes.c_float(prob_thresh), ctypes.c_double(iou_thresh), self.ws.data_ptr(), self.ws_bytes, self.count.data_ptr(),
            self.tlbr.data_ptr(), self.prob.data_ptr(), self.cls.data_ptr(), self.row.data_ptr(), _hip.stream_ptr()))
        if merge is not None:
            mb = self._merge
            if mb is None:
                mb = self._merge = _MergeBuffers(self.batch, self.rows, self.device)
            _hip.check(_hip.lib().y3_merge_tiled(
                self.count.data_ptr(), self.tlbr.data_ptr(), self.prob.data_ptr(), self.cls.data_ptr(), self.row.data_ptr(),
                self.batch, self.rows, self.rows // tiles, ctypes.c_double(merge), mb.ws.data_ptr(), mb.ws_bytes,
                mb.count.data_ptr(), mb.tlbr.data_ptr(), mb.prob.data_ptr(), mb.cls.data_ptr(), mb.row.data_ptr(),
                mb.members.data_ptr(), _hip.stream_ptr()))
            self._merge_run = mb

    @property
    def members(self):
        """After ``run_tiled(merge=...)``: the (batch, rows) int32 device tensor whose first ``count`` entries of a frame say how
        many detections each merged detection stands for (1 = nothing absorbed); None after any other run."""
        tail = self._tail
        return tail._merge_run.members if tail._merge_run is not None else None

    def _run_labels(self, out, orig_hw, prob_thresh, iou_thresh, letterbox, nms_kind, beta_nms, labels, label_capacity):
        _hip.require_capabilities(_hip.CAP_MULTI_LABEL, "Detector.run(labels=...)")
        bbox = out["bbox_xywh"]
        batch, rows_total = int(bbox.shape[0]), int(bbox.shape[1])
        if batch != self.batch:
            raise ValueError("Detector of batch {} given outputs of batch {}".format(self.batch, batch))
        cap = int(label_capacity) if label_capacity is not None else self.rows
        if cap < 1:
            raise ValueError("label_capacity must be >= 1, got {!r}".format(label_capacity))
        lb = self._labels.get((cap, rows_total))
        if lb is None:
            lb = self._labels[(cap, rows_total)] = _LabelBuffers(self.batch, rows_total, cap, self.device)
            lb.tail = self if cap == self.rows else Detector(self.batch, cap, self.device)
        _hip.check(_hip.lib().y3_expand_labels(
            labels, len(labels), bbox.data_ptr(), self.batch, rows_total, ctypes.c_float(prob_thresh), cap, lb.ws.data_ptr(),
            lb.ws_bytes, lb.vbbox.data_ptr(), lb.vprob.data_ptr(), lb.vcls.data_ptr(), lb.vrow.data_ptr(), lb.vcount.data_ptr(),
            _hip.stream_ptr()))
        tail = lb.tail
        Detector.run(tail, {"bbox_xywh": lb.vbbox, "class_prob": lb.vprob, "class_idx": lb.vcls}, orig_hw, prob_thresh,
                     iou_thresh, letterbox=letterbox, nms_kind=nms_kind, beta_nms=beta_nms)
        # the tail reports virtual rows: back to prediction rows on the device, before anything packs records (slots past a
        # frame's count hold whatever was there: clamped for the lookup, never read by anyone)
        # -- through buffers made once, like everything else on this path
        lb.index.copy_(tail.row)
        lb.index.clamp_(0, cap - 1)
        torch.gather(lb.vrow, 1, lb.index, out=tail.row)
        self._tail, self._label_run, self._merge_run = tail, lb, None

    def check_label_capacity(self, n_frames=None):
        """After a multi-label ``run``: RuntimeError if one of the first ``n_frames`` frames (default: all) had more labels than
        the capacity, in which case the candidates of that frame were cut off.  One small synchronising copy."""
        lb = self._label_run
        if lb is None:
            return
        counts = lb.vcount.cpu().numpy()
        raise_label_overflow(counts[:n_frames], lb.cap)

    def fetch(self, return_rows=False, kmax=1024, check_labels=True):
        """Detections of the last ``run`` on the host: ONE device-to-host copy per batch.  The device packs every
        frame's first ``kmax`` detections into fixed-size records that also carry the frame's true count
        (``y3_pack_records``, the multi-GPU gather's format); only if some frame kept more than ``kmax`` boxes is a
        second, larger copy made.  After a multi-label run one more small copy checks the label counts of all frames, unless
        the caller has checked them already (``check_labels=False``: ``Pipeline.results``, which knows the real frames)."""
        if check_labels:
            self.check_label_capacity()
        if self._tail is not self:
            return self._tail.fetch(return_rows=return_rows, kmax=kmax, check_labels=False)
        from .dist import unpack_records
        lib = _hip.lib()
        kmax = max(1, min(int(kmax), self.rows))
        src = self._merge_run if self._merge_run is not None else self     # the merged detections of run_tiled(merge=...)
        while True:
            rec = self._records.get(kmax)
            if rec is None:
                rec = self._records[kmax] = torch.empty((self.batch, kmax, 8), dtype=torch.int32, device=self.device)
            _hip.check(lib.y3_pack_records(src.count.data_ptr(), src.tlbr.data_ptr(), src.prob.data_ptr(),
                                           src.cls.data_ptr(), src.row.data_ptr(), self.batch, self.rows, kmax,
                                           rec.data_ptr(), None, _hip.stream_ptr()))
            host = rec.cpu().numpy()                         # the one synchronising copy
            most = int(host[:, 0, 7].max()) if host.size else 0
            if most <= kmax:
                break
            kmax = min(self.rows, max(most, 2 * kmax))
        results = []
        for item in unpack_records(host):
            results.append(item[:4] if return_rows else item[:3])
        return results


class _MergeBuffers(object):
    """Device buffers of ``y3_merge_tiled`` for one (batch, capacity): its outputs, the members and its workspace."""

    def __init__(self, batch, rows, device):
        self.ws_bytes = _hip.lib().y3_merge_tiled_workspace_bytes(batch, rows)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.count = torch.zeros(batch, dtype=torch.int32, device=device)
        self.tlbr = torch.empty((batch, rows, 4), dtype=torch.int64, device=device)
        self.prob = torch.empty((batch, rows), dtype=torch.float32, device=device)
        self.cls = torch.empty((batch, rows), dtype=torch.int64, device=device)
        self.row = torch.empty((batch, rows), dtype=torch.int32, device=device)
        self.members = torch.empty((batch, rows), dtype=torch.int32, device=device)


class _LabelBuffers(object):
    """Device buffers of ``y3_expand_labels`` for one (batch, rows_total, capacity): the virtual rows and its workspace."""

    def __init__(self, batch, rows_total, cap, device):
        self.cap = cap
        self.ws_bytes = _hip.lib().y3_expand_labels_workspace_bytes(batch, rows_total, cap)
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.vbbox = torch.empty((batch, cap, 4), dtype=torch.float32, device=device)
        self.vprob = torch.empty((batch, cap), dtype=torch.float32, device=device)
        self.vcls = torch.empty((batch, cap), dtype=torch.int64, device=device)
        self.vrow = torch.empty((batch, cap), dtype=torch.int32, device=device)
        self.vcount = torch.zeros(batch, dtype=torch.int32, device=device)
        self.index = torch.empty((batch, cap), dtype=torch.int64, device=device)     # the tail's rows as gather indices
        self.tail = None


def raise_label_overflow(counts, cap):
    """RuntimeError naming the first frame whose true label count exceeds the capacity."""
    for frame, count in enumerate(np.asarray(counts).tolist()):
        if count > cap:
            raise RuntimeError("multi-label detection: frame {} has {} labels above the threshold, more than label_capacity={}; "
                               "pass a larger label_capacity= (or a higher prob_thresh)".format(frame, count, cap))


def tile_geom_tensor(geom, device):
    """[(sx, sy, ox, oy), ...] -> the ``y3_tile_geom`` array as a uint8 device tensor (16 bytes per tile)."""
    arr = np.array([tuple(g) for g in geom], dtype=np.dtype([("sx", "<f4"), ("sy", "<f4"), ("ox", "<i4"), ("oy", "<i4")]))
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def cut_tiles_device(frame, net_h, net_w, grid, fill=128, out=None):
    """The windows of ``grid`` ((y0, x0) origins) of one uint8 (H, W, 3) device frame as a (len(grid), net_h, net_w, 3) uint8
    tensor (``out``, or a new one): ``y3_tiles_u8`` on the current stream, bit-identical to ``tiles.cut_tiles_u8``."""
    _hip.require_capabilities(_hip.CAP_TILES, "cut_tiles_device")
    if frame.dim() != 3 or frame.shape[2] != 3 or frame.dtype != torch.uint8 or not frame.is_contiguous():
        raise ValueError("cut_tiles_device: the frame is not a contiguous uint8 (H, W, 3) tensor: {} {}".format(
            tuple(frame.shape), frame.dtype))
    sh, sw = int(frame.shape[0]), int(frame.shape[1])
    if out is None:
        out = torch.empty((len(grid), net_h, net_w, 3), dtype=torch.uint8, device=frame.device)
    descs = (_hip.Y3Tile * len(grid))(*[_hip.Y3Tile(frame.data_ptr(), sh, sw, int(y0), int(x0)) for y0, x0 in grid])
    with torch.cuda.device(frame.device):
        _hip.check(_hip.lib().y3_tiles_u8(descs, len(grid), out.data_ptr(), net_h, net_w, _fill_byte(fill), _hip.stream_ptr()))
    return out


def frame_tiles_device(image, net_h, net_w, device, overlap, overview=True, fill=128, out=None):
    """One frame -> (its tiles as a (T, net_h, net_w, 3) uint8 device tensor, their [(sx, sy, ox, oy), ...]): the windows of
    ``tiles.tile_grid`` in its order and, with ``overview``, the whole frame resized by ``inference()``'s default resize
    (``y3_resize_bilinear_u8``) to net_h rows and net_w columns -- a tile like the others, so a rectangular network does not get
    the transposed input that ``preprocess.reference_dsize`` gives its untiled frames."""
    src = image if isinstance(image, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(image))
    src = src.to(device).contiguous()
    if src.dim() != 3 or src.shape[2] != 3 or src.dtype != torch.uint8:
        raise ValueError("tiled inference: a frame is not uint8 (H, W, 3): {} {}".format(tuple(src.shape), src.dtype))
    sh, sw = int(src.shape[0]), int(src.shape[1])
    grid = _tiles.tile_grid(sh, sw, net_h, net_w, overlap)
    n = len(grid) + (1 if overview else 0)
    if out is None:
        out = torch.empty((n, net_h, net_w, 3), dtype=torch.uint8, device=device)
    cut_tiles_device(src, net_h, net_w, grid, fill, out=out[:len(grid)])
    if overview:
        resize_on_device(src, net_h, net_w, device, out=out[len(grid)])
    return out, _tiles.tile_geometry(sh, sw, net_h, net_w, grid, overview)


def tile_chunks(n_tiles, tile_batch):
    """[(start, stop), ...]: the chunks in which ``n_tiles`` tiles go through the network, at most ``tile_batch`` each."""
    return [(i, min(i + tile_batch, n_tiles)) for i in range(0, n_tiles, tile_batch)]


class _TileBuffers(object):
    """Device buffers of tiled inference for one tile count and network size, made once: the tiles and, per row count of a
    tile, the concatenated forward outputs."""

    def __init__(self, n_tiles, net_h, net_w, device):
        self.n_tiles, self.device = n_tiles, device
        self.frames = torch.empty((n_tiles, net_h, net_w, 3), dtype=torch.uint8, device=device)
        self._outs = {}

    def outputs(self, rows):
        out = self._outs.get(rows)
        if out is None:
            n, dev = self.n_tiles, self.device
            out = self._outs[rows] = {"bbox_xywh": torch.empty((n, rows, 4), dtype=torch.float32, device=dev),
                                      "class_prob": torch.empty((n, rows), dtype=torch.float32, device=dev),
                                      "class_idx": torch.empty((n, rows), dtype=torch.int64, device=dev)}
        return out


_tile_buffers = {}


def _inference_tiled(net, images, dev, prob_thresh, iou_thresh, return_rows, overlap, overview, fill, tile_batch, merge=None):
    _hip.require_capabilities(_hip.CAP_TILES, "inference(tile_overlap=...)")
    if merge is not None:
        _hip.require_capabilities(_hip.CAP_TILE_MERGE, "inference(tile_merge=...)")
    net_h, net_w = net.net_info["height"], net.net_info["width"]
    results = []
    for image in images:
        n_tiles = len(_tiles.tile_grid(int(image.shape[0]), int(image.shape[1]), net_h, net_w, overlap)) + (1 if overview else 0)
        key = (n_tiles, net_h, net_w, str(dev))
        buf = _tile_buffers.get(key)
        if buf is None:
            buf = _tile_buffers[key] = _TileBuffers(n_tiles, net_h, net_w, dev)
        with torch.cuda.device(dev):
            frames, geom = frame_tiles_device(image, net_h, net_w, dev, overlap, overview, fill, out=buf.frames)
            for start, stop in tile_chunks(n_tiles, tile_batch):
                out = net.forward_frames(frames[start:stop], fresh=False)
                union = buf.outputs(int(out["class_prob"].shape[1]))
                for k, v in out.items():                     # the plan's buffers are rewritten by the next chunk of this size
                    union[k][start:stop].copy_(v)
            rows = int(union["class_prob"].shape[1])
            det = get_detector(1, n_tiles * rows, dev)
            det.run_tiled(union, geom, n_tiles, prob_thresh, iou_thresh, merge=merge)
            results.extend(det.fetch(return_rows=return_rows))
    return results


_detectors = {}


def get_detector(batch, rows, device):
    key = (batch, rows, str(device))
    det = _detectors.get(key)
    if det is None:
        det = Detector(batch, rows, device)
        _detectors[key] = det
    return det


def inference(net, images, device="cuda", prob_thresh=0.05, nms_iou_thresh=0.3, resize=True,
              return_rows=False, letterbox=False, letterbox_fill=128, nms_kind=None, beta_nms=0.6, label_capacity=None,
              preprocess=None, tile_overlap=None, tile_overview=True, tile_fill=128, tile_batch=16, tile_merge=None):
    """Run detection on one frame or a list of HxWx3 uint8 BGR frames.

    Returns, per frame, ``[bbox_tlbr int64 (K,4), class_prob float32 (K,), class_idx int64 (K,)]``
    (plus the prediction-row index of every detection when ``return_rows``), in original-frame
    pixel coordinates -- same contract as the reference's ``inference()``.

    ``letterbox=True``: Darknet letterboxing instead of the stretched resize (aspect ratio kept, the rest of the network
    input filled with the byte ``letterbox_fill``), boxes corrected back to the frame; frames of different sizes may
    then share the call.  It needs ``resize`` (a ValueError otherwise).

    ``nms_kind``: None [default] = the reference's suppression (integer pixel corners, +1 areas, IoU > ``nms_iou_thresh``);
    "iou", "greedynms" or "diounms" = Darknet's on the float32 boxes, with ``nms_iou_thresh`` as its threshold and
    ``beta_nms`` as the exponent of "diounms" (``net.nms_hint`` holds what the cfg asks for).  ValueError for any other kind.

    A network built with ``multi_label=True`` returns Darknet's multi-label detections: every class of a box whose score
    is ``> prob_thresh`` (strictly), so a box may appear once per class.  ``label_capacity``: the most labels a frame may
    have before suppression (default: the number of prediction rows); a frame with more raises a RuntimeError.

    ``preprocess``: None [default] = the uint8 path above; "darknet" = Darknet's own float preprocessing
    (``preprocess.darknet_frames_device``): ``letterbox=True`` then selects its ``letterbox_image`` (pad 0.5;
    ``letterbox_fill`` is ignored) with the same box correction, False its ``resize_image`` to the whole network input, boxes
    scaled as in the default mode.  Frames of different sizes may share the call either way.  It needs ``resize``; any other
    value is a ValueError, as is a frame so long and thin that its target would be one pixel wide.

    ``tile_overlap``: None [default] = every frame is resized to the network, as above; a fraction in [0, 0.9] = tiled
    inference (``yolov3/tiles.py``).  Every frame, one at a time, is cut into net-sized windows at full resolution whose
    neighbours share at least that fraction of the network size (a frame that fits the network is one window, padded with
    the byte ``tile_fill``), plus -- with ``tile_overview`` -- the whole frame resized by the default 8-bit resize to net_h rows
    and net_w columns, for objects larger than a window.  The tiles run through the network in chunks of at most ``tile_batch``; all their rows are the
    frame's candidates, in frame pixels, for one suppression.  With ``return_rows`` the row of a detection is
    ``tile * rows of one tile + row``, tiles in ``tiles.tile_grid``'s order and the overview last.  An object cut by a window's
    border yields partial boxes that suppression does not merge unless ``tile_merge`` is given: otherwise choose the overlap
    larger than the objects looked for.
    ValueError with ``letterbox=True``, ``preprocess="darknet"``, ``resize=False``, an ``nms_kind``, a ``multi_label``
    network, or an overlap outside [0, 0.9].

    ``tile_merge``: None [default] = nothing more (no further launch, no further buffer); a threshold in [0, 1] = the seam merge
    after the suppression (``y3_merge_tiled``; include/yolov3_hip.h states the rule, ``tiles.merge_detections`` restates it).
    In the canonical order, a detection absorbs every later one of its class that comes from a DIFFERENT tile, is not absorbed
    yet, and whose box it matches: intersection over the smaller of the two areas ``>`` the threshold, on the original integer
    boxes.  What it absorbed is dropped and its box becomes the union; score, class and -- with ``return_rows`` -- row stay its
    own, so four arrays per frame as before.  Pairs within one tile are left alone: the network saw both in one view and the IoU
    suppression has ruled.  0.5 is a reasonable start; 1.0 merges nothing.  Its effect on accuracy has not been measured.
    ValueError without ``tile_overlap``, or for a value that is no number in [0, 1].
    """
    if tile_merge is not None:
        if tile_overlap is None:
            raise ValueError("tile_merge needs tile_overlap: seam merging is a stage of tiled inference")
        tile_merge = _tiles.check_merge(tile_merge)
    if tile_overlap is not None:
        tile_overlap = _tiles.check_options(tile_overlap, letterbox=letterbox, preprocess=preprocess, resize=resize,
                                            nms_kind=nms_kind, multi_label=getattr(net, "multi_label", False))
        tile_fill = _fill_byte(tile_fill)
        if int(tile_batch) < 1:
            raise ValueError("tile_batch must be >= 1, got {!r}".format(tile_batch))
    _hip.nms_mode(nms_kind, beta_nms)
    mode = _hip.check_preprocess_mode(preprocess)
    if letterbox and not resize:
        raise ValueError("letterbox=True resizes every frame: it cannot be combined with resize=False")
    if mode and not resize:
        raise ValueError("preprocess='darknet' resizes every frame: it cannot be combined with resize=False")
    if not isinstance(images, (list, tuple)):
        images = [images]
    if str(device).startswith("cuda") and not str(net.device).startswith("cuda"):
        net.cuda(device)
    dev = net._torch_device()
    if tile_overlap is not None:
        return _inference_tiled(net, list(images), dev, float(np.float32(prob_thresh)), float(nms_iou_thresh), return_rows,
                                tile_overlap, bool(tile_overview), tile_fill, int(tile_batch), merge=tile_merge)
    net_h, net_w = net.net_info["height"], net.net_info["width"]
    if mode == "darknet":
        _hip.require_capabilities(_hip.CAP_PREPROCESS_DARKNET | (_hip.CAP_LETTERBOX if letterbox else 0),
                                  "inference(preprocess='darknet')")
        x, shapes = darknet_frames_device(list(images), net_h, net_w, dev, letterbox)
        out = net._run(x, "f32", fresh=False)
    elif letterbox:
        _hip.require_capabilities(_hip.CAP_LETTERBOX, "inference(letterbox=True)")
        frames, shapes = letterbox_frames_device(list(images), net_h, net_w, dev, letterbox_fill)
        out = net.forward_frames(frames, fresh=False)
    else:
        frames, shapes = prepare_frames_device(list(images), net_h, net_w, dev, resize)
        out = net.forward_frames(frames, fresh=False)
    batch, rows = out["class_prob"].shape
    det = get_detector(batch, rows, dev)
    orig_hw = np.array([[s[0], s[1]] for s in shapes], dtype=np.int32)
    with torch.cuda.device(dev):
        det.run(out, orig_hw, float(np.float32(prob_thresh)), float(nms_iou_thresh),
                letterbox=(net_h, net_w) if letterbox else None, nms_kind=nms_kind, beta_nms=beta_nms,
                labels=net.label_heads() if getattr(net, "multi_label", False) else None, label_capacity=label_capacity)
        return det.fetch(return_rows=return_rows)
