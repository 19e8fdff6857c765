"""Host-side frame preparation for ``inference()`` (reference inference.py:314-335).

The reference resizes with ``cv2.resize(image, (net_h, net_w))`` (bilinear, no letterbox, aspect not
preserved) when a frame is not net-sized.  OpenCV is not available in this image, so
:func:`resize_bilinear_u8` RESTATES OpenCV's published algorithm for 8-bit ``INTER_LINEAR``
(opencv/modules/imgproc/src/resize.cpp, 4.x: ``resizeGeneric_`` with ``HResizeLinear<uchar,int,short,2048>``
and the 8-bit specialisation of ``VResizeLinear``; IPP is not used for 8-bit linear unless
``useIPP_NotExact``):

* per destination column ``fx = (float)((dx + 0.5) * scale_x - 0.5)`` with ``scale_x = 1 / (dst_w / src_w)`` in
  double, ``sx = floor(fx)``, ``fx -= sx``; ``sx < 0 -> sx = 0, fx = 0``; ``sx >= src_w - 1 -> sx = src_w - 1,
  fx = 0`` (that column then reads the single pixel times 2048); coefficients
  ``saturate_cast<short>((1 - fx) * 2048)``, ``saturate_cast<short>(fx * 2048)`` (round half to even);
* rows likewise, except that the two source rows are clamped into the image instead of the weight being zeroed;
* horizontal pass to int: ``S[sx] * a0 + S[sx + 1] * a1``; vertical pass
  ``(((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2``  -- two stages, each truncating;
* an exact 2:1 reduction, which OpenCV routes to its INTER_AREA fast path ``(s00 + s01 + s10 + s11 + 2) >> 2``,
  comes out of the formulas above unchanged (all four weights are 1024).

PARITY against OpenCV ITSELF is unpinned for this function (no cv2 in this image: INTEGRATION.md).  What is pinned
(tests/test_resize_pin.py): host (:func:`resize_bilinear_u8`) and device (``y3_resize_bilinear_u8``) are within 1 LSB on
every byte -- 88-91 % of the bytes equal -- of an independent float bilinear with the same conventions
(``torch.nn.functional.interpolate``, kept with the test infrastructure) on the nine sample images, up- and down-scaling, and
bit-identical to each other; net-sized frames -- the benchmark's case, and the crop goldens tests/golden/inference_crops_* --
skip the resize exactly like the reference does (inference.py:322-326).
Like the reference, ``dsize`` is passed as ``(net_h, net_w)`` although cv2 reads it as (width, height): for the
square networks shipped here that is the same thing, and :func:`reference_dsize` keeps the quirk for others.

Letterboxing (opt-in; not in the reference, which stretches): Darknet's ``letterbox_image`` keeps the frame's aspect
ratio, resizes it to :func:`letterbox_geometry`'s (new_h, new_w) with the resize above and pastes it at (top, left) of a
net-sized canvas of the byte ``fill`` (:func:`letterbox_u8`; on the GPU :func:`letterbox_frames_device`, one
``y3_letterbox_u8`` call per batch, bit-identical).  Differences from Darknet on this uint8 path: the fill is a byte, 128 by
default (Darknet fills with 0.5 in float, which a uint8 frame read as v / 255 cannot hold), and the resize is OpenCV's
bilinear, not Darknet's ``resize_image``.  :func:`correct_letterbox_boxes` maps the network's relative boxes back to the frame
(``correct_yolo_boxes(..., letter=1)``; on the GPU inside ``y3_detect_letterbox``).

Darknet's own preprocessing (opt-in, ``preprocess="darknet"`` on the detection entry points; not in the reference) has neither
difference: :func:`darknet_frames_device` turns uint8 BGR frames of any size into the float32 (B, 3, net_h, net_w) RGB input
that Darknet's ``load_image`` -> ``letterbox_image`` / ``resize_image`` produce, bit for bit, with one
``y3_preprocess_darknet_f32`` launch per batch: ``byte / 255`` first, then Darknet's float32 bilinear with its align-corners
geometry ``(src - 1) / (dst - 1)`` (include/yolov3_hip.h states every operation; tests/darknet_resize_restate.py restates it
in numpy), pasted on a canvas of 0.5f when letterboxing.  The result feeds ``Darknet.forward``'s float input, not the fused
uint8 stem.  :func:`darknet_target` gives the size a frame is resized to and where it lies; ``reference_dsize`` and
``letterbox_fill`` play no part in this mode.
"""
import numpy as np

_COEF_BITS = 11
_COEF_ONE = 1 << _COEF_BITS          # INTER_RESIZE_COEF_SCALE


def _round_half_even_to_short(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int64)     # cvRound + saturate_cast<short>


def _axis_taps(src_len, dst_len, clamp_weights):
    """OpenCV's xofs / ialpha (``clamp_weights=True``) or yofs / ibeta (False) tables for one axis:
    (lo index, hi index, weight_lo, weight_hi)."""
    inv_scale = float(dst_len) / float(src_len)
    scale = 1.0 / inv_scale
    f = ((np.arange(dst_len, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_weights:
        low = s < 0
        f[low] = 0.0
        s[low] = 0
        high = s >= src_len - 1
        f[high] = 0.0
        s[high] = src_len - 1
    w_lo = _round_half_even_to_short((np.float32(1.0) - f) * np.float32(_COEF_ONE))
    w_hi = _round_half_even_to_short(f * np.float32(_COEF_ONE))
    lo = np.clip(s, 0, src_len - 1)
    hi = np.clip(s + 1, 0, src_len - 1)
    if clamp_weights:
        # columns at / past the last pixel read that pixel alone, times ONE (HResizeLinear's dx >= xmax loop)
        w_hi = np.where(high, 0, w_hi)
        w_lo = np.where(high, _COEF_ONE, w_lo)
    return lo, hi, w_lo, w_hi


def resize_bilinear_u8(img, out_h, out_w):
    """uint8 (H,W,C) -> uint8 (out_h,out_w,C): OpenCV's 8-bit INTER_LINEAR arithmetic, integers only."""
    img = np.asarray(img)
    if img.shape[0] == out_h and img.shape[1] == out_w:
        return img
    ylo, yhi, wy0, wy1 = _axis_taps(img.shape[0], out_h, False)
    xlo, xhi, wx0, wx1 = _axis_taps(img.shape[1], out_w, True)
    src = img.astype(np.int64)
    rows = src[:, xlo, :] * wx0[None, :, None] + src[:, xhi, :] * wx1[None, :, None]      # HResizeLinear -> int
    top, bot = rows[ylo] >> 4, rows[yhi] >> 4
    out = (((wy0[:, None, None] * top) >> 16) + ((wy1[:, None, None] * bot) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


def reference_dsize(net_h, net_w):
    """Rows, columns of the frame the reference feeds the network: it calls ``cv2.resize(image, (net_h, net_w))``
    (inference.py:323-325) and cv2 reads dsize as (width, height), so the result has net_w rows and net_h columns."""
    return net_w, net_h


def axis_table(src_len, dst_len, clamp_weights):
    """(dst_len, 4) int32 rows {lo, hi, weight_lo, weight_hi}: the tap table both the host resize above and
    the device kernel ``y3_resize_bilinear_u8`` use (so they agree bit for bit)."""
    lo, hi, w0, w1 = _axis_taps(src_len, dst_len, clamp_weights)
    return np.ascontiguousarray(np.stack([lo, hi, w0, w1], axis=1).astype(np.int32))


_device_tables = {}


def _tables(sh, sw, out_h, out_w, device):
    """Device tap tables of an (sh, sw) -> (out_h, out_w) resize, made once per geometry and device."""
    import torch
    key = (sh, sw, out_h, out_w, str(device))
    if key not in _device_tables:
        _device_tables[key] = (torch.from_numpy(axis_table(sh, out_h, False)).to(device),
                               torch.from_numpy(axis_table(sw, out_w, True)).to(device))
    return _device_tables[key]


def resize_on_device(frame, out_h, out_w, device, out=None):
    """uint8 (H,W,3) numpy / torch frame -> uint8 (out_h,out_w,3) torch tensor on ``device`` (HIP kernel;
    identical result to :func:`resize_bilinear_u8`).  ``out`` may be a preallocated slice of a batch tensor."""
    import torch
    from . import _hip
    src = frame if isinstance(frame, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frame))
    src = src.to(device).contiguous()
    sh, sw = int(src.shape[0]), int(src.shape[1])
    if out is None:
        out = torch.empty((out_h, out_w, 3), dtype=torch.uint8, device=device)
    if (sh, sw) == (out_h, out_w):
        out.copy_(src)
        return out
    ytab, xtab = _tables(sh, sw, out_h, out_w, device)
    with torch.cuda.device(device):
        _hip.check(_hip.lib().y3_resize_bilinear_u8(src.data_ptr(), sh, sw, out.data_ptr(), out_h, out_w,
                                                    ytab.data_ptr(), xtab.data_ptr(), _hip.stream_ptr()))
    return out


def _target_shapes(shapes, net_h, net_w, resize):
    """Rows, columns every frame has when it enters the network, following inference.py:320-326: a frame that
    already is (net_h, net_w) stays, any other goes through ``cv2.resize(image, (net_h, net_w))`` and comes out with
    ``reference_dsize`` rows / columns.  Like ``np.stack`` there, a batch must end up with one size."""
    if resize:
        out = [s[:2] if tuple(s[:2]) == (net_h, net_w) else reference_dsize(net_h, net_w) for s in shapes]
    else:
        out = [tuple(s[:2]) for s in shapes]
    if len(set(out)) != 1:
        raise ValueError("frames of different sizes cannot form one batch: {}".format(sorted(set(out))))
    return out[0]


def prepare_frames_device(images, net_h, net_w, device, resize=True):
    """Like :func:`prepare_frames` but uploads every original frame once and resizes on the GPU."""
    import torch
    if not isinstance(images, (list, tuple)):
        images = [images]
    shapes = [tuple(im.shape) for im in images]
    out_h, out_w = _target_shapes(shapes, net_h, net_w, resize)
    batch = torch.empty((len(images), out_h, out_w, 3), dtype=torch.uint8, device=device)
    for i, im in enumerate(images):
        resize_on_device(im, out_h, out_w, device, out=batch[i])
    return batch, shapes


def prepare_frames(images, net_h, net_w, resize=True):
    """list of HxWx3 uint8 BGR -> (uint8 (B,h,w,3) BGR, list of original shapes)."""
    if not isinstance(images, (list, tuple)):
        images = [images]
    shapes = [tuple(im.shape) for im in images]
    out_h, out_w = _target_shapes(shapes, net_h, net_w, resize)
    images = [resize_bilinear_u8(im, out_h, out_w) for im in images]
    return np.ascontiguousarray(np.stack(images)), shapes


# ---------------------------------------------------------------------------------------------- letterboxing
def letterbox_geometry(h, w, net_h, net_w):
    """(new_h, new_w, top, left) of an (h, w) frame letterboxed into (net_h, net_w): Darknet's ``letterbox_image``.
    The side whose float32 scale is smaller fills the network, the other is scaled by the integer product (truncated)
    and clamped to at least 1; the pad splits with integer halves.  Same definition as ``y3_letterbox_geometry``."""
    h, w, net_h, net_w = int(h), int(w), int(net_h), int(net_w)
    if min(h, w, net_h, net_w) <= 0:
        raise ValueError("letterbox_geometry: sizes must be positive, got {}".format((h, w, net_h, net_w)))
    if np.float32(net_w) / np.float32(w) < np.float32(net_h) / np.float32(h):
        new_w, new_h = net_w, (h * net_w) // w
    else:
        new_h, new_w = net_h, (w * net_h) // h
    new_h, new_w = max(new_h, 1), max(new_w, 1)
    return new_h, new_w, (net_h - new_h) // 2, (net_w - new_w) // 2


def _fill_byte(fill):
    fill = int(fill)
    if not 0 <= fill <= 255:
        raise ValueError("letterbox fill must be a byte (0..255), got {}".format(fill))
    return fill


def letterbox_u8(img, net_h, net_w, fill=128):
    """uint8 (H,W,3) -> uint8 (net_h,net_w,3): the frame resized to :func:`letterbox_geometry`'s size with
    :func:`resize_bilinear_u8` and pasted at (top, left) of a canvas of ``fill``.  A net-sized frame comes back unchanged."""
    img = np.asarray(img)
    new_h, new_w, top, left = letterbox_geometry(img.shape[0], img.shape[1], net_h, net_w)
    out = np.full((net_h, net_w, 3), _fill_byte(fill), dtype=np.uint8)
    out[top:top + new_h, left:left + new_w] = resize_bilinear_u8(img, new_h, new_w)
    return out


def letterbox_frames_device(images, net_h, net_w, device, fill=128):
    """Letterbox a list of uint8 (H,W,3) frames -- sizes may differ -- into a (B, net_h, net_w, 3) uint8 device tensor
    with ONE ``y3_letterbox_u8`` call on the current stream (bit-identical to :func:`letterbox_u8`).  Every frame is
    uploaded as :func:`prepare_frames_device` does; the tap tables are cached per geometry.  Returns (batch, shapes)."""
    import torch
    from . import _hip
    _hip.require_capabilities(_hip.CAP_LETTERBOX, "letterbox_frames_device")
    if not isinstance(images, (list, tuple)):
        images = [images]
    fill = _fill_byte(fill)
    shapes = [tuple(im.shape) for im in images]
    batch = torch.empty((len(images), net_h, net_w, 3), dtype=torch.uint8, device=device)
    descs = (_hip.Y3LetterboxFrame * len(images))()
    keep = []                                            # uploads alive until the launch is queued
    for i, im in enumerate(images):
        src = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        src = src.to(device).contiguous()
        sh, sw = int(src.shape[0]), int(src.shape[1])
        if src.dim() != 3 or src.shape[2] != 3 or src.dtype != torch.uint8:
            raise ValueError("letterbox_frames_device: frame {} is not uint8 (H, W, 3): {} {}".format(
                i, tuple(src.shape), src.dtype))
        new_h, new_w, _, _ = letterbox_geometry(sh, sw, net_h, net_w)
        ytab, xtab = _tables(sh, sw, new_h, new_w, device)
        descs[i] = _hip.Y3LetterboxFrame(src.data_ptr(), sh, sw, ytab.data_ptr(), xtab.data_ptr())
        keep.append(src)
    with torch.cuda.device(device):
        _hip.check(_hip.lib().y3_letterbox_u8(descs, len(images), batch.data_ptr(), net_h, net_w, fill, _hip.stream_ptr()))
    return batch, shapes


def correct_letterbox_boxes(bbox_xywh, orig_hw, net_h, net_w):
    """Darknet's ``correct_yolo_boxes(..., letter=1)`` on relative boxes, for callers who run ``forward`` on
    letterboxed frames themselves: bbox_xywh (B, N, 4) (or (N, 4) with one (h, w)), orig_hw (B, 2) frame sizes.
    Per frame: ``x' = (float32)((x - deltaw / 2 / net_w) / ratiow)`` in float64 and ``w' = w * (1 / ratiow)`` in float32,
    with ``deltaw = float32(net_w - new_w)`` and ``ratiow = float32(new_w) / net_w``; y, h likewise.  The correction
    uses delta / 2 even where the image was shifted by the integer top / left (Darknet's own mismatch).  Returns a new
    float32 array; feed it to the reference's ``* orig_w`` / ``* orig_h`` post-processing.  ``y3_detect_letterbox``
    computes exactly this."""
    box = np.array(bbox_xywh, dtype=np.float32)
    hw = np.asarray(orig_hw).reshape(-1, 2)
    single = box.ndim == 2
    if single:
        box = box[None]
    if box.ndim != 3 or box.shape[2] < 4 or box.shape[0] != hw.shape[0]:
        raise ValueError("correct_letterbox_boxes: expected (B, N, >=4) boxes and (B, 2) sizes, got {} and {}".format(
            np.shape(bbox_xywh), np.shape(orig_hw)))
    for i, (h, w) in enumerate(hw.tolist()):
        new_h, new_w, _, _ = letterbox_geometry(h, w, net_h, net_w)
        for c, (new, net) in ((0, (new_w, net_w)), (1, (new_h, net_h))):
            delta = np.float32(net - new)
            ratio = np.float32(new) / np.float32(net)
            shift = np.float64(delta) / 2.0 / np.float64(net)
            box[i, :, c] = ((box[i, :, c].astype(np.float64) - shift) / np.float64(ratio)).astype(np.float32)
            box[i, :, c + 2] = box[i, :, c + 2] * (np.float32(1.0) / ratio)
    return box[0] if single else box


# ---------------------------------------------------------------------------------------------- Darknet's float preprocessing
def darknet_target(h, w, net_h, net_w, letterbox):
    """(new_h, new_w, top, left): the size Darknet resizes an (h, w) frame to and where the result lies in the network input --
    :func:`letterbox_geometry` when ``letterbox`` (``letterbox_image``), else the whole (net_h, net_w) input (``resize_image``;
    rows first: there is no ``reference_dsize`` quirk in this mode).  ValueError for a target of one row / column from a longer
    source: Darknet's ``resize_image`` divides by ``target - 1`` there."""
    h, w, net_h, net_w = int(h), int(w), int(net_h), int(net_w)
    if min(h, w, net_h, net_w) <= 0:
        raise ValueError("darknet_target: sizes must be positive, got {}".format((h, w, net_h, net_w)))
    new_h, new_w, top, left = letterbox_geometry(h, w, net_h, net_w) if letterbox else (net_h, net_w, 0, 0)
    if (new_h == 1 and h > 1) or (new_w == 1 and w > 1):
        raise ValueError("preprocess='darknet': a {} x {} frame would be resized to {} x {}, and Darknet's resize_image divides "
                         "by target - 1 (a 1-pixel target needs a 1-pixel source)".format(h, w, new_h, new_w))
    return new_h, new_w, top, left


def darknet_frames_device(images, net_h, net_w, device, letterbox=False):
    """uint8 (H,W,3) BGR frames -- sizes may differ -- into the float32 (B, 3, net_h, net_w) RGB network input Darknet makes of
    them, on ``device``, with ONE ``y3_preprocess_darknet_f32`` call on the current stream: ``letterbox=True`` is Darknet's
    ``letterbox_image`` (aspect ratio kept, canvas 0.5), False its ``resize_image`` to the whole input.  Every frame is uploaded
    as :func:`prepare_frames_device` does.  Returns (input, shapes); ``Darknet.forward`` takes the input as it is."""
    import torch
    from . import _hip
    _hip.require_capabilities(_hip.CAP_PREPROCESS_DARKNET | (_hip.CAP_LETTERBOX if letterbox else 0), "darknet_frames_device")
    if not isinstance(images, (list, tuple)):
        images = [images]
    shapes = [tuple(im.shape) for im in images]
    for i, s in enumerate(shapes):
        if len(s) != 3 or s[2] != 3 or images[i].dtype != (torch.uint8 if isinstance(images[i], torch.Tensor) else np.uint8):
            raise ValueError("darknet_frames_device: frame {} is not uint8 (H, W, 3): {} {}".format(i, s, images[i].dtype))
        darknet_target(s[0], s[1], net_h, net_w, letterbox)
    x = torch.empty((len(images), 3, net_h, net_w), dtype=torch.float32, device=device)
    descs = (_hip.Y3DarknetFrame * len(images))()
    keep = []                                            # uploads alive until the launch is queued
    for i, im in enumerate(images):
        src = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im))
        src = src.to(device).contiguous()
        descs[i] = _hip.Y3DarknetFrame(src.data_ptr(), int(src.shape[0]), int(src.shape[1]))
        keep.append(src)
    with torch.cuda.device(device):
        _hip.check(_hip.lib().y3_preprocess_darknet_f32(descs, len(images), x.data_ptr(), net_h, net_w, 1 if letterbox else 0,
                                                        _hip.stream_ptr()))
    return x, shapes
