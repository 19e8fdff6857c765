"""Darknet's preprocessing restated in numpy float32, independent of the package: ``load_image`` (byte / 255, BGR -> planar
RGB), ``resize_image`` as the TWO-PASS form with an explicit ``part`` image, ``letterbox_image`` (geometry, 0.5 canvas, paste).
Every numpy operation below is one float32 operation with one rounding (numpy never fuses a product into a sum), which is the
arithmetic include/yolov3_hip.h states for ``y3_preprocess_darknet_f32``.

Pixel value: Darknet computes ``(float)(byte / 255.)`` -- the division in double, stored to float.  For all 256 bytes that
equals the float32 division ``float32(byte) / float32(255)`` used here (tests/test_darknet_resize_host.py checks it), so the
float32 form is the specification.

Two places where Darknet's C leaves the arithmetic undefined are pinned here: an axis with ONE source pixel takes scale 0
(Darknet computes 0 / 0 for 1 -> 1 and never uses the result for a pixel that matters), and a target of one row / column from a
longer source (a division by zero there) is a ValueError."""
import numpy as np

F = np.float32


def pixel_values(frame_bgr):
    """uint8 (h, w, 3) BGR -> float32 (3, h, w) RGB: ``p = float32(byte) / float32(255)``"""
    frame = np.asarray(frame_bgr)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3
    rgb = frame[:, :, ::-1].transpose(2, 0, 1)
    return np.ascontiguousarray(rgb.astype(F) / F(255.0))


def _scale(src, dst):
    return F(0.0) if src == 1 else F(src - 1) / F(dst - 1)


def horizontal(src, W):
    """``part`` (C, h, W): the first pass of resize_image over float32 ``src`` (C, h, w)"""
    C, h, w = src.shape
    part = np.empty((C, h, W), F)
    part[:, :, W - 1] = src[:, :, w - 1]
    if w == 1:
        part[:] = src[:, :, :1]
        return part
    c = np.arange(W - 1)
    sx = c.astype(F) * _scale(w, W)
    ix = sx.astype(np.int64)                       # (int)sx: truncation
    dx = sx - ix.astype(F)
    assert sx.dtype == F and dx.dtype == F and (ix + 1 <= w - 1).all()
    part[:, :, :W - 1] = (F(1.0) - dx) * src[:, :, ix] + dx * src[:, :, ix + 1]
    return part


def vertical(part, H):
    """(C, H, W): the second pass over ``part`` (C, h, W).  dy is NOT forced to 0 on the last row: where (H - 1) * h_scale rounds
    to just below h - 1 that row is (1 - dy) * part[h - 2] with dy just below 1, and its second term is dropped -- Darknet's quirk."""
    C, h, W = part.shape
    r = np.arange(H)
    sy = r.astype(F) * _scale(h, H)
    iy = sy.astype(np.int64)
    dy = sy - iy.astype(F)
    assert sy.dtype == F and dy.dtype == F and (iy <= h - 1).all()
    out = (F(1.0) - dy)[None, :, None] * part[:, iy, :]
    if h > 1:
        assert (iy[:H - 1] + 1 <= h - 1).all()
        out[:, :H - 1] = out[:, :H - 1] + dy[None, :H - 1, None] * part[:, iy[:H - 1] + 1, :]
    assert out.dtype == F
    return out


def resize(src, H, W):
    """Darknet's ``resize_image``: float32 (C, h, w) -> (C, H, W); equal sizes come back unchanged (a copy)"""
    src = np.asarray(src)
    assert src.dtype == F and src.ndim == 3
    h, w = src.shape[1:]
    if (h, w) == (H, W):
        return src.copy()
    if H < 1 or W < 1 or (H == 1 and h > 1) or (W == 1 and w > 1):
        raise ValueError("resize_image to %d x %d from %d x %d divides by zero" % (H, W, h, w))
    return vertical(horizontal(src, W), H)


def geometry(h, w, net_h, net_w):
    """(new_h, new_w, top, left) of ``letterbox_image``: the side with the smaller float32 scale fills the network, the other is
    the truncated integer product (at least 1); the pad splits in integer halves"""
    if F(net_w) / F(w) < F(net_h) / F(h):
        new_w, new_h = net_w, (h * net_w) // w
    else:
        new_h, new_w = net_h, (w * net_h) // h
    new_h, new_w = max(new_h, 1), max(new_w, 1)
    return new_h, new_w, (net_h - new_h) // 2, (net_w - new_w) // 2


def letterbox(frame_bgr, net_h, net_w):
    """uint8 (h, w, 3) BGR -> float32 (3, net_h, net_w): ``letterbox_image`` of ``load_image``"""
    src = pixel_values(frame_bgr)
    new_h, new_w, top, left = geometry(src.shape[1], src.shape[2], net_h, net_w)
    out = np.full((3, net_h, net_w), F(0.5), F)
    out[:, top:top + new_h, left:left + new_w] = resize(src, new_h, new_w)
    return out


def stretch(frame_bgr, net_h, net_w):
    """uint8 (h, w, 3) BGR -> float32 (3, net_h, net_w): ``resize_image`` of ``load_image`` to the whole network input"""
    return resize(pixel_values(frame_bgr), net_h, net_w)


def network_input(frames, net_h, net_w, letterbox_mode):
    """(B, 3, net_h, net_w) float32 of a list of frames whose sizes may differ"""
    one = letterbox if letterbox_mode else stretch
    return np.stack([one(f, net_h, net_w) for f in frames])


def random_frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)
