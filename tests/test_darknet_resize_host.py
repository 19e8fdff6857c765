"""Darknet's float preprocessing without a GPU: the numpy restatement (tests/darknet_resize_restate.py) pinned to hand-derived
answers, the C ABI additions (``y3_preprocess_darknet_f32``, ``y3_darknet_frame``, ``Y3_CAP_PREPROCESS_DARKNET``) and the
``preprocess=`` option of every caller, the command line's ``--darknet-resize`` and ``Pipeline``'s refusal."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import yolov3
from yolov3 import _hip, stream
from yolov3.__main__ import build_parser, main
from yolov3.pipeline import Pipeline
from yolov3.preprocess import darknet_frames_device, darknet_target, letterbox_geometry

import darknet_resize_restate as R
from golden_util import GOLDEN, ROOT, SAMPLE_IMAGES

F = np.float32
MINI = os.path.join(GOLDEN, "cfg", "mini.cfg")
HEADER = os.path.join(ROOT, "include", "yolov3_hip.h")


def _planes(h, w, seed, c=2):
    return np.random.default_rng(seed).random((c, h, w), dtype=F)


# ---- the restatement -------------------------------------------------------------------------------------------------------------

def test_float32_division_is_darknets_double_division_for_every_byte():
    b = np.arange(256)
    double_form = (b.astype(np.float64) / 255.0).astype(F)             # (float)(byte / 255.)
    assert np.array_equal((b.astype(F) / F(255.0)).view(np.uint32), double_form.view(np.uint32))
    frame = np.stack([b, b[::-1], (b * 7) % 256], axis=1).astype(np.uint8)[None]      # (1, 256, 3) BGR
    p = R.pixel_values(frame)
    assert p.shape == (3, 1, 256) and p.dtype == F
    assert np.array_equal(p[2, 0], double_form) and np.array_equal(p[1, 0], double_form[::-1])     # R is the frame's third byte
    assert np.array_equal(p[0, 0], double_form[(b * 7) % 256])
    assert p.min() == 0.0 and p.max() == 1.0


def test_equal_sizes_come_back_unchanged():
    src = _planes(5, 7, 1)
    out = R.resize(src, 5, 7)
    assert out is not src and np.array_equal(out.view(np.uint32), src.view(np.uint32))


def test_two_by_two_to_three_by_three():
    """scales (2 - 1) / (3 - 1) = 0.5: the middle column / row sit half way (dx = dy = 0.5, exact), the last ones copy"""
    a, b, c, d = F(0.1), F(0.7), F(0.25), F(0.9)
    out = R.resize(np.array([[[a, b], [c, d]]], F), 3, 3)[0]
    half = F(0.5)
    top = [a, half * a + half * b, b]
    bot = [c, half * c + half * d, d]
    want = np.array([top, [half * t + half * u for t, u in zip(top, bot)], bot], F)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    # halving is exact, so each middle value is the correctly rounded average of its two neighbours
    assert out[0, 1] == (a + b) / F(2.0) and out[2, 1] == (c + d) / F(2.0) and out[1, 0] == (a + c) / F(2.0)
    assert out[1, 1] == (out[0, 1] + out[2, 1]) / F(2.0)


def test_one_row_and_one_column_sources():
    row = _planes(1, 9, 2)
    out = R.resize(row, 8, 8)
    part = R.horizontal(row, 8)
    assert np.array_equal(out, np.repeat(part, 8, axis=1))                 # h == 1: every row is (1 - 0) * part[0]
    assert np.array_equal(out[:, :, 0], np.repeat(row[:, :1, 0], 8, axis=1))
    col = _planes(9, 1, 3)
    out = R.resize(col, 8, 8)
    assert (out == out[:, :, :1]).all()                                    # w == 1: every column is the source's only one
    assert np.array_equal(out[:, :, 0], R.vertical(col, 8)[:, :, 0])
    assert np.array_equal(out[:, 0, 0], col[:, 0, 0])
    one = _planes(1, 1, 4)
    assert (R.resize(one, 4, 6) == one).all()                              # both at once: a constant image
    assert np.array_equal(R.resize(_planes(1, 5, 5), 1, 9), R.horizontal(_planes(1, 5, 5), 9))      # 1 -> 1 rows: scale 0


@pytest.mark.parametrize("shape,target", [((5, 7), (9, 13)), ((37, 23), (16, 24)), ((100, 301), (64, 96)), ((4, 4), (4, 9))])
def test_last_column_is_the_sources_last_column(shape, target):
    src = _planes(*shape, seed=sum(shape))
    part = R.horizontal(src, target[1])
    assert np.array_equal(part[:, :, -1], src[:, :, -1]) and np.array_equal(part[:, :, 0], src[:, :, 0])
    out = R.resize(src, *target)
    assert np.array_equal(out[:, 0, -1], src[:, 0, -1]) and np.array_equal(out[:, 0, 0], src[:, 0, 0])
    # an interior column by hand
    c = target[1] // 2
    sx = F(c) * (F(shape[1] - 1) / F(target[1] - 1))
    ix = int(sx)
    dx = sx - F(ix)
    assert np.array_equal(part[:, :, c], (F(1) - dx) * src[:, :, ix] + dx * src[:, :, ix + 1])


def _quirk_cases():
    """(h, H) for which float32(H - 1) * float32((h - 1) / (H - 1)) is below h - 1"""
    found = []
    for h in range(2, 64):
        for H in range(2, 200):
            if H != h and F(H - 1) * (F(h - 1) / F(H - 1)) < F(h - 1):
                found.append((h, H))
    return found


def test_last_row_quirk():
    cases = _quirk_cases()
    assert cases, "no size pair whose last row's sy rounds below h - 1"
    h, H = cases[0]
    sy = F(H - 1) * (F(h - 1) / F(H - 1))
    assert int(sy) == h - 2
    dy = sy - F(h - 2)
    assert F(0.999) < dy < F(1.0)
    src = np.ones((1, h, 3), F)
    src[0, h - 2] = F(0.75)
    out = R.resize(src, H, 3)
    # the last row is (1 - dy) * part[h - 2] alone: nearly black, not the source's last row
    assert np.array_equal(out[0, H - 1], (F(1.0) - dy) * R.horizontal(src, 3)[0, h - 2])
    assert (out[0, H - 1] < F(1e-3)).all() and (out[0, H - 2] > F(0.7)).all()
    # a pair without the quirk: the last row is the source's last row
    ok = next((a, b) for a in range(2, 64) for b in range(2, 200) if a != b and (a, b) not in set(cases))
    src = _planes(ok[0], 3, 6)
    assert np.array_equal(R.resize(src, ok[1], 3)[:, -1], src[:, -1])


@pytest.mark.parametrize("shape,net", [((20, 90), (32, 48)), ((90, 20), (32, 48)), ((50, 50), (32, 48)), ((1080, 1920), (608, 608))])
def test_letterbox_fill_and_paste(shape, net):
    frame = R.random_frame(*shape, seed=shape[0])
    assert R.geometry(*shape, *net) == letterbox_geometry(*shape, *net) == darknet_target(*shape, *net, True)
    new_h, new_w, top, left = letterbox_geometry(*shape, *net)
    out = R.letterbox(frame, *net)
    assert out.shape == (3,) + net and out.dtype == F
    inside = np.zeros(net, bool)
    inside[top:top + new_h, left:left + new_w] = True
    assert (~inside).any() and (out[:, ~inside] == F(0.5)).all()
    assert np.array_equal(out[:, top:top + new_h, left:left + new_w], R.resize(R.pixel_values(frame), new_h, new_w))
    assert (top, left) == ((net[0] - new_h) // 2, (net[1] - new_w) // 2) and (top == 0 or left == 0)
    # stretching fills the whole input and uses rows, columns = net_h, net_w
    assert darknet_target(*shape, *net, False) == (net[0], net[1], 0, 0)
    assert np.array_equal(R.stretch(frame, *net), R.resize(R.pixel_values(frame), *net))


def test_wide_tall_and_square_frames_pad_the_right_sides():
    assert R.geometry(20, 90, 32, 48) == (10, 48, 11, 0)            # wide: bands above and below
    assert R.geometry(90, 20, 32, 48) == (32, 7, 0, 20)             # tall: bands left and right
    assert R.geometry(50, 50, 32, 48) == (32, 32, 0, 8)             # square in a non-square net


def test_a_one_pixel_target_is_refused():
    with pytest.raises(ValueError):
        R.resize(_planes(5, 7, 0), 1, 9)
    with pytest.raises(ValueError):
        R.resize(_planes(5, 7, 0), 9, 1)
    with pytest.raises(ValueError):
        R.letterbox(R.random_frame(5, 5000, 0), 608, 608)           # new_h = 5 * 608 / 5000 = 0 -> clamped to 1
    with pytest.raises(ValueError, match="resize_image"):
        darknet_target(5, 5000, 608, 608, True)
    with pytest.raises(ValueError, match="resize_image"):
        darknet_target(5000, 5, 608, 608, True)
    with pytest.raises(ValueError, match="resize_image"):
        darknet_target(5, 7, 1, 9, False)
    assert darknet_target(5, 5000, 608, 608, False) == (608, 608, 0, 0)
    assert darknet_target(1, 5000, 608, 608, True) == (1, 608, 303, 0)       # a 1-pixel source may stay 1 pixel
    with pytest.raises(ValueError, match="resize_image"):           # refused before anything touches a device
        darknet_frames_device([R.random_frame(5, 5000, 0)], 608, 608, "cuda", True)
    with pytest.raises(ValueError, match="uint8"):
        darknet_frames_device([np.zeros((5, 7, 3), np.float32)], 32, 48, "cuda", True)


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

def test_header_and_binding_agree():
    with open(HEADER) as fh:
        text = fh.read()
    assert "#define Y3_CAP_PREPROCESS_DARKNET 512u" in text and "#define Y3_ABI_VERSION 6" in text
    assert _hip.CAP_PREPROCESS_DARKNET == 512 and _hip.ABI_VERSION == 6
    m = re.search(r"typedef struct \{\s*const uint8_t \*d_src;\s*int32_t ([^;]+);\s*\} y3_darknet_frame;", text)
    assert m, "y3_darknet_frame not declared"
    assert ["d_src"] + [n.strip() for n in m.group(1).split(",")] == [f[0] for f in _hip.Y3DarknetFrame._fields_]
    assert ctypes.sizeof(_hip.Y3DarknetFrame) == 16
    m = re.search(r"int y3_preprocess_darknet_f32\(([^)]*)\);", text)
    assert m, "y3_preprocess_darknet_f32 not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert [p.split()[-1].lstrip("*") for p in params] == ["frames", "batch", "d_dst", "net_h", "net_w", "letterbox", "stream"]
    restype, argtypes = _hip.PROTOTYPES["y3_preprocess_darknet_f32"]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 7
    assert argtypes[0] == ctypes.POINTER(_hip.Y3DarknetFrame)
    assert "y3_preprocess_darknet_f32" in _hip._OPTIONAL
    assert ctypes.sizeof(_hip.Y3Op) == 248 and ctypes.sizeof(_hip.Y3Options) == 64


def test_library_reports_the_capability_and_the_entry_point():
    lib = _hip.lib()
    assert lib.y3_abi_version() == 6
    assert lib.y3_capabilities() & 512 and _hip.capabilities() & _hip.CAP_PREPROCESS_DARKNET
    assert hasattr(lib, "y3_preprocess_darknet_f32")
    _hip.require_capabilities(_hip.CAP_PREPROCESS_DARKNET, "test")


def test_stale_library_is_refused(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: 511)               # everything but bit 512
    with pytest.raises(_hip.HipLibraryError, match="Darknet preprocessing"):
        _hip.require_capabilities(_hip.CAP_LETTERBOX | _hip.CAP_PREPROCESS_DARKNET, "inference(preprocess='darknet')")
    _hip.require_capabilities(_hip.CAP_LETTERBOX, "test")
    with pytest.raises(_hip.HipLibraryError, match="Darknet preprocessing"):
        darknet_frames_device([R.random_frame(5, 7, 0)], 32, 48, "cuda", False)


def _c_call(frames, batch, dst, net_h, net_w, letterbox):
    """the entry point's argument checks come before any device work: fake addresses, no GPU"""
    lib = _hip.lib()
    rc = lib.y3_preprocess_darknet_f32(frames, batch, dst, net_h, net_w, letterbox, None)
    return rc, (lib.y3_last_error() or b"").decode()


def test_entry_point_validates_its_arguments():
    fake = 1 << 44
    ok = (_hip.Y3DarknetFrame * 1)(_hip.Y3DarknetFrame(fake, 5, 7))
    for args in ((None, 1, fake, 32, 48, 0), (ok, 1, None, 32, 48, 0), (ok, 0, fake, 32, 48, 0), (ok, 1, fake, 0, 48, 0),
                 (ok, 1, fake, 32, -1, 1), (ok, 1, fake + 2, 32, 48, 0), (ok, 1, fake, 1 << 16, 1 << 16, 0)):
        rc, msg = _c_call(*args)
        assert rc == -1 and msg.startswith("y3_preprocess_darknet_f32:"), (args[1:], rc, msg)
    for h, w in ((0, 7), (5, -1), (1 << 24, 7)):
        rc, msg = _c_call((_hip.Y3DarknetFrame * 1)(_hip.Y3DarknetFrame(fake, h, w)), 1, fake, 32, 48, 0)
        assert rc == -1 and "frame 0" in msg
    rc, msg = _c_call((_hip.Y3DarknetFrame * 2)(_hip.Y3DarknetFrame(fake, 5, 7), _hip.Y3DarknetFrame(None, 5, 7)), 2, fake, 32, 48, 1)
    assert rc == -1 and "frame 1" in msg
    # a 1-pixel target of a longer source: Darknet's division by zero
    thin = (_hip.Y3DarknetFrame * 1)(_hip.Y3DarknetFrame(fake, 5, 5000))
    rc, msg = _c_call(thin, 1, fake, 608, 608, 1)
    assert rc == -1 and "resize_image" in msg and "5 x 5000" in msg and "1 x 608" in msg
    rc, msg = _c_call(ok, 1, fake, 1, 48, 0)
    assert rc == -1 and "resize_image" in msg


# ---- the option ----------------------------------------------------------------------------------------------------------------------

CALLERS = (yolov3.inference, yolov3.detect_in_frames, yolov3.detect_in_images, yolov3.detect_in_video, yolov3.detect_in_cam)


def test_the_option_is_off_by_default_everywhere():
    for fn in CALLERS + (Pipeline.__init__,):
        assert inspect.signature(fn).parameters["preprocess"].default is None, fn
    assert _hip.check_preprocess_mode(None) is None and _hip.check_preprocess_mode("darknet") == "darknet"
    assert _hip.PREPROCESS_MODES == (None, "darknet")


@pytest.mark.parametrize("bad", ["opencv", "Darknet", "", True, 1, b"darknet"])
def test_any_other_value_is_a_value_error_on_every_caller(bad):
    net = yolov3.Darknet(MINI)
    frame = np.zeros((32, 48, 3), np.uint8)
    with pytest.raises(ValueError, match="preprocess"):
        _hip.check_preprocess_mode(bad)
    with pytest.raises(ValueError, match="preprocess"):
        yolov3.inference(net, [frame], preprocess=bad)
    with pytest.raises(ValueError, match="preprocess"):
        list(yolov3.detect_in_frames(net, [frame], preprocess=bad))
    with pytest.raises(ValueError, match="preprocess"):
        yolov3.detect_in_images(net, "no_such.jpg", preprocess=bad)
    with pytest.raises(ValueError, match="preprocess"):
        yolov3.detect_in_video(net, "no_such.avi", preprocess=bad)
    with pytest.raises(ValueError, match="preprocess"):
        yolov3.detect_in_cam(net, preprocess=bad)
    with pytest.raises(ValueError, match="preprocess"):
        Pipeline(net, 2, preprocess=bad)


def test_the_mode_needs_resize():
    net = yolov3.Darknet(MINI)
    with pytest.raises(ValueError, match="resize=False"):
        yolov3.inference(net, [np.zeros((32, 48, 3), np.uint8)], preprocess="darknet", resize=False)


def test_pipeline_refuses_the_mode_by_name():
    net = yolov3.Darknet(MINI)
    with pytest.raises(ValueError, match="preprocess='darknet'.*uint8"):
        Pipeline(net, 2, preprocess="darknet")


def test_command_line_flag_reaches_the_callers(monkeypatch):
    base = ["-c", "a.cfg", "-w", "a.weights"]
    image = os.path.join(GOLDEN, "images", SAMPLE_IMAGES[0])
    assert build_parser().parse_args(base + ["-I", image, "--darknet-resize"]).darknet_resize is True
    assert build_parser().parse_args(base + ["-I", image, "--letterbox"]).darknet_resize is False

    class Seen(Exception):
        pass

    class Net(object):
        def __init__(self, *a, **kw):
            pass

        def load_weights(self, path):
            return self

        def eval(self):
            return self

        def cuda(self, device=None):
            return self

    def fake(*a, **kw):
        raise Seen("%r %r" % (kw["preprocess"], kw["letterbox"]))

    monkeypatch.setattr(yolov3, "Darknet", Net)
    for name in ("detect_in_frames", "detect_in_video", "detect_in_cam"):
        monkeypatch.setattr(stream, name, fake)
    monkeypatch.setattr(stream, "video_fps", lambda path, default: default)
    for source in (["-I", image], ["-V", image], ["-C"]):
        with pytest.raises(Seen, match="^'darknet' True$"):
            main(base + source + ["--darknet-resize", "--letterbox"])
        with pytest.raises(Seen, match="^'darknet' False$"):
            main(base + source + ["--darknet-resize", "--darknet-pool"])
        with pytest.raises(Seen, match="^None True$"):
            main(base + source + ["--letterbox"])
