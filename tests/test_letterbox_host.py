"""Darknet letterboxing without a GPU: the geometry (hand-computed cases, and the Python definition against the library's
``y3_letterbox_geometry``), the host letterbox ``preprocess.letterbox_u8``, the box correction
``preprocess.correct_letterbox_boxes`` on hand cases, the C ABI additions and the ``--letterbox`` flag."""
import ctypes

import numpy as np
import pytest

from yolov3 import _hip
from yolov3.__main__ import build_parser
from yolov3.preprocess import correct_letterbox_boxes, letterbox_geometry, letterbox_u8, resize_bilinear_u8

HAND = [
    ((1080, 1920), (608, 608), (342, 608, 133, 0)),
    ((480, 640), (416, 416), (312, 416, 52, 0)),
    ((640, 427), (608, 608), (608, 405, 0, 101)),
    ((427, 640), (608, 608), (405, 608, 101, 0)),      # delta 203: the image moves by 101, the boxes by 101.5
    ((1216, 1216), (608, 608), (608, 608, 0, 0)),
    ((1080, 1920), (256, 416), (234, 416, 11, 0)),     # a rectangular network
    ((608, 608), (608, 608), (608, 608, 0, 0)),
]


def _c_geometry(h, w, net_h, net_w):
    out = (ctypes.c_int32 * 4)()
    _hip.check(_hip.lib().y3_letterbox_geometry(h, w, net_h, net_w, out))
    return tuple(out)


@pytest.mark.parametrize("frame,net,want", HAND)
def test_geometry_hand_cases(frame, net, want):
    assert letterbox_geometry(*frame, *net) == want
    assert _c_geometry(*frame, *net) == want


def test_geometry_clamps_to_one_pixel():
    # 1 x 5000 into 608: 1 * 608 / 5000 truncates to 0, which Darknet would turn into an empty image
    assert letterbox_geometry(1, 5000, 608, 608) == (1, 608, 303, 0)
    assert letterbox_geometry(5000, 1, 608, 608) == (608, 1, 0, 303)
    assert _c_geometry(1, 5000, 608, 608) == (1, 608, 303, 0)
    assert _c_geometry(5000, 1, 608, 608) == (608, 1, 0, 303)


def test_geometry_python_equals_library_on_a_grid():
    sizes = [1, 2, 3, 7, 100, 255, 256, 415, 416, 417, 427, 480, 511, 512, 607, 608, 609, 640, 720, 1080, 1216, 1920, 4000]
    nets = [(416, 416), (512, 512), (608, 608), (256, 416), (608, 320)]
    for net_h, net_w in nets:
        for h in sizes:
            for w in sizes:
                assert letterbox_geometry(h, w, net_h, net_w) == _c_geometry(h, w, net_h, net_w), (h, w, net_h, net_w)


def test_geometry_refuses_empty_sizes():
    with pytest.raises(ValueError):
        letterbox_geometry(0, 5, 608, 608)
    out = (ctypes.c_int32 * 4)()
    assert _hip.lib().y3_letterbox_geometry(0, 5, 608, 608, out) != 0
    assert _hip.lib().y3_letterbox_geometry(5, 5, 608, -1, out) != 0


def test_library_reports_letterbox():
    assert _hip.CAP_LETTERBOX == 16
    assert _hip.capabilities() & _hip.CAP_LETTERBOX
    _hip.require_capabilities(_hip.CAP_LETTERBOX, "test")
    for name in ("y3_letterbox_geometry", "y3_letterbox_u8", "y3_detect_letterbox"):
        assert name in _hip.PROTOTYPES and name in _hip._OPTIONAL
        getattr(_hip.lib(), name)
    assert ctypes.sizeof(_hip.Y3LetterboxFrame) == 32
    assert _hip.lib().y3_abi_version() == _hip.ABI_VERSION == 6


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("shape,net", [((1080, 1920), (608, 608)), ((640, 427), (608, 608)), ((427, 640), (416, 416)),
                                       ((31, 17), (416, 416)), ((1080, 1920), (256, 416)), ((2, 1500), (608, 608))])
@pytest.mark.parametrize("fill", [0, 128, 255])
def test_letterbox_u8_border_and_interior(shape, net, fill):
    img = _frame(*shape, seed=sum(shape))
    out = letterbox_u8(img, *net, fill=fill)
    new_h, new_w, top, left = letterbox_geometry(*shape, *net)
    assert out.shape == (net[0], net[1], 3) and out.dtype == np.uint8
    assert np.array_equal(out[top:top + new_h, left:left + new_w], resize_bilinear_u8(img, new_h, new_w))
    border = np.ones(net, dtype=bool)
    border[top:top + new_h, left:left + new_w] = False
    assert border.any()
    assert (out[border] == fill).all()


def test_letterbox_u8_identities():
    img = _frame(608, 608, seed=1)
    assert np.array_equal(letterbox_u8(img, 608, 608), img)                  # net-sized: unchanged
    big = _frame(1216, 1216, seed=2)
    assert np.array_equal(letterbox_u8(big, 608, 608), resize_bilinear_u8(big, 608, 608))   # the net's aspect: plain resize


def test_letterbox_u8_refuses_a_fill_that_is_no_byte():
    with pytest.raises(ValueError):
        letterbox_u8(_frame(10, 20, 0), 416, 416, fill=256)


def test_correct_boxes_hand_cases():
    # (304, 608) into 608: new (304, 608), top 152.  x keeps, y: (0.5 - 152 / 608) / 0.5 = 0.5, h doubles
    got = correct_letterbox_boxes(np.array([[[0.5, 0.5, 0.25, 0.25]]], np.float32), [[304, 608]], 608, 608)
    assert got.dtype == np.float32
    assert got.tolist() == [[[0.5, 0.5, 0.25, 0.5]]]
    # (427, 640) into 608: new_h 405, delta 203 -- the correction subtracts 101.5 / 608, not the image's integer 101
    y = np.array([101.5 / 608, 506.5 / 608, 0.5, 101.0 / 608], np.float32)
    box = np.stack([np.full(4, 0.25, np.float32), y, np.full(4, 0.1, np.float32), np.full(4, 0.2, np.float32)], axis=1)
    got = correct_letterbox_boxes(box, [427, 640], 608, 608)
    ratio = np.float32(405) / np.float32(608)
    want_y = ((y.astype(np.float64) - 203.0 / 2.0 / 608.0) / np.float64(ratio)).astype(np.float32)
    assert np.array_equal(got[:, 1], want_y)
    np.testing.assert_allclose(got[:, 1], [0.0, 1.0, 0.5, -0.5 / 405], atol=1e-6)
    assert abs(got[3, 1]) > 1e-3                      # the integer shift would have given 0 there
    assert np.array_equal(got[:, 0], box[:, 0]) and np.array_equal(got[:, 2], box[:, 2])
    assert np.array_equal(got[:, 3], box[:, 3] * (np.float32(1.0) / ratio))
    np.testing.assert_allclose(got[:, 3], 0.2 * 608 / 405, rtol=1e-6)


def test_correct_boxes_is_the_identity_on_net_sized_frames():
    rng = np.random.default_rng(3)
    box = rng.uniform(-0.5, 1.5, size=(2, 50, 4)).astype(np.float32)
    got = correct_letterbox_boxes(box, [[416, 416], [416, 416]], 416, 416)
    assert np.array_equal(got.view(np.uint32), box.view(np.uint32))


def test_parser_accepts_letterbox():
    args = build_parser().parse_args(["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg", "--letterbox"])
    assert args.letterbox is True
    args = build_parser().parse_args(["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg"])
    assert args.letterbox is False
