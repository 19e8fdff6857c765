"""Tiled inference without a GPU: the tile grid's properties over a sweep of sizes and overlaps, the numpy statement of the
cutter against the restatement of tests/tiles_restate.py, the restatement of the tiled detection tail on hand cases, the C ABI
additions (struct sizes, prototypes, the capability bit), every refusal of ``y3_tiles_u8`` and ``y3_detect_tiled`` -- all of
them return before anything is launched -- and every refusal of ``inference(tile_overlap=...)`` and of the command line."""
import ctypes
import os
import re

import numpy as np
import pytest

import yolov3
from yolov3 import _hip, tiles
from yolov3.__main__ import build_parser, check_tiling, main

import tiles_restate as R
from golden_util import ROOT

FRACTIONS = [0.0, 0.1, 0.2, 0.25, 0.5, 0.75, 0.9]


# ---- the grid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("net", [1, 2, 7, 64, 608])
def test_axis_origins_cover_overlap_and_end_on_the_last_pixel(net):
    for f in FRACTIONS:
        ov = int(f * net)
        for length in range(1, 3 * net + 1):
            o = tiles.axis_origins(length, net, f)
            assert all(isinstance(v, int) for v in o)
            if length <= net:
                assert o == [0], (length, f)
                continue
            assert o[0] == 0 and o[-1] == length - net, (length, f, o)
            d = np.diff(o)
            assert (d >= 0).all() and (d <= net - ov).all(), (length, f, o)     # neighbours share >= ov pixels (and no gap)
            covered = np.zeros(length, bool)
            for v in o:
                covered[v:v + net] = True
            assert covered.all(), (length, f, o)
            assert len(o) == -(-(length - ov) // (net - ov))


def test_one_pixel_more_than_the_network_gives_origins_0_and_1():
    for net in (2, 7, 64, 608):
        for f in FRACTIONS:
            assert tiles.axis_origins(net + 1, net, f) == [0, 1]
    assert tiles.tile_grid(65, 33, 64, 32, 0.25) == [(0, 0), (0, 1), (1, 0), (1, 1)]


def test_grid_is_row_major_and_a_4k_frame_is_8_by_5():
    grid = tiles.tile_grid(2160, 3840, 608, 608, 0.2)
    ys, xs = tiles.axis_origins(2160, 608, 0.2), tiles.axis_origins(3840, 608, 0.2)
    assert len(ys) == 5 and len(xs) == 8 and len(grid) == 40
    assert grid == [(y, x) for y in ys for x in xs]
    assert grid[0] == (0, 0) and grid[1] == (0, xs[1]) and grid[-1] == (2160 - 608, 3840 - 608)
    assert tiles.tile_grid(100, 150, 608, 608, 0.5) == [(0, 0)]                      # fits: one padded tile
    assert tiles.tile_grid(100, 1000, 608, 608, 0.0) == [(0, 0), (0, 392)]           # one axis fits, the other does not


def test_geometry_of_plain_tiles_and_overview():
    grid = tiles.tile_grid(100, 150, 64, 64, 0.25)
    geom = tiles.tile_geometry(100, 150, 64, 64, grid, overview=True)
    assert geom[:-1] == R.plain_geom(64, 64, grid) == [(64.0, 64.0, x0, y0) for y0, x0 in grid]
    assert geom[-1] == (150.0, 100.0, 0, 0)
    assert tiles.tile_geometry(100, 150, 64, 64, grid, overview=False) == geom[:-1]


@pytest.mark.parametrize("bad", [-0.01, 0.91, 1.0, float("nan"), float("inf"), "a lot", None])
def test_overlap_outside_the_range_is_refused(bad):
    with pytest.raises(ValueError, match="tile_overlap"):
        tiles.check_overlap(bad)
    with pytest.raises(ValueError, match="tile_overlap"):
        tiles.tile_grid(100, 100, 64, 64, bad)
    assert tiles.check_overlap(0) == 0.0 and tiles.check_overlap(0.9) == 0.9


# ---- the cutter and the tail, restated ------------------------------------------------------------------------------------------
def test_numpy_cutter_equals_crop_plus_pad():
    img = R.arange_frame(33, 65)
    grid = tiles.tile_grid(33, 65, 32, 64, 0.25) + [(32, 64), (5, 0), (0, 60)]
    got = tiles.cut_tiles_u8(img, 32, 64, grid, fill=9)
    assert got.shape == (len(grid), 32, 64, 3) and got.dtype == np.uint8
    for i, (y0, x0) in enumerate(grid):
        assert np.array_equal(got[i], R.crop_pad(img, y0, x0, 32, 64, 9))
    assert (got[4, 1:] == 9).all() and (got[4, :, 1:] == 9).all() and np.array_equal(got[4, 0, 0], img[32, 64])
    small = R.arange_frame(20, 30, 5)
    one = tiles.cut_tiles_u8(small, 32, 64, [(0, 0)], fill=200)[0]
    assert np.array_equal(one[:20, :30], small) and (one[20:] == 200).all() and (one[:, 30:] == 200).all()


def test_restated_tail_truncates_before_it_adds_the_offset():
    # x * sx = -0.75 truncates to 0 (floor would give -1), 2.5 to 2; the offsets 10 / 7 come after
    box = np.array([[[-0.75 / 64, 2.5 / 64, 0.0, 0.0], [0.5, 0.5, 5.0 / 64, 4.0 / 64]]], np.float32)
    prob = np.array([[0.9, 0.8]], np.float32)
    cls = np.array([[0, 1]], np.int64)
    got, n = R.tiled_postprocess(box, prob, cls, [(64.0, 64.0, 10, 7)], 0.5, 0.3)
    assert n == 2
    order = np.argsort(got[3])
    assert got[0][order].tolist() == [[10, 9, 10, 9], [42 - 2, 39 - 2, 42 + 2, 39 + 2]]
    assert got[3][order].tolist() == [0, 1]


def test_restated_tail_keeps_one_of_an_object_seen_by_two_tiles():
    # the object at frame (56, 20), 10 x 10, seen by the tile at x0 = 0 and the one at x0 = 48; a third tile sees nothing
    box = np.zeros((3, 5, 4), np.float32)
    prob = np.zeros((3, 5), np.float32)
    cls = np.zeros((3, 5), np.int64)
    box[0, 2] = [56 / 64, 20 / 64, 10 / 64, 10 / 64]
    box[1, 4] = [8 / 64, 20 / 64, 10 / 64, 10 / 64]
    prob[0, 2], prob[1, 4] = 0.9, 0.8
    geom = [(64.0, 64.0, 0, 0), (64.0, 64.0, 48, 0), (64.0, 64.0, 96, 0)]
    got, n = R.tiled_postprocess(box, prob, cls, geom, 0.5, 0.3)
    assert n == 2 and got[3].tolist() == [2] and got[0].tolist() == [[51, 15, 61, 25]]
    prob[0, 2] = 0.8                                          # an exact tie: the higher combined row
    got, n = R.tiled_postprocess(box, prob, cls, geom, 0.5, 0.3)
    assert n == 2 and got[3].tolist() == [1 * 5 + 4]


# ---- header and bindings ---------------------------------------------------------------------------------------------------------
def test_structs_prototypes_and_the_capability_bit():
    assert ctypes.sizeof(_hip.Y3Tile) == 24 and ctypes.sizeof(_hip.Y3TileGeom) == 16
    assert [n for n, _ in _hip.Y3Tile._fields_] == ["d_src", "src_h", "src_w", "y0", "x0"]
    assert [n for n, _ in _hip.Y3TileGeom._fields_] == ["sx", "sy", "ox", "oy"]
    assert len(_hip.PROTOTYPES["y3_tiles_u8"][1]) == 7
    assert len(_hip.PROTOTYPES["y3_detect_tiled_workspace_bytes"][1]) == 3
    assert len(_hip.PROTOTYPES["y3_detect_tiled"][1]) == 17
    assert _hip.PROTOTYPES["y3_detect_tiled_workspace_bytes"][0] is ctypes.c_size_t
    for name in ("y3_tiles_u8", "y3_detect_tiled_workspace_bytes", "y3_detect_tiled"):
        assert name in _hip._OPTIONAL
        getattr(_hip.lib(), name)
    assert _hip.CAP_TILES == 8192 and _hip.capabilities() & _hip.CAP_TILES
    _hip.require_capabilities(_hip.CAP_TILES, "test")
    assert _hip.lib().y3_abi_version() == _hip.ABI_VERSION == 6 and ctypes.sizeof(_hip.Y3Op) == 248
    header = open(os.path.join(ROOT, "include", "yolov3_hip.h")).read()
    assert re.search(r"#define Y3_CAP_TILES 8192u", header)
    assert re.search(r"const uint8_t \*d_src;\s*int32_t src_h, src_w, y0, x0;\s*} y3_tile;", header)
    assert re.search(r"float sx, sy;[^}]*int32_t ox, oy;[^}]*} y3_tile_geom;", header)
    for name in ("y3_tiles_u8", "y3_detect_tiled_workspace_bytes", "y3_detect_tiled"):
        assert re.search(r"\b%s\(" % name, header)


def test_a_stale_library_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: 0x3FFF & ~_hip.CAP_TILES)
    with pytest.raises(_hip.HipLibraryError, match="tiled inference"):
        _hip.require_capabilities(_hip.CAP_TILES, "test")


def test_workspace_query():
    lib = _hip.lib()
    for batch, t, rows in ((1, 1, 10), (2, 3, 5), (1, 41, 22743), (3, 9, 1000)):
        assert lib.y3_detect_tiled_workspace_bytes(batch, t, rows) == lib.y3_detect_workspace_bytes(batch, t * rows) > 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 2, 2), (1, 1 << 16, 1 << 16)):
        assert lib.y3_detect_tiled_workspace_bytes(*bad) == 0


# ---- refusals of the two entry points: each returns before a launch -------------------------------------------------------
FAKE = 1 << 44          # stands for a device address; no call below gets as far as using one


def _tiles_u8(tile=(FAKE, 100, 200, 0, 0), n=1, tiles_ptr=True, dst=FAKE + 4096, net=(32, 64), fill=128):
    arr = (_hip.Y3Tile * 2)(_hip.Y3Tile(FAKE, 100, 200, 0, 0), _hip.Y3Tile(*tile))
    rc = _hip.lib().y3_tiles_u8(arr if tiles_ptr else None, n + 1 if n > 0 else n, dst, net[0], net[1], fill, None)
    return rc, (_hip.lib().y3_last_error() or b"").decode()


@pytest.mark.parametrize("kw,words", [
    (dict(tiles_ptr=False), "null pointer"), (dict(dst=None), "null pointer"),
    (dict(n=0), "must be positive"), (dict(n=-3), "must be positive"),
    (dict(net=(0, 64)), "must be positive"), (dict(net=(32, -1)), "must be positive"),
    (dict(net=(30000, 30000)), "too large"),
    (dict(fill=256), "not a byte"), (dict(fill=-1), "not a byte"),
    (dict(tile=(None, 100, 200, 0, 0)), "tile 1: null pointer or empty frame"),
    (dict(tile=(FAKE, 0, 200, 0, 0)), "tile 1: null pointer or empty frame"),
    (dict(tile=(FAKE, 100, -5, 0, 0)), "tile 1: null pointer or empty frame"),
    (dict(tile=(FAKE, 100, (1 << 31) - 1, 0, 0)), "columns are too many"),
    (dict(tile=(FAKE, 100, 200, 100, 0)), r"tile 1: origin \(100, 0\) lies outside its 100 x 200 frame"),
    (dict(tile=(FAKE, 100, 200, -1, 0)), "lies outside"),
    (dict(tile=(FAKE, 100, 200, 0, 200)), "lies outside"),
    (dict(tile=(FAKE, 100, 200, 0, -1)), "lies outside"),
])
def test_tiles_u8_refusals(kw, words):
    rc, msg = _tiles_u8(**kw)
    assert rc != 0 and msg.startswith("y3_tiles_u8: ") and re.search(words, msg), msg


_TAIL_POINTERS = ("d_bbox", "d_prob", "d_cls", "d_geom", "d_workspace", "d_det_count", "d_det_tlbr", "d_det_prob", "d_det_cls",
                  "d_det_row")


def _detect_tiled(batch=1, n_tiles=3, rows=5, ws_bytes=None, null=None):
    lib = _hip.lib()
    p = {name: FAKE + 4096 * i for i, name in enumerate(_TAIL_POINTERS)}
    if null:
        p[null] = None
    if ws_bytes is None:
        ws_bytes = lib.y3_detect_tiled_workspace_bytes(batch, n_tiles, rows)
    elif ws_bytes == "one tile":                             # what y3_detect asks for one tile's rows is not enough
        ws_bytes = lib.y3_detect_workspace_bytes(batch, rows)
    rc = lib.y3_detect_tiled(p["d_bbox"], p["d_prob"], p["d_cls"], batch, n_tiles, rows, p["d_geom"], 0.5, 0.3, p["d_workspace"],
                             ws_bytes, p["d_det_count"], p["d_det_tlbr"], p["d_det_prob"], p["d_det_cls"], p["d_det_row"], None)
    return rc, (lib.y3_last_error() or b"").decode()


@pytest.mark.parametrize("kw,words", [
    (dict(n_tiles=0), "tiles must be positive"), (dict(n_tiles=-1), "tiles must be positive"),
    (dict(batch=0), "batch and rows must be positive"), (dict(rows=0), "batch and rows must be positive"),
    (dict(n_tiles=1 << 16, rows=1 << 16, ws_bytes=0), "too many for one frame"),
    (dict(batch=1 << 16, n_tiles=1 << 16, rows=1, ws_bytes=0), "too many"),
    (dict(ws_bytes=0), "workspace too small"),
    (dict(ws_bytes="one tile"), "workspace too small"),
] + [(dict(null=name), "null pointer") for name in _TAIL_POINTERS])
def test_detect_tiled_refusals(kw, words):
    rc, msg = _detect_tiled(**kw)
    assert rc != 0 and msg.startswith("y3_detect_tiled: ") and words in msg, msg


# ---- refusals of inference() and of the command line ------------------------------------------------------------------------
class _NoDevice(object):
    """Stands for a network: touching anything but ``multi_label`` is an AttributeError, not the ValueError asked for."""

    def __init__(self, multi_label=False):
        self.multi_label = multi_label


@pytest.mark.parametrize("kw,words", [
    (dict(letterbox=True), "letterbox=True"),
    (dict(preprocess="darknet"), "preprocess='darknet'"),
    (dict(resize=False), "resize=False"),
    (dict(nms_kind="iou"), "nms_kind='iou'"), (dict(nms_kind="diounms"), "nms_kind='diounms'"),
    (dict(multi_label=True), "multi_label"),
    (dict(tile_overlap=0.95), "tile_overlap"), (dict(tile_overlap=-0.1), "tile_overlap"),
    (dict(tile_fill=256), "fill"), (dict(tile_batch=0), "tile_batch"),
])
def test_inference_refuses_before_it_touches_a_device(kw, words):
    kw = dict(kw)
    net = _NoDevice(kw.pop("multi_label", False))
    kw.setdefault("tile_overlap", 0.25)
    with pytest.raises(ValueError, match=re.escape(words)):
        yolov3.inference(net, [np.zeros((100, 150, 3), np.uint8)], **kw)


BASE = ["-c", "a.cfg", "-w", "a.weights"]


def test_parser_accepts_the_tiling_flags():
    args = build_parser().parse_args(BASE + ["-I", "x.jpg", "--tile-overlap", "0.2", "--no-tile-overview"])
    assert args.tile_overlap == 0.2 and args.no_tile_overview is True
    args = build_parser().parse_args(BASE + ["-I", "x.jpg"])
    assert args.tile_overlap is None and args.no_tile_overview is False
    check_tiling(vars(args))
    check_tiling(vars(build_parser().parse_args(BASE + ["-I", "x.jpg", "--tile-overlap", "0.9"])))


@pytest.mark.parametrize("extra,words", [
    (["-V", "x.mp4", "--tile-overlap", "0.2"], "video or camera"),
    (["-C", "0", "--tile-overlap", "0.2"], "video or camera"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--letterbox"], "letterbox"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--darknet-resize"], "preprocess"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--nms-kind", "greedynms"], "nms_kind"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--multi-label"], "multi_label"),
    (["-I", "x.jpg", "--tile-overlap", "0.95"], "tile_overlap"),
    (["-I", "x.jpg", "--no-tile-overview"], "--tile-overlap"),
])
def test_command_line_refusals_come_before_anything_is_loaded(extra, words):
    # a.cfg does not exist: getting as far as the network would be another error
    with pytest.raises(SystemExit) as exc:
        main(BASE + extra)
    assert words in str(exc.value) and str(exc.value).startswith("yolov3: ")
