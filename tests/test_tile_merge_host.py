"""The seam merge of tiled inference without a GPU: ``tiles.merge_detections`` against the restatement of
tests/tile_merge_restate.py on the whole case table (tests/tile_merge_cases.py), the hand-computed answers of the planted cases,
the evidence that the table tells the right rule from each of five wrong ones, the rule's consequences (identity at 1.0 and on
one tile, canonical output order, members summing to the input), the C ABI additions, every refusal of ``y3_merge_tiled`` -- all
return before anything is launched -- every refusal of ``inference(tile_merge=...)`` and of the command line, and the new
library's code object."""
import ctypes
import os
import re

import numpy as np
import pytest

import yolov3
from yolov3 import _hip
from yolov3.__main__ import build_parser, check_tiling, main
from yolov3.tiles import check_merge, merge_detections

import code_object
import kernel_census as census
import tile_merge_cases as C
import tile_merge_restate as M
from golden_util import ROOT

CALLS = [(c, thr) for c in C.CASES for thr in c.thrs]
IDS = ["%s @ %r" % (c.name, thr) for c, thr in CALLS]


def _same(got, want):
    assert len(got) == len(want) == 5
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert got[1].tobytes() == want[1].tobytes()              # score bits


def _differs(a, b):
    return len(a[4]) != len(b[4]) or any(not np.array_equal(x, y) for x, y in zip(a, b))


# ---- the rule -----------------------------------------------------------------------------------------------------------------------
def test_the_table_is_in_canonical_order_and_holds_what_the_issue_lists():
    for c in C.CASES:
        for b in range(c.batch):
            box, prob, cls, row = c.frame(b)
            assert C.is_canonical(prob, cls, row), c.name
            assert row.min(initial=0) >= 0 and row.max(initial=0) < c.capacity
    by = C.BY_NAME
    seg = np.unique(by["segments 1 63 64 65 129 1500"].frame(0)[2], return_counts=True)[1]
    assert seg.tolist() == [1, 63, 64, 65, 129, 1500]
    # absorptions cross the chunk boundaries: in the segment of 129 (and in that of 1500) a keeper of chunk 0 takes a lane of
    # chunk 2 or later -- from the restatement's owners, per class segment
    case = by["segments 1 63 64 65 129 1500"]
    box, prob, cls, row = case.frame(0)
    owners = M.merge(box.tolist(), prob.tolist(), cls.tolist(), row.tolist(), case.tile_rows, 0.5, owners=True)
    for size in (129, 1500):
        start = int(np.flatnonzero(cls == seg.tolist().index(size))[0])
        far = [(k - start, j - start) for j, k in enumerate(owners) if k is not None and start <= k < start + 64 <= start + 128 <= j < start + size]
        assert far, size
        if size == 129:
            assert (42, 128) in far          # the keeper at lane 42 of chunk 0 takes lane 0 of chunk 2
    assert len(np.unique(by["80 classes"].frame(0)[2])) == 80 and len(np.unique(by["2000 classes"].frame(0)[2])) == 2000
    assert [by["batch tile_rows 500"].count.tolist(), by["batch tile_rows 1000"].tile_rows] == [[0, 1, 300], 1000]
    full = by["count equals capacity"]
    assert int(full.count[0]) == full.capacity
    negative = by["negative"].frame(0)[0]
    assert np.abs(by["wide"].frame(0)[0]).max() > 40000 and negative.min() < -16000 < negative[:, 0].max()
    # a narrow first chunk and a wide second one in one class
    box = by["narrow chunk meets wide chunk"].frame(0)[0]
    assert np.abs(box[:64]).max() < 16000 and np.abs(box[64:128]).max() > 16000 and np.abs(box[64:128]).min() < 16000
    for name in C.RANDOM:
        box, prob, cls, row = by[name].frame(0)
        assert len(box) == 600 and len(np.unique(cls)) == 3 and sorted(set((row // 1000).tolist())) == list(range(7))


@pytest.mark.parametrize("case,thr", CALLS, ids=IDS)
def test_numpy_twin_equals_the_restatement(case, thr):
    for b in range(case.batch):
        got = merge_detections(*case.frame(b), case.tile_rows, thr)
        _same(got, C.expected(case, b, thr))


@pytest.mark.parametrize("key", sorted(C.PLANTED, key=str), ids=str)
def test_planted_cases_give_the_answers_computed_by_hand(key):
    name, thr = key
    box, prob, cls, row, members = C.expected(C.BY_NAME[name], 0, thr)
    got = [(tuple(b), float(p), int(r), int(m)) for b, p, r, m in zip(box.tolist(), prob, row, members)]
    want = [(b, float(np.float32(p)), r, m) for b, p, r, m in C.PLANTED[key]]
    assert got == want


def test_the_measures_of_the_two_halves():
    a, b = (10, 10, 40, 50), (30, 10, 70, 50)
    assert M.intersection(a, b) == 451 and min(M.measures(a)[2], M.measures(b)[2]) == 1271
    assert M.ios(a, b) == 451 / 1271 and round(M.iou(a, b), 2) == 0.18
    assert M.ios((0, 0, 9, 9), (5, 0, 14, 9)) == 0.5


@pytest.mark.parametrize("wrong", M.WRONG_RULES)
def test_each_wrong_rule_is_told_apart_by_a_planted_case_and_by_every_random_frame(wrong):
    name, thr = C.TELLS[wrong]
    case = C.BY_NAME[name]
    assert _differs(C.expected(case, 0, thr, wrong), C.expected(case, 0, thr)), name
    for name in C.RANDOM:
        case = C.BY_NAME[name]
        assert _differs(C.expected(case, 0, 0.5, wrong), C.expected(case, 0, 0.5)), name


def test_random_frames_keep_about_290_of_600_in_groups_of_up_to_15():
    for name in C.RANDOM:
        members = C.expected(C.BY_NAME[name], 0, 0.5)[4]
        print(name, len(members), int(members.max()))
        assert 275 <= len(members) <= 305 and 10 <= members.max() <= 15


@pytest.mark.parametrize("case", C.CASES, ids=[c.name for c in C.CASES])
def test_threshold_one_is_the_identity(case):
    for b in range(case.batch):
        box, prob, cls, row = case.frame(b)
        for got in (merge_detections(box, prob, cls, row, case.tile_rows, 1.0), C.expected(case, b, 1.0)):
            _same(got, (box, prob, cls, row, np.ones(len(row), np.int32)))


def test_one_tile_is_the_identity():
    for case in C.CASES:
        for b in range(case.batch):
            box, prob, cls, row = case.frame(b)
            got = merge_detections(box, prob, cls, row, case.capacity, 0.0)      # tile_rows = capacity: one tile
            _same(got, (box, prob, cls, row, np.ones(len(row), np.int32)))
    one = C.BY_NAME["one tile"]
    assert int(one.count[0]) == 200 and len(C.expected(one, 0, 0.0)[4]) == 200


@pytest.mark.parametrize("case,thr", CALLS, ids=IDS)
def test_output_is_canonical_a_subset_and_members_sum_to_the_input(case, thr):
    for b in range(case.batch):
        box, prob, cls, row, members = C.expected(case, b, thr)
        assert C.is_canonical(prob, cls, row) or len(row) < 2
        assert int(members.sum()) == int(case.count[b]) and (members >= 1).all()
        in_rows = case.frame(b)[3].tolist()
        assert set(row.tolist()) <= set(in_rows)
        # a keeper's box holds its own
        own = case.frame(b)[0][[in_rows.index(r) for r in row.tolist()]]
        assert (box[:, :2] <= own[:, :2]).all() and (box[:, 2:] >= own[:, 2:]).all()
        assert np.array_equal(box[members == 1], own[members == 1])


# ---- header and bindings ---------------------------------------------------------------------------------------------------------
def test_prototypes_and_the_capability_bit():
    assert len(_hip.PROTOTYPES["y3_merge_tiled_workspace_bytes"][1]) == 2
    assert _hip.PROTOTYPES["y3_merge_tiled_workspace_bytes"][0] is ctypes.c_size_t
    assert len(_hip.PROTOTYPES["y3_merge_tiled"][1]) == 18 and _hip.PROTOTYPES["y3_merge_tiled"][1][8] is ctypes.c_double
    for name in ("y3_merge_tiled_workspace_bytes", "y3_merge_tiled"):
        assert name in _hip._OPTIONAL
        getattr(_hip.lib(), name)
    assert _hip.CAP_TILE_MERGE == 65536 and _hip.capabilities() & _hip.CAP_TILE_MERGE
    _hip.require_capabilities(_hip.CAP_TILE_MERGE, "test")
    assert _hip.lib().y3_abi_version() == _hip.ABI_VERSION == 6 and ctypes.sizeof(_hip.Y3Op) == 248
    header = open(os.path.join(ROOT, "include", "yolov3_hip.h")).read()
    assert re.search(r"#define Y3_CAP_TILE_MERGE 65536u", header) and re.search(r"#define Y3_ABI_VERSION 6\b", header)
    assert re.search(r"size_t y3_merge_tiled_workspace_bytes\(int batch, int capacity\);", header)
    proto = re.search(r"int y3_merge_tiled\(([^;]*)\);", header).group(1)
    assert [a.split()[-1].lstrip("*") for a in proto.split(",")] == [
        "d_det_count", "d_det_tlbr", "d_det_prob", "d_det_cls", "d_det_row", "batch", "capacity", "tile_rows", "thr", "d_workspace",
        "workspace_bytes", "d_out_count", "d_out_tlbr", "d_out_prob", "d_out_cls", "d_out_row", "d_out_members", "stream"]
    assert "y3_detect_tiled itself is unchanged" in header


def test_a_stale_library_is_refused_by_name(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: 0xFFFFFFFF & ~_hip.CAP_TILE_MERGE)
    with pytest.raises(_hip.HipLibraryError, match="tile seam merging"):
        _hip.require_capabilities(_hip.CAP_TILE_MERGE, "test")
    with pytest.raises(_hip.HipLibraryError, match="tile seam merging"):
        _hip.require_capabilities(_hip.CAP_TILES | _hip.CAP_TILE_MERGE, "test")


def test_workspace_query():
    lib = _hip.lib()
    sizes = [lib.y3_merge_tiled_workspace_bytes(b, c) for b, c in ((1, 1), (1, 3000), (3, 3000), (2, 41 * 22743))]
    assert all(s > 0 for s in sizes) and sizes[1] < sizes[2] < sizes[3] and sizes[2] >= 3 * 3000 * 16
    for bad in ((0, 1), (1, 0), (-1, 5), (5, -1)):
        assert lib.y3_merge_tiled_workspace_bytes(*bad) == 0


# ---- refusals of the entry point: each returns before a launch ------------------------------------------------------------------
FAKE = 1 << 44          # stands for a device address; no call below gets as far as using one
_POINTERS = ("d_det_count", "d_det_tlbr", "d_det_prob", "d_det_cls", "d_det_row", "d_workspace", "d_out_count", "d_out_tlbr",
             "d_out_prob", "d_out_cls", "d_out_row", "d_out_members")


def _merge_tiled(batch=2, capacity=3000, tile_rows=1000, thr=0.5, ws_bytes=None, null=None, alias=None):
    lib = _hip.lib()
    p = {name: FAKE + (1 << 24) * i for i, name in enumerate(_POINTERS)}       # 16 MiB apart: nothing overlaps
    if null:
        p[null] = None
    if alias:
        out, inp, shift = alias
        p[out] = p[inp] + shift
    if ws_bytes is None:
        ws_bytes = lib.y3_merge_tiled_workspace_bytes(max(batch, 1), max(capacity, 1))
    rc = lib.y3_merge_tiled(p["d_det_count"], p["d_det_tlbr"], p["d_det_prob"], p["d_det_cls"], p["d_det_row"], batch, capacity,
                            tile_rows, thr, p["d_workspace"], ws_bytes, p["d_out_count"], p["d_out_tlbr"], p["d_out_prob"],
                            p["d_out_cls"], p["d_out_row"], p["d_out_members"], None)
    return rc, (lib.y3_last_error() or b"").decode()


@pytest.mark.parametrize("kw,words", [
    (dict(batch=0), "batch must be positive"), (dict(batch=-2), "batch must be positive"),
    (dict(capacity=0), "capacity must be positive"), (dict(capacity=-1000), "capacity must be positive"),
    (dict(tile_rows=0), "tile_rows must be positive"), (dict(tile_rows=-1000), "tile_rows must be positive"),
    (dict(tile_rows=999), "capacity 3000 is no multiple of tile_rows 999"), (dict(tile_rows=6000), "no multiple of tile_rows"),
    (dict(thr=float("nan")), "thr must be a finite number in [0, 1]"), (dict(thr=float("inf")), "thr must be"),
    (dict(thr=-1e-9), "thr must be"), (dict(thr=1.0000001), "thr must be"), (dict(thr=float("-inf")), "thr must be"),
    (dict(ws_bytes=0), "workspace too small"), (dict(ws_bytes="one short"), "workspace too small"),
    (dict(alias=("d_out_tlbr", "d_det_tlbr", 0)), "d_out_tlbr aliases d_det_tlbr"),
    (dict(alias=("d_out_count", "d_det_count", 4)), "d_out_count aliases d_det_count"),
    (dict(alias=("d_out_prob", "d_det_cls", 2 * 3000 * 8 - 4)), "d_out_prob aliases d_det_cls"),
    (dict(alias=("d_out_row", "d_det_prob", -2 * 3000 * 4 + 4)), "d_out_row aliases d_det_prob"),
    (dict(alias=("d_out_members", "d_det_row", 400)), "d_out_members aliases d_det_row"),
    (dict(alias=("d_out_cls", "d_det_tlbr", 8)), "d_out_cls aliases d_det_tlbr"),
    (dict(alias=("d_workspace", "d_det_tlbr", 64)), "d_workspace aliases d_det_tlbr"),
] + [(dict(null=name), "%s is null" % name) for name in _POINTERS if name != "d_out_members"])
def test_merge_tiled_refusals(kw, words):
    if kw.get("ws_bytes") == "one short":
        kw = dict(kw, ws_bytes=_hip.lib().y3_merge_tiled_workspace_bytes(2, 3000) - 1)
    rc, msg = _merge_tiled(**kw)
    assert rc != 0 and msg.startswith("y3_merge_tiled: ") and words in msg, msg


def test_buffers_that_only_touch_are_not_aliases():
    # an output that begins where an input ends passes the alias check; the workspace's size is checked after it, so that
    # refusal shows that the call got past the alias check
    rc, msg = _merge_tiled(alias=("d_out_prob", "d_det_prob", 2 * 3000 * 4), ws_bytes=0)
    assert rc != 0 and "workspace too small" in msg
    rc, msg = _merge_tiled(alias=("d_out_prob", "d_det_prob", 2 * 3000 * 4 - 1), ws_bytes=1 << 30)
    assert rc != 0 and "d_out_prob aliases d_det_prob" in msg


# ---- refusals of inference() and of the command line ------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-0.01, 1.01, float("nan"), float("inf"), "0.5", None, [0.5], True])
def test_check_merge_refuses_what_is_no_number_in_0_1(bad):
    with pytest.raises(ValueError, match="tile_merge must be a number in"):
        check_merge(bad)


def test_check_merge_returns_a_float():
    for ok in (0, 1, 0.5, np.float32(0.25), np.float64(1.0)):
        got = check_merge(ok)
        assert type(got) is float and got == float(ok)


class _NoDevice(object):
    """Stands for a network: touching anything but ``multi_label`` is an AttributeError, not the ValueError asked for."""
    multi_label = False


@pytest.mark.parametrize("kw,words", [
    (dict(tile_merge=0.5), "tile_merge needs tile_overlap"),
    (dict(tile_merge=0.5, tile_overlap=None), "tile_overlap"),
    (dict(tile_merge=1.5, tile_overlap=0.25), "tile_merge must be a number in [0, 1]"),
    (dict(tile_merge=float("nan"), tile_overlap=0.25), "tile_merge must be a number in [0, 1]"),
    (dict(tile_merge="half", tile_overlap=0.25), "tile_merge must be a number in [0, 1]"),
    (dict(tile_merge=0.5, tile_overlap=0.25, letterbox=True), "letterbox=True"),
])
def test_inference_refuses_before_it_touches_a_device(kw, words):
    with pytest.raises(ValueError, match=re.escape(words)):
        yolov3.inference(_NoDevice(), [np.zeros((100, 150, 3), np.uint8)], **kw)


BASE = ["-c", "a.cfg", "-w", "a.weights"]


def test_parser_accepts_the_merge_flag():
    args = build_parser().parse_args(BASE + ["-I", "x.jpg", "--tile-overlap", "0.2", "--tile-merge", "0.5"])
    assert args.tile_overlap == 0.2 and args.tile_merge == 0.5
    check_tiling(vars(args))
    args = build_parser().parse_args(BASE + ["-I", "x.jpg", "--tile-overlap", "0.2"])
    assert args.tile_merge is None
    check_tiling(vars(args))
    check_tiling(vars(build_parser().parse_args(BASE + ["-I", "x.jpg", "--tile-overlap", "0", "--tile-merge", "1"])))


@pytest.mark.parametrize("extra,words", [
    (["-I", "x.jpg", "--tile-merge", "0.5"], "--tile-overlap"),
    (["-V", "x.mp4", "--tile-merge", "0.5"], "--tile-overlap"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--tile-merge", "1.5"], "--tile-merge refused: tile_merge must be a number in [0, 1]"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--tile-merge", "nan"], "--tile-merge refused"),
    (["-I", "x.jpg", "--tile-overlap", "0.2", "--tile-merge", "-0.5"], "--tile-merge refused"),
    (["-V", "x.mp4", "--tile-overlap", "0.2", "--tile-merge", "0.5"], "video or camera"),
])
def test_command_line_refusals_come_before_anything_is_loaded(extra, words):
    # a.cfg does not exist: getting as far as the network would be another error
    with pytest.raises(SystemExit) as exc:
        main(BASE + extra)
    assert words in str(exc.value) and str(exc.value).startswith("yolov3: ")


# ---- the code object ----------------------------------------------------------------------------------------------------------------
def test_merge_library_holds_the_kernel_without_scratch_and_within_64_kib_of_lds():
    kernels = census.kernels("tilemerge")          # (asserts: built, device code for gfx950 only)
    assert len(kernels) == 1 and "tile_merge_kernel" in kernels[0][".name"]
    k = kernels[0]
    assert k[".private_segment_fixed_size"] == 0, "scratch memory (register spills)"
    assert k[".group_segment_fixed_size"] <= 65536
    assert k[".max_flat_workgroup_size"] == 1024 and k[".wavefront_size"] == 64
    assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 128          # 16 waves of one workgroup on one CU


def test_main_library_names_the_merge_library_and_does_not_hold_its_kernel():
    with open(code_object.LIB, "rb") as fh:
        data = fh.read()
    assert b"libyolov3_hip_tilemerge.so" in data and b"$ORIGIN" in data
    assert b"tile_merge_kernel" not in data
    assert not any("tile_merge" in k[".name"] for k in census.kernels("main"))
