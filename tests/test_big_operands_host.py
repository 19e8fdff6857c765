"""Operands past 4 GiB and ops of 2^31 pixels, without a GPU (tests/footprint_util.py big_cases(); the GPU half is
tests/test_gpu_big_operands.py).  The choosers run on fake addresses, as in tests/test_footprint_host.py.

  * every kernel family has a row of big_cases() whose activation operands span more than 2^32 bytes plus one frame and whose
    chooser still names the family at that size -- or a PROVEN bound: the largest operand the family's own chooser rule lets it
    have lies below 2^31 bytes (BIG_BOUNDED);
  * plan creation refuses every row once an op of it has more than MAX_PIXELS = 2^31 - 1 - 256 input or output pixels (DESIGN.md
    section 1 has the audit: which 32-bit quantity of which kernel that protects), or once the launch of its kernel would hold
    more than MAX_THREADS = 2^32 - 256 threads (footprint_util.launch_threads restates every launcher's grid x block): each row
    is taken at the family's true limit and refused one frame later, by name;
  * the fused groups whose lanes hold 32-bit offsets from a tile's base divert to the unfused kernels where a row of the map
    outgrows those, the fused block at 2^32 bytes, the SPP pyramid at its launch limit;
  * the checker of the GPU test reports a shifted frame, a frame left at its prefill and a changed pad byte, and passes a clean
    tensor."""
import ctypes
import json

import pytest
import torch

import footprint_util as fu
from kernel_choice_util import FIXTURE

MARKER = "(fused into the previous op)"
TAGS = ("f32", "bf16", "f16")


def _no_gpu():
    if torch.cuda.is_available():
        pytest.skip("fake device addresses must never reach a library that can see a GPU")


def _create(case, dtype, mode="strided"):
    """(kernel names, None) or (None, the library's error message) of plan creation for ``case``"""
    H = fu._H()
    lib = H.lib()
    opt = H.options(**fu._opts()[case["opt"]])
    ops, lay, _, _ = fu.build(case, dtype, mode, opt)
    handle = ctypes.c_void_p()
    rc = lib.y3_plan_create_ex(ops, len(ops), lay["zero page"].ptr(1 << 44), ctypes.byref(opt), ctypes.byref(handle))
    if rc != 0:
        return None, lib.y3_last_error().decode()
    try:
        return [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))], None
    finally:
        lib.y3_plan_destroy(handle)


def _names(fam):
    return {fam % t for t in TAGS} if "%s" in fam else {fam}


# ------------------------------------------------------------------------------------------------ the table

def test_every_family_has_a_big_row_or_a_proven_bound():
    """no skip list: a family of the kernel-choice fixture or of cases() with neither fails here"""
    big = {c["family"] for c in fu.big_cases()}
    assert not (big & set(fu.BIG_BOUNDED)), sorted(big & set(fu.BIG_BOUNDED))
    covered = big | set(fu.BIG_BOUNDED)
    assert {c["family"] for c in fu.cases()} == covered, sorted({c["family"] for c in fu.cases()} ^ covered)
    with open(FIXTURE) as f:
        fixture = {r[0] for r in json.load(f)["rows"]} - {MARKER}
    reach = set().union(*(_names(f) for f in covered))
    assert fixture - reach == set(), "families without a big row or a bound: %s" % sorted(fixture - reach)
    # one row per family, each derived from a row of cases() of that family, float32 where the family has it, bf16 always
    # (the VALU stem on uint8 frames has two: float32, and the 48-channel row that alone reaches it in 16 bits)
    pairs = [(c["family"], d) for c in fu.big_cases() for d in c["dtypes"]]
    assert len(set(pairs)) == len(pairs) and len(fu.big_cases()) == len(big) + 1
    for c in fu.big_cases():
        src = fu.case_by_id(c["src"])
        assert src["family"] == c["family"] and src["opt"] == c["opt"], c["id"]
        for key in ("cin", "cout", "c", "k", "s", "res", "inp", "pad", "kind", "dk", "wide", "form3d", "n_anchor", "ncls", "ld", "c0"):
            assert src.get(key) == c.get(key), (c["id"], key)
        assert set(c["dtypes"]) == set(src["dtypes"]) - {"fp16"}, c["id"]
        assert "bf16" in c["dtypes"] or c["id"] == "stem_u8_f32_ragged", c["id"]
    for fam, src in fu.BIG_BOUNDED.items():
        assert fu.case_by_id(src)["family"] == fam


def test_big_rows_span_4_gib_on_odd_maps_and_keep_their_family():
    _no_gpu()
    H = fu._H()
    n = 0
    for row in fu.big_cases():
        for dtype in row["dtypes"]:
            case = fu.big_case(row, dtype)
            names, lay = fu.chosen(case, dtype, "strided")
            assert names[0] == fu.family_name(row, dtype) and all(x == MARKER for x in names[1:]), (row["id"], dtype, names)
            ops, _, _, _ = fu.build(case, dtype, "strided", H.options(**fu._opts()[row["opt"]]))
            for op in ops:
                assert max(op.batch * op.in_h * op.in_w, op.batch * op.out_h * op.out_w) <= fu.MAX_PIXELS
            spans = fu.span_operands(row, lay)
            assert spans, row["id"]
            if fu._is_frames_input(row):
                assert [o.name for o in spans] == ["output"], row["id"]
            for o in spans:
                frame = o.body_bytes // case["B"]
                assert frame * case["B"] == o.body_bytes == o.pixels * o.ld * o.es
                if row["group"] == "block":
                    # x and z: within one frame BELOW 2^32 bytes
                    assert fu.SPAN - frame <= o.body_bytes < fu.SPAN, (row["id"], o.name)
                else:
                    assert o.body_bytes > fu.SPAN + frame, (row["id"], dtype, o.name, o.body_bytes)
                # a frame's byte size divides neither 2^31 nor 2^32: a wrapped address lands mid-frame
                assert frame & (frame - 1) != 0, (row["id"], o.name, frame)
                n += 1
            if row["group"] != "block":                 # ... and the batch is no larger than that takes
                assert any(o.body_bytes - 2 * (o.body_bytes // case["B"]) <= fu.SPAN + o.body_bytes // case["B"] for o in spans), row["id"]
            # odd maps, but where the op demands even sides (then its output map is odd)
            if row["id"] in ("dw48_k3s2_ragged", "reorg_ragged"):
                assert ops[0].out_h % 2 == 1 and ops[0].out_w % 2 == 1, row["id"]
            else:
                assert row["h"] % 2 == 1 and row["w"] % 2 == 1, row["id"]
    assert n >= 100


# ------------------------------------------------------------------------------------------------ refusals at 2^31 pixels

def _over_and_edge(row, dtype):
    fp = fu.frame_pixels(row, dtype)
    over = -(-(1 << 31) // fp)                       # the first batch with 2^31 pixels or more
    edge = fu.MAX_PIXELS // fp + 1                   # the first batch past the limit: less than one tile below 2^31 - 1 where frames are small
    ok = fu.MAX_PIXELS // fp
    return fp, over, edge, ok


def test_every_row_is_refused_from_2_31_pixels_on_and_without_room_for_a_tile():
    """Every family, the ones that hold pixel indices in 64 bits included: ONE check at plan creation for every op kind
    (csrc/api.hip check_size), so no row needs the audit table's "64-bit throughout" to pass here."""
    _no_gpu()
    for row in fu.big_cases() + [fu.case_by_id(s) for s in fu.BIG_BOUNDED.values()]:
        for dtype in row["dtypes"]:
            fp, over, edge, ok = _over_and_edge(row, dtype)
            for B in (over, edge):
                assert B * fp > fu.MAX_PIXELS and B < (1 << 31)
                names, err = _create(dict(row, B=B), dtype)
                assert names is None, (row["id"], dtype, B, names)
                assert "pixels" in err and "limit is %d" % fu.MAX_PIXELS in err and "block" in err, err
            if fp < fu.TILE_PIXELS:
                # small frames: the refused batch lies within one tile of 2^31 - 1 (the pixel count 2^31 - 1 itself is prime)
                assert (1 << 31) - 1 - fu.TILE_PIXELS < edge * fp <= (1 << 31) - 1 + fp
            if row["family"] in fu.BIG_BOUNDED or row["group"] == "block":
                continue                                 # (at such sizes other kernels have the op)
            # ... and the family's TRUE limit: the pixel limit, or grid x block of its launch (fu.launch_threads restates the
            # launchers) at 2^32 - 256 threads, whichever comes first; taken there, refused one frame later, by name
            ok, why = fu.largest_batch(row, dtype)
            names, err = _create(dict(row, B=ok), dtype)
            assert names is not None and names[0] == fu.family_name(row, dtype), (row["id"], dtype, ok, names, err)
            names, err = _create(dict(row, B=ok + 1), dtype)
            assert names is None and "block" in err, (row["id"], dtype, ok + 1, names)
            if why == "pixels":
                assert "pixels" in err and "limit is %d" % fu.MAX_PIXELS in err, err
            else:
                assert "threads" in err and "limit is %d" % fu.MAX_THREADS in err, err
                assert row["group"] == "spp" or fu.family_name(row, dtype) in err, err      # (the pyramid falls back to three pools first)


@pytest.mark.parametrize("kind", ["conv1x1", "conv3x3", "maxpool", "upsample", "add", "copy", "yolo"])
def test_2_31_minus_1_pixels_literally(kind):
    """a 1 x 1 map at batch 2^31 - 1: refused for its pixels (upsample just past a quarter of that: the OUTPUT count decides); the
    layer kernels and the decode have more than two threads a pixel, so their launch limit comes first: taken there, refused one
    frame later"""
    _no_gpu()
    if kind.startswith("conv"):
        k = int(kind[4])
        row = dict(fu.case_by_id("igemm1_64_full"), k=k, pad=(k - 1) // 2, h=1, w=1)
    elif kind == "yolo":
        row = dict(fu.case_by_id("yolo_few_classes"), h=1, w=1)
    else:
        row = dict(fu.case_by_id({"maxpool": "maxpool_s1_k5_wide"}.get(kind, kind + "_wide")), h=1, w=1)
    per = 4 if kind == "upsample" else 1
    for B in ((1 << 31) - 1, fu.MAX_PIXELS // per + 1):
        names, err = _create(dict(row, B=B), "bf16")
        assert names is None and "pixels" in err and "limit is %d" % fu.MAX_PIXELS in err, (B, names, err)
        assert ("output pixels" in err) == (kind == "upsample" and B < fu.MAX_PIXELS), err
    ok, why = fu.largest_batch(row, "bf16")
    assert (why == "pixels") == kind.startswith("conv")       # (a 128-pixel tile of 256 threads: 2 threads a pixel, just inside)
    names, err = _create(dict(row, B=ok), "bf16")
    assert names is not None and names[0] == fu.family_name(row, "bf16"), (ok, names, err)
    names, err = _create(dict(row, B=ok + 1), "bf16")
    assert names is None and why in err, (names, err)
    assert why == "pixels" or ("limit is %d" % fu.MAX_THREADS in err and fu.family_name(row, "bf16") in err), err


def test_stride_2_conv_is_refused_by_its_input_pixels():
    """the kernels of a stride-2 conv index INPUT pixels, four per output pixel"""
    _no_gpu()
    row = fu.case_by_id("igemm1_128_ragged_s2_res")
    fp = row["h"] * row["w"]
    names, err = _create(dict(row, B=fu.MAX_PIXELS // fp + 1), "bf16")
    assert names is None and "input pixels" in err, (names, err)
    names, err = _create(dict(row, B=fu.MAX_PIXELS // fp), "bf16")
    assert names == ["conv_igemm_bf16_128x128"], (names, err)


# ------------------------------------------------------------------------------------------------ bounded families

def _largest_accepted(row, dtype):
    """(largest batch at which the row's chooser names the family, batches tried): every batch up to four times the last
    accepted one, then every power of two and its neighbours up to the pixel limit"""
    want = fu.family_name(row, dtype)
    fp = fu.frame_pixels(row, dtype)
    last, B, tried = 0, 1, 0
    while B <= max(64, 4 * last):
        names, _ = _create(dict(row, B=B), dtype)
        tried += 1
        if names and names[0] == want:
            last = B
        B += 1
    e = 1
    while (1 << e) * fp <= fu.MAX_PIXELS:
        for b in ((1 << e) - 1, 1 << e, (1 << e) + 1, 3 << (e - 1)):
            if b > 4 * last:
                names, _ = _create(dict(row, B=b), dtype)
                tried += 1
                assert not (names and names[0] == want), (row["id"], dtype, b)
        e += 1
    return last, tried


@pytest.mark.parametrize("family", sorted(fu.BIG_BOUNDED))
def test_bounded_families_stay_below_2_gib(family):
    """The families without a GPU row.  conv1x1_dw: dw1x1_bm takes at most one tile per CU, 96 pixels x 256 CUs, asserted as that.
    The 192-pixel strip tile: halo_tile_fragments compares rounds x time per tile, which has no closed form in the batch, so this
    is a SEARCH on the family's ragged row, not a proof -- every batch up to four times the last accepted one, then every power
    of two and its neighbours up to the pixel limit -- and a tripwire for a change of the rule.  The largest operand either
    search finds is below 2^31 bytes by three orders of magnitude."""
    _no_gpu()
    row = fu.case_by_id(fu.BIG_BOUNDED[family])
    for dtype in row["dtypes"]:
        assert fu.chosen(row, dtype, "strided")[0][0] == fu.family_name(row, dtype)
        last, tried = _largest_accepted(row, dtype)
        assert last >= row["B"] and tried > 100, (family, dtype, last, tried)
        _, lay = fu.chosen(dict(row, B=last), dtype, "strided")
        largest = max(o.body_bytes for o in lay.operands)
        assert largest < (1 << 31), (family, dtype, last, largest)
        # the bound is one on PIXELS (one round of 96-pixel tiles; about ten rounds of strip tiles): under 2700 frames of 19 x 13,
        # which at 1024 channels of 16 bits -- the deepest layers of the shipped networks -- is 1.37e9 bytes, still below 2^31
        assert last * row["h"] * row["w"] <= 2700 * 19 * 13, (family, dtype, last)
        assert 2700 * 19 * 13 * 1024 * 2 < (1 << 31)
        if family.startswith("conv1x1_dw"):                 # the rule itself: one round of tiles on the 256 CUs of a dry run
            bm = int(family.rsplit("_", 1)[1].split("x")[0])
            assert (last * row["h"] * row["w"] + bm - 1) // bm * (row["cout"] // 256) <= 256, (family, last)


# ------------------------------------------------------------------------------------------------ the fused groups

def test_fused_block_takes_the_row_below_4_gib_and_diverts_one_frame_later():
    _no_gpu()
    row = fu.big_row("block_ragged_res")
    case = fu.big_case(row, "bf16")
    names, lay = fu.chosen(case, "bf16", "strided")
    assert names == ["conv_block_fused_bf16_x128", MARKER], names
    x, z = lay["input"], lay["output"]
    assert x.ld == z.ld and x.body_bytes == z.body_bytes < fu.SPAN <= x.body_bytes + x.body_bytes // case["B"]
    names, err = _create(dict(case, B=case["B"] + 1), "bf16")
    assert names is not None, err
    assert not names[0].startswith("conv_block_fused") and MARKER not in names and len(names) == 2, names   # two launches


def test_fused_stem_and_residual_block_divert_where_a_row_outgrows_their_lane_offsets():
    """conv_fused.hip: each lane keeps a 32-bit offset from its tile's 64-bit base: up to 35 rows of W x 3 bytes of frames
    (stem pair; int), up to 18 rows of W pixels of x (residual block; uint32_t).  Wider maps run unfused."""
    _no_gpu()
    stem = fu.case_by_id("stem_s2_ragged")
    w = ((1 << 31) // (35 * 3) | 1) + 2                      # 35 x w x 3 >= 2^31
    assert 35 * w * 3 >= (1 << 31) > 35 * (w - 2) * 3
    for ww, fused in ((w - 2, True), (w, False)):
        names, err = _create(dict(stem, B=1, h=3, w=ww), "bf16")
        assert names is not None, err
        assert (names == ["conv_stem_s2_fused_u8_bf16", MARKER]) == fused, (ww, names)
    res = fu.case_by_id("resblock_ragged")
    _, lay = fu.chosen(res, "bf16", "strided")
    ld = max(lay["input"].ld, lay["output"].ld)
    w = ((1 << 32) // (18 * ld * 2) | 1) + 2
    assert 18 * w * ld * 2 >= (1 << 32) > 18 * (w - 2) * ld * 2
    for ww, fused in ((w - 2, True), (w, False)):
        names, err = _create(dict(res, B=1, h=3, w=ww), "bf16")
        assert names is not None, err
        assert (names == ["conv_resblock_fused_bf16_64_32_64", MARKER]) == fused, (ww, names)


# ------------------------------------------------------------------------------------------------ one thread per element

def test_one_thread_per_element_kernels_are_refused_past_2_32_threads():
    """conv_direct, the layer kernels and reorg launch (unsigned)((total + 255) / 256) workgroups of 256 threads, and a launch
    holds fewer than 2^32 threads: a larger total is refused, by kernel name, well below the pixel limit"""
    _no_gpu()
    for cid, per_frame in (("direct_odd_cin_res", 13 * 11 * 24), ("copy_elem", 19 * 13 * 13), ("add_elem", 19 * 13 * 13),
                           ("upsample_elem", 26 * 22 * 13), ("maxpool_s1_elem", 13 * 11 * 13), ("reorg_ragged", 7 * 5 * 48)):
        row = fu.case_by_id(cid)
        ok = fu.MAX_THREADS // per_frame
        assert (ok + 1) * fu.frame_pixels(row, "bf16") < fu.MAX_PIXELS // 4
        names, err = _create(dict(row, B=ok), "bf16")
        assert names is not None and names[0] == fu.family_name(row, "bf16"), (cid, err)
        names, err = _create(dict(row, B=ok + 1), "bf16")
        assert names is None and fu.family_name(row, "bf16") in err and "limit is %d" % fu.MAX_THREADS in err, (cid, names, err)
        assert (ok, "threads") == fu.largest_batch(row, "bf16"), cid
    # the wide form moves 16 bytes per thread: the same batch of 64 channels is eight times fewer threads, and is taken
    row = fu.case_by_id("copy_wide")
    B = fu.MAX_THREADS // (19 * 13 * 13) + 1
    assert _create(dict(row, B=B), "bf16")[0] == ["copy_bf16"]
    assert _create(dict(row, B=fu.MAX_THREADS // (19 * 13 * 8) + 1), "bf16")[0] is None


def test_spp_pyramid_falls_back_at_its_launch_limit():
    """one workgroup of 256 threads per frame and 32-byte channel group: past 2^32 - 256 threads it is no pyramid launch, and
    the three single pools run (8 channels per thread: fewer threads) until they reach the limit themselves"""
    _no_gpu()
    row = dict(fu.case_by_id("spp_full"), h=1, w=1)                            # 64 channels of 16 bits: four groups a frame
    ok = fu.MAX_THREADS // (4 * 256)
    assert (ok, "threads") == fu.largest_batch(row, "bf16")
    assert _create(dict(row, B=ok), "bf16")[0] == ["maxpool_spp_pyramid_bf16", MARKER, MARKER]
    assert _create(dict(row, B=ok + 1), "bf16")[0] == ["maxpool_bf16"] * 3
    assert _create(dict(row, B=fu.MAX_THREADS // 8), "bf16")[0] == ["maxpool_bf16"] * 3
    names, err = _create(dict(row, B=fu.MAX_THREADS // 8 + 1), "bf16")
    assert names is None and "maxpool_bf16" in err and "threads" in err, (names, err)


# ------------------------------------------------------------------------------------------------ the checker, on the CPU

def _synthetic():
    """an "output" of 7 frames x 5 pixels x 8 bf16 channels at stride 24 behind a pad, as the GPU test lays it out"""
    pad = fu.Operand("pad", "pad", "u8", 1, 4096, [(0, 4096)], tile_elems=1)
    x = fu.Operand("input", "in", "bf16", 35, 16, [(4, 8)])
    o = fu.Operand("output", "out", "bf16", 35, 24, [(8, 8)])
    lay = fu.Layout([pad, x, o])
    alloc = torch.empty(lay.total, dtype=torch.uint8)
    base = (torch.arange(3 * 5 * 8, dtype=torch.float32).reshape(3, 40) + 1).to(torch.bfloat16)
    frames = base[torch.arange(7) % 3].reshape(35, 8)
    fu.fill(alloc, lay, {"input": [frames]}, poisoned=True)
    before = alloc.clone()
    body = alloc[o.body:o.body + o.body_bytes].view(35, 48)
    body[:, 16:32] = frames.view(torch.uint8).reshape(35, 16)              # the "kernel": writes its slice, nothing else
    return lay, o, before, alloc, base


def _check(lay, o, before, after, base):
    msg = fu.region_violations(before, after, lay, chunk=1000)
    if msg:
        return msg
    t = fu.read_slice(after, o, 0, torch.uint8)
    return (fu.nan_violations(t, 7, o.fmt, chunk=100) or fu.frame_violations(t, 7, chunk=200)
            or fu.frame_violations(t, 7, base.view(torch.uint8).reshape(3, -1), chunk=200))


def test_checker_passes_a_clean_tensor():
    lay, o, before, after, base = _synthetic()
    assert int((before[:lay["pad"].end] != 0).all()) == 1                    # the pad holds the byte pattern
    assert _check(lay, o, before, after, base) is None


def test_checker_reports_a_frame_shifted_by_a_fraction_of_a_frame():
    lay, o, before, after, base = _synthetic()
    t = fu.read_slice(after, o, 0, torch.uint8).reshape(7, -1)
    flat = t.reshape(-1)
    shifted = flat[4 * 80 - 2 * 16:5 * 80 - 2 * 16].clone()                  # frame 4, read two pixels early: a wrapped address
    body = after[o.body:o.body + o.body_bytes].view(35, 48)
    body[20:25, 16:32] = shifted.reshape(5, 16)
    msg = _check(lay, o, before, after, base)
    assert msg and msg.startswith("frame 4 differs from frame 1 (4 % 3)") and "1 frames of" in msg, msg


def test_checker_reports_a_frame_left_at_its_prefill():
    lay, o, before, after, base = _synthetic()
    body = after[o.body:o.body + o.body_bytes].view(35, 48)
    body[30:35, 16:32] = before[o.body:o.body + o.body_bytes].view(35, 48)[30:35, 16:32]
    msg = _check(lay, o, before, after, base)
    assert msg == "frame 6 holds NaN: 40 of its 40 elements never written or poisoned", msg
    # one element of one frame is enough
    lay, o, before, after, base = _synthetic()
    after[o.body + 17 * 48 + 16:o.body + 17 * 48 + 18] = torch.tensor(fu.NAN_BYTES["bf16"], dtype=torch.uint8)
    assert _check(lay, o, before, after, base).startswith("frame 3 holds NaN: 1 of its 40"), _check(lay, o, before, after, base)


def test_checker_reports_a_changed_byte_in_the_pad_a_margin_and_an_input():
    lay, o, before, after, base = _synthetic()
    after[lay["pad"].body + 1234] ^= 0xFF
    msg = _check(lay, o, before, after, base)
    assert msg and "operand 'pad' (pad): slice 0 changed" in msg and "1 in all" in msg, msg
    lay, o, before, after, base = _synthetic()
    after[7] ^= 1                                                          # the very front of the allocation
    assert "operand 'pad' (pad): front guard changed" in _check(lay, o, before, after, base)
    lay, o, before, after, base = _synthetic()
    after[o.body + 33 * 48 + 40] ^= 1
    msg = _check(lay, o, before, after, base)
    assert "operand 'output' (out): right margin changed, first at pixel 33 channel 20" in msg, msg
    lay, o, before, after, base = _synthetic()
    x = lay["input"]
    after[x.body + 9 * 32 + 8] ^= 1
    msg = _check(lay, o, before, after, base)
    assert "operand 'input' (in): slice 0 changed, first at pixel 9 channel 0" in msg, msg
