"""The footprint case table and harness arithmetic (tests/footprint_util.py), without a GPU: every case's strided ops go to the
chooser with fake addresses (``y3_plan_create_ex`` only decides, as in tests/kernel_choice_util.py) and get the family the
case claims; the table reaches every kernel name of tests/golden/kernel_choice.json; guards, margins and alignment of every
layout meet the conditions a GPU run of the cases relies on."""
import ctypes
import json

import pytest
import torch

import footprint_util as fu
from kernel_choice_util import FIXTURE

MARKER = "(fused into the previous op)"


def _fixture_families():
    with open(FIXTURE) as f:
        names = {r[0] for r in json.load(f)["rows"]}
    names.discard(MARKER)
    return names


def _no_gpu():
    if torch.cuda.is_available():
        pytest.skip("fake device addresses must never reach a library that can see a GPU")


@pytest.mark.parametrize("mode", ["dense", "strided"])
def test_every_case_gets_the_family_it_claims(mode):
    _no_gpu()
    wrong = []
    for case in fu.cases():
        for dtype in case["dtypes"]:
            names, _ = fu.chosen(case, dtype, mode)
            if names[0] != fu.family_name(case, dtype) or any(n != MARKER for n in names[1:]):
                wrong.append((case["id"], dtype, fu.family_name(case, dtype), names))
    assert not wrong, wrong


def test_table_reaches_every_family_of_the_kernel_choice_fixture():
    """Exact names (dtype included): what the table reaches == the fixture's kernel names + the kernels no shipped cfg's plan
    under the fixture's option sets holds (add, copy, maxpool_dk, maxpool_spp_pyramid_dk, conv_direct, the two reorg forms,
    the VALU stem with 16-bit stores).  No skip list: removing a row of the table that is a family's only one fails here."""
    reached = {fu.family_name(c, d) for c in fu.cases() for d in c["dtypes"]}
    fixture = _fixture_families()
    extra = {f % t if "%s" in f else f for f in fu.NOT_IN_FIXTURE for t in ("f32", "bf16", "f16")}
    assert not (extra & fixture), "a kernel listed as absent from the fixture is in it: %s" % sorted(extra & fixture)
    assert fixture - reached == set(), "families without a footprint case: %s" % sorted(fixture - reached)
    assert reached - fixture == extra, "cases for kernels neither in the fixture nor declared: %s" % sorted(reached - fixture - extra)


def test_every_family_has_a_full_and_a_ragged_case_and_both_shortcut_forms():
    by_family = {}
    for c in fu.cases():
        by_family.setdefault(c["family"], []).append(c)
    for fam, cs in by_family.items():
        assert len(cs) >= 2, fam
        if all(c["group"] == "conv" for c in cs) and any(c["res"] for c in cs):
            assert any(not c["res"] for c in cs), fam + ": no case without the shortcut operand"
    # the conv families that take a shortcut operand (their choosers accept Y3_F_RESIDUAL) have a case with one
    for fam in ("conv_igemm_%s_128x128", "conv_igemm2_%s_128x128", "conv_igemm2_%s_96x64", "conv_igemm3_%s_128x128",
                "conv_igemm3_%s_64x128", "conv_halo_ws_%s_192x128", "conv_halo_ws_%s_256x128", "conv_halo_dw_%s_192x256",
                "conv_patch_wsp_%s_8x32x128", "conv_dw48_k1_%s", "conv_dw48_k3_%s", "conv_block_fused_%s_x128", "conv_direct_%s"):
        assert any(c.get("res") for c in by_family[fam]), fam
    # shapes stay at or below 16 x 76 x 76 x 512 ...
    for c in fu.cases():
        # (a row on a map of one pixel a side has a batch of its own, 37 or 5 -- conv1x1_dw: what fills one round of workgroups --,
        # and stays below 16 x 76 x 76 PIXELS all the same)
        assert c["B"] <= 16 or (c.get("tiny") and min(c["h"], c["w"]) <= 3 and c["B"] * c["h"] * c["w"] <= 16 * 76 * 76), c["id"]
        assert c["h"] * c["w"] <= 76 * 76 and max(c.get("cout", 0), c.get("c", 0)) <= 512, c["id"]
        # ... but for the input channels of a row that is there for ONE compiled K depth of a direct-weights kernel, which are
        # then exactly what that instance dictates: 64 x nkt per halo image (the stride-2 kernel's two-image form: twice that),
        # on the smallest grid its chooser takes: at most half the elements of a tensor at the limit
        if c.get("cin", 0) > 512:
            assert c.get("nkt") in (12, 16) and c["cin"] == 64 * c["nkt"] and c["h"] * c["w"] <= 38 * 38, c["id"]
            assert c["B"] * c["h"] * c["w"] * c["cin"] <= 16 * 76 * 76 * 512 // 2, c["id"]
        if "nkt" in c:
            assert c["cin"] in (64 * c["nkt"], 128 * c["nkt"]) and (c["cin"] == 64 * c["nkt"] or "two_images" in c["id"]), c["id"]
        # only the patch kernel's maps are wider than 76 (its chooser asks rows of more than 128 px), and the one row of the
        # stride-2 kernel's two-image form at 256 channels (conv_dw48.hip dw48_shape: one image of all channels must outgrow LDS)
        assert max(c["h"], c["w"]) <= 76 or c["family"].startswith("conv_patch_wsp") or c.get("wide_map"), c["id"]
    assert [c["id"] for c in fu.cases() if c.get("wide_map")] == ["dw48_k3s2_c256_two_images"]


def test_tiny_rows_cover_every_family_or_a_declined_entry():
    """every family of the table has a "dot", a "row" and a "column" row (footprint_util.tiny_cases), or an entry in
    TINY_DECLINED -- and then plan creation, under the option set that forces the family on its other rows, gives each of the
    three shapes to the kernels the entry names"""
    _no_gpu()
    H = fu._H()
    lib = H.lib()
    tags = [t for t, _, _, _ in fu.TINY_SHAPES]
    by_family = {}
    for c in fu.cases():
        by_family.setdefault(c["family"], []).append(c.get("tiny"))
    for fam, have in by_family.items():
        if fam in fu.TINY_DECLINED:
            assert not any(have), fam + ": rows AND a declined entry"
            continue
        for t in tags:
            assert t in have, "%s has no %r row" % (fam, t)
    # output maps of the rows are what their names say
    for c in fu.tiny_cases():
        for dtype in c["dtypes"]:
            ops, _, _, _ = fu.build(c, dtype, "dense", H.options(**fu._opts()[c["opt"]]))
            last = ops[len(ops) - 1]
            out = (last.out_h, last.out_w) if last.kind != H.OP_YOLO else (last.in_h, last.in_w)
            if c["group"] == "layer" and c["kind"] == "upsample":
                out = (last.in_h, last.in_w)                  # (named by its input: 1 x 1 to 2 x 2)
            want = {t: (h, w) for t, _, h, w in fu.TINY_SHAPES}[c["tiny"]]
            assert out == want, (c["id"], out, want)
    for fam, (src, goes_to) in fu.TINY_DECLINED.items():
        for tag, B, h, w in fu.TINY_SHAPES:
            case = dict(fu.case_by_id(src), B=B, h=h, w=w)
            for dtype in case["dtypes"]:
                opt = H.options(**fu._opts()[case["opt"]])
                ops, lay, _, _ = fu.build(case, dtype, "strided", opt)
                for i in range(len(ops)):                     # (whatever reads fragment-order weights gets a fake copy: decide only)
                    if ops[i].kind == H.OP_CONV and not ops[i].d_weight_frag:
                        ops[i].d_weight_frag = (1 << 45) + (i << 32)
                handle = ctypes.c_void_p()
                H.check(lib.y3_plan_create_ex(ops, len(ops), lay["zero page"].ptr(1 << 44), ctypes.byref(opt), ctypes.byref(handle)))
                try:
                    names = tuple(lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops)))
                finally:
                    lib.y3_plan_destroy(handle)
                assert names == tuple(g % fu.TAG[dtype] for g in goes_to), (fam, tag, dtype, names)


def _kmode(case, dtype):
    """(K-tiling mode, whether the last K-tile is partial): csrc/conv_igemm.hip igemm_ktiles restated"""
    bke = 128 // fu.ES[dtype]                                   # elements of one K-tile
    mode = 0 if case["cin"] % bke == 0 else (2 if bke % case["cin"] == 0 else 1)
    return mode, (case["k"] ** 2 * case["cin"]) % bke != 0


def test_k_tilings_of_the_table():
    """every implicit-GEMM version runs every K-tiling in every element type: one tap per K-tile (0), per-chunk taps (1),
    several whole taps per K-tile (2); a 5x5 (25-bit tap mask); a last K-tile that K ends inside of"""
    for dtype in fu.ALL:
        for version in ("conv_igemm_%s_", "conv_igemm2_%s_", "conv_igemm3_%s_"):
            cs = [c for c in fu.cases() if c["group"] == "conv" and c["family"].startswith(version) and dtype in c["dtypes"]]
            modes = [_kmode(c, dtype) for c in cs]
            assert {m for m, _ in modes} == {0, 1, 2}, (dtype, version, sorted({m for m, _ in modes}))
            assert any(c["k"] == 5 for c in cs), (dtype, version, "no 5x5")
            assert any(partial for _, partial in modes), (dtype, version, "no partial last K-tile")
            # the modes that can end inside a K-tile each do so once
            assert {m for m, partial in modes if partial} == {1, 2}, (dtype, version)


def test_no_family_is_dense_only():
    """every chooser takes pixel strides (the strided half of test_every_case_gets_the_family_it_claims): 0 entries"""
    assert len(fu.DENSE_ONLY) == 0


def test_layout_guards_margins_and_alignment():
    _no_gpu()
    H = fu._H()
    n = 0
    for case in fu.cases():
        for dtype in case["dtypes"]:
            opt = H.options(**fu._opts()[case["opt"]])
            ops, lay, _, _ = fu.build(case, dtype, "strided", opt)
            prev_end = 0
            for o in lay.operands:
                assert o.front == prev_end and o.body % fu.ALIGN == 0, (case["id"], o.name)
                need = max(fu.GUARD_MIN, fu.TILE_PIXELS * (o.ld if o.pixels > 1 and case["group"] != "yolo" else o.tile_elems) * o.es)
                assert o.body - o.front >= need and o.end - (o.body + o.body_bytes) >= need, (case["id"], o.name)
                prev_end = o.end
                n += 1
            assert lay.total == prev_end
            acts = [o for o in lay.operands if o.pixels > 1 and o.side in ("in", "out", "inout") and o.fmt != "i64"
                    and not (case["group"] == "yolo" and o.name != "input")]
            assert acts, case["id"]
            for o in acts:
                if case["id"] == "yolo_ld256":
                    continue                     # 255 channels at stride 256: the head's own layout, right margin only
                assert o.slices[0][0] > 0 and o.slices[-1][0] + o.slices[-1][1] < o.ld, (case["id"], o.name)
            # different strides for input, output and residual
            lds = [o.ld for o in acts]
            assert len(set(lds)) == len(lds), (case["id"], lds)
            # c0 and ld: multiples of the chooser's unit, of nothing larger
            unit = 16 // fu.ES[dtype]
            for o in acts:
                if case["group"] == "layer":
                    continue                     # (test_layer_cases_take_the_form_they_claim)
                elif case["group"] in ("conv", "stem_pair", "resblock", "block", "head", "spp") and o.fmt == dtype:
                    # (the strip and patch kernels ask 8-element output strides in float32 too: conv_halo.hip, `out_ld % 8`)
                    u = (case.get("out_unit") or unit) if o.name in ("output", "residual") else unit
                    assert o.ld % u == 0 and o.slices[0][0] % u == 0 and o.ld % (2 * u) != 0, (case["id"], o.name, o.ld)
    assert n > 500


def test_violation_report_names_operand_region_pixel_and_channel():
    """the check helpers on a CPU tensor: a byte changed in a right margin, a guard and a read-only operand is named"""
    a = fu.Operand("input", "in", "bf16", 10, 24, [(8, 8)])
    b = fu.Operand("output", "out", "bf16", 10, 40, [(8, 16)])
    lay = fu.Layout([a, b])
    before = torch.zeros(lay.total, dtype=torch.uint8)
    after = before.clone()
    after[b.body:b.body + b.body_bytes].view(10, 80)[:, 16:48] = 1      # the slice itself: allowed
    assert fu.footprint_violations(before, after, lay) is None
    after[b.body + 3 * 80 + 48] = 1                                      # pixel 3, first channel right of the slice
    msg = fu.footprint_violations(before, after, lay)
    assert "operand 'output'" in msg and "right margin" in msg and "pixel 3 channel 24" in msg and "1 in all" in msg, msg
    after2 = before.clone()
    after2[b.body + b.body_bytes + 5] = 7
    assert "back guard" in fu.footprint_violations(before, after2, lay)
    after3 = before.clone()
    after3[a.body + 2 * 48 + 16] = 7
    msg = fu.footprint_violations(before, after3, lay)
    assert "operand 'input' (in)" in msg and "slice 0" in msg and "pixel 2 channel 0" in msg, msg


def test_fill_puts_nan_round_inputs_pattern_round_outputs_and_nan_in_output_slices():
    """``fill`` on a CPU tensor: the strided layout's poison is where the GPU test relies on it"""
    a = fu.Operand("input", "in", "bf16", 6, 24, [(8, 8)])
    b = fu.Operand("output", "out", "fp16", 6, 40, [(8, 16)])
    f = fu.Operand("scale", "in", "float32", 1, 16, [(0, 16)], tile_elems=1)
    lay = fu.Layout([a, b, f])
    x = torch.arange(48, dtype=torch.float32).reshape(6, 8).to(torch.bfloat16)
    s = torch.arange(16, dtype=torch.float32).reshape(1, 16)
    alloc = torch.empty(lay.total, dtype=torch.uint8)
    fu.fill(alloc, lay, {"input": [x], "scale": [s]}, poisoned=True)
    whole = alloc[a.front:a.end].view(torch.bfloat16)
    assert int(torch.isnan(whole.float()).sum()) == whole.numel() - 48            # NaN everywhere but the slice
    assert torch.equal(fu.read_slice(alloc, a, 0, torch.bfloat16), x)
    assert alloc[a.front:a.front + 2].tolist() == [0xC0, 0x7F]
    sc = alloc[f.front:f.end].view(torch.float32)
    assert int(torch.isnan(sc).sum()) == sc.numel() - 16 and torch.equal(fu.read_slice(alloc, f, 0, torch.float32), s)
    assert bool(torch.isnan(fu.read_slice(alloc, b, 0, torch.float16).float()).all())   # an element never written shows
    body = alloc[b.body:b.body + b.body_bytes].view(6, 80)
    off = b.body + 3 * 80 + 48
    assert int(body[3, 48]) == off % fu.PATTERN_PERIOD + 1 and int(alloc[b.front]) == b.front % fu.PATTERN_PERIOD + 1
    assert int((alloc[b.front:b.body] == 0).sum()) == 0
    # the dense run: zero guards, data in place
    fu.fill(alloc, lay, {"input": [x], "scale": [s]}, poisoned=False)
    assert int(alloc[a.front:a.body].sum()) == 0 and int(alloc[b.front:b.body].sum()) == 0
    assert torch.equal(fu.read_slice(alloc, a, 0, torch.bfloat16), x)


def test_layer_cases_take_the_form_they_claim():
    """The wide and the element-wise form of a layer kernel carry one name; which one runs is decided at launch
    (layers.hip launch_layer): wide iff in_c, in_ld, out_ld (add: res_ld too) are multiples of the 16-byte vector and d_in,
    d_out (add: d_res) are 16-byte aligned.  The "wide" cases meet that in both layouts, the "elem" cases break it."""
    _no_gpu()
    H = fu._H()
    n = {True: 0, False: 0}
    for case in fu.cases():
        if case["group"] != "layer":
            continue
        for dtype in case["dtypes"]:
            vec = 16 // fu.ES[dtype]
            for mode in ("dense", "strided"):
                ops, _, _, _ = fu.build(case, dtype, mode, H.options())
                op = ops[0]
                wide = op.in_c % vec == 0 and op.in_ld % vec == 0 and op.out_ld % vec == 0 and op.d_in % 16 == 0 and op.d_out % 16 == 0
                if case["kind"] == "add":
                    wide = wide and op.res_ld % vec == 0 and op.d_res % 16 == 0
                assert wide == case["wide"], (case["id"], dtype, mode, op.in_c, op.in_ld, op.out_ld, op.res_ld)
                if not wide and mode == "strided":           # the strides themselves, not only the channel count, are odd
                    assert op.in_ld % vec != 0 and op.out_ld % vec != 0, (case["id"], dtype, op.in_ld, op.out_ld)
                n[wide] += 1
    assert n[True] >= 50 and n[False] >= 50, n
