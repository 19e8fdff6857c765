"""CPU-side checks of the direct-weights fused block kernel (csrc/conv_block_dw.hip; y3_options.fuse_block = 3 / 4): the
shared library it lives in -- its two instances, their register budget, the keys of its census
(tests/golden/kernel_instances_block.json; the checks every library gets are tests/test_code_object.py's) -- and where plans
name it, through the fake-address route of
tests/kernel_choice_util.py.  That every configuration of tests/golden/kernel_choice.json still reproduces, and that the main
library's census is what it was, is tests/test_kernel_choice.py's and tests/test_code_object.py's to say: they run unchanged."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_dw_cases as BDC  # noqa: E402
import block_dw_util as BU  # noqa: E402
import code_object  # noqa: E402
import footprint_util as fu  # noqa: E402
import kernel_census as census  # noqa: E402

NAME = {"bf16": "conv_block_dw_bf16_x128", "fp16": "conv_block_dw_f16_x128"}


@pytest.fixture(scope="module")
def kernels():
    return census.kernels("block")          # (asserts: built, device code for gfx950 only)


def test_block_library_budgets(kernels):
    """two instances, at most 256 VGPRs each and workgroups of 512 (the launch's dynamic LDS size is a plan's to say, below); no
    scratch, no spills, VGPR + AGPR, static LDS and wave64 are tests/test_code_object.py's, for every library"""
    assert len(kernels) == 2, [k[".name"] for k in kernels]
    for k in kernels:
        name = k[".name"]
        assert "conv_block_dw_kernel" in name, name
        assert k[".vgpr_count"] <= 256, name
        assert k[".max_flat_workgroup_size"] == 512, name


def test_block_library_census():
    """every case of tests/test_gpu_block_dw.py and of the kernel-level suites has its entry, of one symbol of its storage type
    (the rules -- every compiled kernel launched by a recorded case and by a contention case, no recorded symbol the library
    lacks -- are tests/test_code_object.py's, for every library)"""
    fixture = census.load("block")
    assert set(fixture) == {"footprint", "contention"}
    for table in fixture.values():
        for key, syms in table.items():
            assert syms == sorted(set(syms)) and len(syms) == 1, key
            assert ("IDF16bE" in syms[0]) == key.endswith("-bf16") and ("IDF16_E" in syms[0]) == key.endswith("-fp16"), (key, syms)
    want = {BU.case_key(*c) for c in BU.CASES} | {"block_dw_oracle-bf16"}
    # ... and every run of the kernel-level suites (tests/block_dw_cases.py): the footprint trio and the three exact-sum plants on
    # every row in both types, the epilogue pins in both types, the row below 2^32 bytes
    want |= {BDC.footprint_key(c, d) for c, d in BDC.case_ids()} | {BDC.exact_key(c, d, k) for c, d in BDC.case_ids() for k in BDC.PLANTS}
    want |= {BDC.epilogue_key(d) for d in BDC.DTYPES} | {BDC.big_key("bf16")}
    assert set(fixture["footprint"]) == want, sorted(set(fixture["footprint"]) ^ want)
    assert set(fixture["contention"]) == {"block_dw_res-bf16", "block_dw_nores-bf16", "block_dw_res-fp16"}


def suite_keys(suite, dtype=None):
    """the census keys under which ``suite`` (block_dw_cases.SUITES; "exact": a dict per plant) records its runs"""
    ids = [(c, d) for c, d in BDC.case_ids() if dtype in (None, d)]
    if suite == "footprint":
        return {BDC.footprint_key(c, d) for c, d in ids}
    if suite == "epilogue":
        return {BDC.epilogue_key(d) for d in BDC.DTYPES if dtype in (None, d)}
    return {k: {BDC.exact_key(c, d, k) for c, d in ids} for k in BDC.PLANTS}


def instances_without(fixture, library):
    """[(symbol, suite)] for every compiled instance that no recorded run of a suite launches: the footprint trio, the epilogue
    pins, each of the three exact-sum plants"""
    table = fixture["footprint"]
    sets = {"footprint": suite_keys("footprint"), "epilogue": suite_keys("epilogue")}
    sets.update({"exact " + k: v for k, v in suite_keys("exact").items()})
    return [(sym, suite) for sym in sorted(library) for suite, keys in sorted(sets.items())
            if not any(sym in table.get(k, ()) for k in keys)]


def test_every_compiled_instance_is_held_by_every_suite(kernels):
    """no skip list: an instance compiled later -- another storage type, another x-buffer count -- fails here until a row of the
    footprint trio, an epilogue pin and each exact-sum plant launch it (tests/test_grouped_host.py
    test_every_compiled_instance_has_an_epilogue_form_and_a_big_row is the model)"""
    fixture = census.load("block")
    library = {k[".name"] for k in kernels}
    assert instances_without(fixture, library) == []
    # the check sees a missing suite: without the epilogue keys both instances lack it, and an unknown symbol lacks all five
    cut = {"footprint": {k: v for k, v in fixture["footprint"].items() if k not in suite_keys("epilogue")}}
    assert instances_without(cut, library) == [(s, "epilogue") for s in sorted(library)]
    assert len(instances_without(fixture, {"_Z20conv_block_dw_kernelIfEv11BlockDwArgs"})) == 5
    # ... and the row below 2^32 bytes runs the bf16 instance (fp16 shares its address code)
    assert "IDF16bE" in fixture["footprint"][BDC.big_key("bf16")][0]


def test_main_library_names_the_block_library_as_a_dependency():
    with open(code_object.LIB, "rb") as f:
        data = f.read()
    assert b"libyolov3_hip_block.so" in data and b"$ORIGIN" in data
    assert b"conv_block_dw_kernel" not in data              # its device code is not in the main library


def _no_gpu():
    if torch.cuda.is_available():
        pytest.skip("fake device addresses must never reach a library that can see a GPU")


def _overlap(a, b):
    """whether z, the output of op b, overlaps x, the input of op a (conv_block.hip: such a pair must not run fused)"""
    x0, xb = a.d_in, a.batch * a.in_h * a.in_w * a.in_ld * 2
    z0, zb = b.d_out, b.batch * b.out_h * b.out_w * b.out_ld * 2
    return x0 < z0 + zb and z0 < x0 + xb


def _plan(dtype, batch, overrides, strip=()):
    """(ops, kernel name per op) of yolov3 608 on fake addresses; ``strip``: op indices that lose their d_weight_frag"""
    import kernel_choice_util as K
    from yolov3 import _hip
    lib = _hip.lib()
    opt = _hip.options(**overrides)
    ops, frag, fake = K.build_ops("yolov3", 608, dtype, batch, "u8", opt)
    for i in strip:
        ops[i].d_weight_frag = None
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
        dims = [_hip.plan_op_dims(handle, i) for i in range(len(ops))]
    finally:
        lib.y3_plan_destroy(handle)
    return ops, names, frag, dims


def _pairs(ops):
    """indices i of the 1x1 -> 3x3 pairs of the plan that the block kernels support by shape"""
    from yolov3 import _hip
    out = []
    for i in range(len(ops) - 1):
        a, b = ops[i], ops[i + 1]
        if a.kind != _hip.OP_CONV or b.kind != _hip.OP_CONV or not a.flags & _hip.F_FUSE_NEXT:
            continue
        if a.ksize == 1 and a.out_c == 128 and a.in_c >= 192 and b.ksize == 3 and b.stride == 1 and b.in_c == 128 and b.d_in == a.d_out:
            out.append(i)
    return out


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_fuse_block_3_names_the_kernel_on_the_76x76_pairs_and_nowhere_else(dtype):
    from yolov3 import _hip
    _no_gpu()
    ops, names, frag, dims = _plan(dtype, 16, {"fuse_block": 3})
    _, plain, frag0, _ = _plan(dtype, 16, {})
    pairs = _pairs(ops)
    residual = [i for i in pairs if ops[i + 1].flags & _hip.F_RESIDUAL]
    branch = [i for i in pairs if i not in residual]
    assert len(residual) == 8 and branch, (residual, branch)
    for i in pairs:
        assert (ops[i].in_h, ops[i].in_w) == (76, 76) and ops[i].d_weight_frag and ops[i + 1].d_weight_frag, i
        assert frag[i] == ops[i].cout_pad * ops[i].k_ld * 2 and frag[i + 1] == ops[i + 1].cout_pad * ops[i + 1].k_ld * 2, i
    # the eight residual pairs: z is a buffer of its own (x is read again as the shortcut operand), all fused
    for i in residual:
        assert not _overlap(ops[i], ops[i + 1]), i
        assert names[i] == NAME[dtype] and names[i + 1] == "(fused into the previous op)", (i, names[i], names[i + 1])
        assert dims[i] == (256, 512, BU_LDS), (i, dims[i])
    # the branch pairs have no shortcut: the arena may give z the bytes of x, and those pairs run as two launches
    for i in branch:
        fused = names[i] == NAME[dtype]
        assert fused == (not _overlap(ops[i], ops[i + 1])), (i, names[i], "z overlaps x" if _overlap(ops[i], ops[i + 1]) else "z apart from x")
        if not fused:
            assert names[i] == plain[i] and names[i + 1] == plain[i + 1], i
    taken = {j for i in pairs if names[i] == NAME[dtype] for j in (i, i + 1)}
    for j in range(len(ops)):
        if j not in taken:
            assert names[j] == plain[j] and "block_dw" not in names[j], (j, names[j], plain[j])
            if j not in pairs and j - 1 not in pairs:
                assert frag[j] == frag0[j], (j, frag[j], frag0[j])


BU_LDS = 4 * 448 * 64          # the launch: four 28-KiB x buffers (conv_block_dw.hip kNB), which the mid image then fills


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("batch", [1, 8])
def test_fuse_block_3_names_it_nowhere_below_the_70_percent_rule(dtype, batch):
    """one and eight frames: 16 and 128 rectangles on 256 CUs (eff < 0.7), and nobody is asked for a fragment-order copy"""
    _no_gpu()
    _, names, frag, _ = _plan(dtype, batch, {"fuse_block": 3})
    _, plain, frag0, _ = _plan(dtype, batch, {})
    assert names == plain and frag == frag0


def test_a_pair_without_a_fragment_copy_is_two_launches():
    _no_gpu()
    ops, names, _, _ = _plan("bf16", 16, {"fuse_block": 3})
    _, plain, _, _ = _plan("bf16", 16, {})
    first = _pairs(ops)[0]
    assert names[first] == NAME["bf16"]
    for strip in (first, first + 1):
        _, got, _, _ = _plan("bf16", 16, {"fuse_block": 3}, strip=(strip,))
        assert got[first] == plain[first] and got[first + 1] == plain[first + 1], (strip, got[first], got[first + 1])
        assert got[first + 2] == NAME["bf16"]           # the next pair is untouched


def test_float32_and_the_other_modes_never_name_it():
    _no_gpu()
    _, names, _, _ = _plan("float32", 16, {"fuse_block": 3})
    assert not any("block_dw" in n for n in names)
    for mode in (0, 1, 2):
        _, names, _, _ = _plan("bf16", 16, {"fuse_block": mode})
        assert not any("block_dw" in n for n in names), mode


# ------------------------------------------------------------------------------------------------ the case table

def _row_plan(case, dtype, mode, **over):
    """(kernel names, launch dims per op) of a row of tests/block_dw_cases.py on fake addresses; every conv gets a fake
    fragment-order copy where the layout holds none (a declined pair's two launches may read one: creation only decides)"""
    from yolov3 import _hip
    lib = _hip.lib()
    case = dict(case, **over)
    opt = _hip.options(**fu._opts()[case["opt"]])
    ops, lay, frag, _ = fu.build(case, dtype, mode, opt)
    for i in range(len(ops)):
        if not ops[i].d_weight_frag:
            ops[i].d_weight_frag = (1 << 45) + (i << 32)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), lay["zero page"].ptr(1 << 44), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        return ([lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))],
                [_hip.plan_op_dims(handle, i) for i in range(len(ops))], lay, frag, ops)
    finally:
        lib.y3_plan_destroy(handle)


MARKER = "(fused into the previous op)"


@pytest.mark.parametrize("cid", ["%s-%s" % p for p in BDC.case_ids()])
def test_every_row_gets_the_family_it_claims_and_the_grid_of_its_rectangles(cid):
    _no_gpu()
    cname, dtype = cid.rsplit("-", 1)
    case = BDC.case_by_id(cname)
    assert case["family"] == BDC.FAMILY and case["opt"] == BDC.OPT and case["group"] == "block"
    for mode in ("dense", "strided"):
        names, dims, lay, frag, ops = _row_plan(case, dtype, mode)
        assert names == [NAME[dtype], MARKER], (cid, mode, names)
        # both convs' fragment-order copies are operands of the layout, of the size the library asks for
        assert frag == {0: "op0 fragment weights", 1: "op1 fragment weights"}, frag
        for i in (0, 1):
            assert lay[frag[i]].body_bytes == ops[i].cout_pad * ops[i].k_ld * 2 and ops[i].d_weight_frag == lay[frag[i]].ptr(1 << 44)
        tw, th = fu.block_tile(case["h"], case["w"])
        tiles_x, tiles_y = -(-case["w"] // tw), -(-case["h"] // th)
        assert dims[0] == (tiles_x * tiles_y * case["B"], 512, BU_LDS) and dims[0][0] == BDC.grid(case), (cid, dims[0])
        x, z = lay["input"], lay["output"]
        if mode == "strided":
            assert x.slices[0][0] > 0 and z.slices[0][0] > 0 and x.ld != z.ld, (x.ld, z.ld)
            assert ops[1].res_ld == (x.ld if case["res"] else 0) and ops[0].in_ld == x.ld and ops[1].out_ld == z.ld
        else:
            assert (x.ld, z.ld) == (case["cin"], case["cout"])


def test_the_table_holds_what_its_rows_are_for():
    """the rows of cases() as they are; rectangles over both frame edges; three passes with the shortcut; ten sub-steps; more than
    one round of workgroups on 256 CUs; grids above 8 that are no multiple of 8"""
    rows = {c["id"]: c for c in BDC.cases()}
    assert len(rows) == len(BDC.cases()) == 10
    for src in BDC.FROM_CASES:
        mine, theirs = rows[src.replace("block_", "block_dw_", 1)], fu.case_by_id(src)
        assert theirs["family"] == "conv_block_fused_%s_x128"
        for key in ("B", "h", "w", "cin", "cout", "res", "dtypes", "group"):
            assert mine[key] == theirs[key], (src, key)
    c = rows["block_dw_25x43_res"]
    tw, th = fu.block_tile(c["h"], c["w"])
    assert (tw, th) == BU.RECTANGLES["25x43"][:2] and tw * 2 > c["w"] > tw and th * 2 > c["h"] > th
    c = rows["block_dw_19x19_c384_res"]
    assert c["res"] and c["cin"] == c["cout"] == 384 and c["cout"] // 128 == 3
    c = rows["block_dw_19x19_c320"]
    assert c["cin"] // 32 == 10 and 10 % 4 != 0 and c["cout"] == 128 and not c["res"]
    assert BDC.grid(rows["block_dw_19x19_b300"]) == 300 > 256 and 300 % 8 != 0
    assert BDC.grid(rows["block_dw_38x38_b5"]) == 20 and 20 % 8 != 0
    c = rows["block_dw_smallest"]
    assert BDC.grid(c) == c["B"] == 37 and c["h"] * c["w"] == 32            # two of a workgroup's 24 pixel fragments hold pixels


def test_the_smallest_map_is_taken_and_one_pixel_less_either_way_is_two_launches():
    """csrc/conv_block.hip choose_tile: ``if (tw > W || th < 4) continue`` with tw from 8: 8 x 4 is the smallest map; 7 x 4 and
    8 x 3 go to the two launches footprint_util.TINY_DECLINED names for the fused block"""
    _no_gpu()
    case = BDC.case_by_id("block_dw_smallest")
    assert (case["h"], case["w"]) == (BDC.SMALLEST_H, BDC.SMALLEST_W) == (4, 8)
    assert fu.block_tile(4, 8) == (8, 4) and fu.block_tile(4, 7) is None and fu.block_tile(3, 8) is None
    _, goes_to = fu.TINY_DECLINED["conv_block_fused_%s_x128"]
    for dtype in BDC.DTYPES:
        for mode in ("dense", "strided"):
            assert _row_plan(case, dtype, mode)[0] == [NAME[dtype], MARKER]
            for over in (dict(w=7), dict(h=3)):
                names = _row_plan(case, dtype, mode, **over)[0]
                assert names == [g % fu.TAG[dtype] for g in goes_to], (dtype, mode, over, names)


def test_block_dw_takes_the_row_below_4_gib_and_diverts_one_frame_later():
    """beside tests/test_big_operands_host.py's check for conv_block_fused: x and z at one stride, each within one frame below
    2^32 bytes, are named conv_block_dw; one frame later the pair is two launches, neither a block kernel"""
    _no_gpu()
    row = BDC.big_row()
    case = fu.big_case(row, "bf16")
    assert case["B"] == fu.big_case(fu.big_row("block_ragged_res"), "bf16")["B"]          # (the copies are no span operands)
    names, _, lay, _, _ = _row_plan(case, "bf16", "strided")
    assert names == [NAME["bf16"], MARKER], names
    x, z = lay["input"], lay["output"]
    assert x.ld == z.ld and x.body_bytes == z.body_bytes < fu.SPAN <= x.body_bytes + x.body_bytes // case["B"]
    names = _row_plan(case, "bf16", "strided", B=case["B"] + 1)[0]
    assert len(names) == 2 and MARKER not in names and not any(n.startswith("conv_block") for n in names), names


def test_the_small_network_of_the_gpu_tests_holds_the_kernel_where_the_table_says():
    """tests/block_dw_cases.py NET under fuse_block = 4, both types: the arena plan names the kernel on exactly NET_BLOCKS -- nine
    pairs on the 20 x 28 map, eight with the shortcut --, one of them writes a channel slice of a route buffer, none writes over
    its own input; under fuse_block = 3 the same network names it nowhere (27 rectangles on 256 CUs)"""
    import kernel_choice_util as K
    from yolov3 import _hip
    _no_gpu()
    lib = _hip.lib()
    model, h, w, batch = BDC.NET
    for dtype in BDC.DTYPES:
        for mode in (4, 3):
            opt = _hip.options(fuse_block=mode)
            ops, _, fake = K.build_ops(model, h, dtype, batch, "u8", opt, w)
            handle = ctypes.c_void_p()
            _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
            try:
                names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
            finally:
                lib.y3_plan_destroy(handle)
            ix = [i for i, n in enumerate(names) if n == NAME[dtype]]
            if mode == 3:
                assert ix == [] and not any("conv_block" in n for n in names)
                continue
            assert tuple(ops[i].block_idx for i in ix) == BDC.NET_BLOCKS
            assert all((ops[i].in_h, ops[i].in_w) == (20, 28) and not _overlap(ops[i], ops[i + 1]) for i in ix)
            assert sum(1 for i in ix if ops[i + 1].flags & _hip.F_RESIDUAL) == 8
            blk, c, ld = BDC.NET_ROUTE_SLICE
            assert [(ops[i + 1].out_c, ops[i + 1].out_ld) for i in ix if ops[i].block_idx == blk] == [(c, ld)]
            assert all(ops[i + 1].out_ld == ops[i + 1].out_c for i in ix if ops[i].block_idx != blk)


def test_set_tuning_accepts_3():
    from yolov3 import _hip
    lib = _hip.lib()
    try:
        assert lib.y3_set_tuning(b"fuse_block", 3) == 0 and _hip.options().fuse_block == 3
    finally:
        assert lib.y3_set_tuning(b"fuse_block", 0) == 0
    assert _hip.options().fuse_block == 0
