"""CPU-side checks of the direct-weights fused block kernel (csrc/conv_block_dw.hip; y3_options.fuse_block = 3 / 4): the
shared library it lives in -- gfx950 code only, no scratch, register and LDS budgets, its census
(tests/golden/kernel_instances_block.json) -- and where plans name it, through the fake-address route of
tests/kernel_choice_util.py.  That every configuration of tests/golden/kernel_choice.json still reproduces, and that the main
library's census is what it was, is tests/test_kernel_choice.py's and tests/test_code_object.py's to say: they run unchanged."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_dw_util as BU  # noqa: E402

NAME = {"bf16": "conv_block_dw_bf16_x128", "fp16": "conv_block_dw_f16_x128"}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(BU.BLOCK_LIB):
        pytest.fail("libyolov3_hip_block.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    return BU.library_kernels()          # (asserts: device code for gfx950 only)


def test_block_library_budgets(kernels):
    """no scratch, at most 512 VGPR + AGPR, at most 160 KiB of LDS (static; the launch's dynamic size is a plan's to say, below)"""
    assert len(kernels) == 2, [k[".name"] for k in kernels]
    for k in kernels:
        name = k[".name"]
        assert "conv_block_dw_kernel" in name, name
        assert k[".private_segment_fixed_size"] == 0, (name, "uses scratch memory (register spills)")
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 512, name
        assert k[".vgpr_count"] <= 256, name
        assert k[".group_segment_fixed_size"] <= 160 * 1024, name
        assert k[".wavefront_size"] == 64 and k[".max_flat_workgroup_size"] == 512, name


def test_block_library_census(kernels):
    """the library's symbols equal the fixture's: every compiled kernel launched by a recorded case and by a contention case, no
    recorded symbol the library lacks; every case of tests/test_gpu_block_dw.py has its entry"""
    fixture = BU.load_census()
    library = {k[".name"] for k in kernels}
    uncovered, stale, quiet_only = BU.census_report(fixture, library)
    assert not uncovered and not stale and not quiet_only, (uncovered, stale, quiet_only)
    assert set(fixture) == {"footprint", "contention"}
    for table in fixture.values():
        for key, syms in table.items():
            assert syms == sorted(set(syms)) and len(syms) == 1, key
            assert ("IDF16bE" in syms[0]) == key.endswith("-bf16") and ("IDF16_E" in syms[0]) == key.endswith("-fp16"), (key, syms)
    want = {BU.case_key(*c) for c in BU.CASES} | {"block_dw_oracle-bf16", "block_dw_exact_unit-bf16", "block_dw_exact_unit-fp16"}
    assert set(fixture["footprint"]) == want
    assert set(fixture["contention"]) == {"block_dw_res-bf16", "block_dw_nores-bf16", "block_dw_res-fp16"}


def test_main_library_names_the_block_library_as_a_dependency():
    with open(os.path.join(os.path.dirname(BU.BLOCK_LIB), "libyolov3_hip.so"), "rb") as f:
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


def test_set_tuning_accepts_3():
    from yolov3 import _hip
    lib = _hip.lib()
    try:
        assert lib.y3_set_tuning(b"fuse_block", 3) == 0 and _hip.options().fuse_block == 3
    finally:
        assert lib.y3_set_tuning(b"fuse_block", 0) == 0
    assert _hip.options().fuse_block == 0
