"""Every kernel family on operands whose byte offsets pass 2^32 (tests/footprint_util.py big_cases(); the host half, with the
refusals at 2^31 pixels and the families whose own rules keep them small, is tests/test_big_operands_host.py).

One device allocation per case, ``[pad of 4 GiB][operand][operand] ...``, every operand ``[guard | body | guard]`` in the strided
layout of tests/test_gpu_footprint.py: an address that wraps at 2^32 or a sign-extended 32-bit offset lands in the pad or in a
neighbouring operand -- recorded, never a fault.  The inputs' frame b holds base frame b % 3 of three random frames (expanded on
the device), NaN round them; the output slice is prefilled with NaN, the byte pattern round it.  After the run, through
y3_plan_create_ex / y3_plan_run with the family name asserted:

  (a) frames 0-2 and the last three hold, bit for bit, what the SAME family gives on the three base frames alone, run dense
      between zero guards -- and that small run passes the suite's oracle gate (test_gpu_footprint._check_dense_against_oracle);
  (b) every frame b of the output equals its frame b % 3 bit for bit, and no element is NaN: position independence, which only
      holds if every address of every frame was right;
  (c) the pad, every guard, every margin and every read-only operand is byte for byte what it was.

No tolerance of its own: the gates are those of tests/test_gpu_footprint.py.  A case takes 8 to 30 GiB for its allocation and as
much again for the copy (c) compares with; it is skipped where the device has less free (an MI355X has 288 GB: no skip there).
Need an MI355X: -m gpu."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import footprint_util as fu
import kernel_census as census
import test_gpu_footprint as G

pytestmark = pytest.mark.gpu

FRAME_OPERANDS = ("input", "input/output", "residual")       # input-side operands that hold one frame per batch entry
SLACK = 3 << 30                                              # temporaries of the fills and checks, the small run


def _big_data(case, dtype, lay, paths, dev):
    """the data of the three-frame case (seeded by the case's id, as every run of it is), its frame operands expanded on the
    device: frame b of the big operand is frame b % 3"""
    small = dict(case, B=3)
    opt = fu._H().options(**fu._opts()[case["opt"]])
    _, lay3, _, _ = fu.build(small, dtype, "strided", opt)
    data, _ = G._make_data(small, dtype, lay3, paths)
    idx = torch.arange(case["B"], device=dev) % 3
    for name in FRAME_OPERANDS:
        if name in data:
            o = lay[name]
            base = data[name][0].to(dev).reshape(3, -1)
            data[name] = [base[idx].reshape(o.pixels, -1)]
    for o in lay.operands:                                   # (a fragment-order copy only the big grid's kernel reads: made below)
        if o.side == "in" and o.name not in data:
            assert o.name.endswith("fragment weights"), o.name
            data[o.name] = [torch.zeros(o.slices[0][1], dtype=fu.TORCH_DT[dtype])]
    return data


@pytest.mark.parametrize("cid", ["%s-%s" % p for p in fu.big_case_ids()])
def test_kernel_addresses_operands_past_4_gib(cid):
    cname, dtype = cid.rsplit("-", 1)
    big_operands_run(fu.big_row(cname), dtype)


def big_operands_run(row, dtype, log=False):
    """the whole check for one row of big_cases() -- or a row in its format from another table (tests/block_dw_cases.py big_row).
    ``log``: the big run is taken with the launch log and its symbols are left in test_gpu_footprint.LAUNCHED"""
    from yolov3 import _hip as H
    H.require_gpu()
    lib = H.lib()
    dev = torch.device("cuda:0")
    cid = "%s-%s" % (row["id"], dtype)
    case = fu.big_case(row, dtype)
    B = case["B"]
    want = fu.family_name(row, dtype)
    opt = H.options(**fu._opts()[row["opt"]])
    _, lay0, _, _ = fu.build(case, dtype, "strided", opt, lead=[fu.pad_operand()])
    need = 2 * lay0.total + SLACK
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("%s needs %.1f GiB of device memory, %.1f GiB are free" % (cid, need / 2.0 ** 30, free / 2.0 ** 30))

    # ---- the three base frames alone, dense between zero guards: the oracle gate, and what (a) compares with
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
    small = dict(case, B=3)
    dense, msg, names, ref, lay3 = G._run(small, dtype, "dense")
    assert names[0] == want, (names, want)
    assert msg is None, "small dense run: " + msg
    G._no_nan(dense, lay3)
    G._check_dense_against_oracle(small, dtype, dense, ref, lay3)
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]

    # ---- the big run
    raw = torch.empty(lay0.total + fu.ALIGN, dtype=torch.uint8, device=dev)
    shift = -raw.data_ptr() % fu.ALIGN
    alloc = raw[shift:shift + lay0.total]
    base = alloc.data_ptr()
    ops, lay, frag, path = fu.build(case, dtype, "strided", opt, base, lead=[fu.pad_operand()])
    assert lay.total == lay0.total and lay.operands[0].name == "pad" and lay.operands[0].body_bytes >= (1 << 32)
    data = _big_data(case, dtype, lay, [path, H.PATH_IGEMM], dev)
    fu.fill(alloc, lay, data, poisoned=True, u8_guard=0xFF)
    del data
    for i in frag:
        H.check(lib.y3_conv_make_fragment_weights(ctypes.byref(ops[i]), ctypes.c_void_p(ops[i].d_weight_frag), None))
    torch.cuda.synchronize()
    handle = ctypes.c_void_p()
    H.check(lib.y3_plan_create_ex(ops, len(ops), lay["zero page"].ptr(base), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
        assert names[0] == want and all(n == "(fused into the previous op)" for n in names[1:]), (names, want)
        before = alloc.clone()
        d_input = lay["input"].ptr(base) if lay.has("input") else None
        if log:
            census.logged(lambda: H.check(lib.y3_plan_run(handle, d_input, None)))
        else:
            H.check(lib.y3_plan_run(handle, d_input, None))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)

    try:
        # (c) nothing but the output slices (and the private intermediate of a fused group) changed
        for i, name in frag.items():
            assert lay[name].side == "in"                      # (the fragment-order copy was made before ``before``)
        msg = fu.region_violations(before, alloc, lay)
        assert msg is None, msg
        del before
        n_out = 0
        for o in lay.operands:
            if o.side not in ("out", "inout"):
                continue
            for k in range(len(o.slices)):
                key = "%s/%d" % (o.name, k)
                t = fu.read_slice(alloc, o, k, torch.uint8)
                f = t.reshape(B, -1)
                three = dense[key].reshape(3, -1).to(dev)
                assert three.shape[1] == f.shape[1], (key, tuple(three.shape), tuple(f.shape))
                # (a) the first and the last three frames against the small run of the same family
                for b in (0, 1, 2, B - 3, B - 2, B - 1):
                    differ = int((f[b] != three[b % 3]).sum())
                    assert differ == 0, "%s: frame %d of %d differs from the three-frame run's frame %d in %d of %d bytes" % (
                        key, b, B, b % 3, differ, f.shape[1])
                # (b) no NaN, and every frame is frame b % 3
                msg = fu.nan_violations(t, B, o.fmt) or fu.frame_violations(t, B)
                assert msg is None, "%s: %s" % (key, msg)
                n_out += 1
                del t, f, three
        assert n_out >= 1
    finally:
        before = alloc = raw = None
        torch.cuda.empty_cache()
