"""The direct-weights form of the fused 1x1 -> 3x3 (+ shortcut) kernel (csrc/conv_block_dw.hip, libyolov3_hip_block.so;
y3_options.fuse_block = 3, and 4 = wherever supported for the small maps here) against the two separate launches of the same
plan under fuse_block = 0: same operands, same K order, same epilogue arithmetic -> ``torch.equal``.  Every case also asserts,
through the library's launch log, that it launched the symbol tests/golden/kernel_instances_block.json records for it
(``kernel_census.assert_census``; tools/make_kernel_instances.py --library block writes that file on an MI355X).

One case more goes against a float64 oracle at the one-ulp gate of tests/test_gpu_bf16.py, and one runs beside the
memory-saturating copy kernel as tests/test_gpu_contention.py runs the other run-ahead families: a mis-counted wait shows there
as a changed bit.  The kernel-level suites -- strided slices and footprint, the three integer plants of tests/exact_sums.py, the
row below 2^32 bytes -- are tests/test_gpu_block_dw_suites.py, on the table of tests/block_dw_cases.py.
Need an MI355X: -m gpu."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_dw_util as BU  # noqa: E402
import kernel_census as census  # noqa: E402

pytestmark = pytest.mark.gpu

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _run(ops, t, shape, dtype, mode, log_key=None):
    """the pair's output under fuse_block = mode (on a background of 7.0), the kernel name of op 0, the grid of op 0"""
    from yolov3 import _hip
    lib = _hip.lib()
    out = torch.full(shape, 7.0, dtype=TDT[dtype], device=t["x"].device)
    plan = BU.make_plan(ops, t["zero"], out, fuse_block=mode)
    try:
        name, grid = lib.y3_plan_op_kernel(plan, 0).decode(), _hip.plan_op_dims(plan, 0)[0]
        with _hip.launch_log() as log:
            _hip.check(lib.y3_plan_run(plan, None, _hip.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(plan)
    if log_key:
        assert all("conv_block_dw_kernel" in s for s in log.symbols) and len(log.names) == 1, log.names
        census.assert_census(log_key, library="block", launched=[log.symbols])
    return out, name, grid


@pytest.mark.parametrize("m,c,dtype", BU.CASES, ids=[BU.case_key(*k) for k in BU.CASES])
def test_block_dw_is_bit_identical_to_the_two_launches(m, c, dtype):
    from yolov3 import _hip
    _hip.require_gpu()
    (h, w), (cin, cout, res) = BU.MAPS[m], BU.CHANNELS[c]
    t, ops, _, _ = BU.random_pair(torch.device("cuda:0"), dtype, BU.FRAMES, h, w, cin, cout, res, seed=h * 131 + w * 7 + cin)
    shape = (BU.FRAMES, h, w, cout)
    fused, n_f, grid = _run(ops, t, shape, dtype, 4, BU.case_key(m, c, dtype))
    plain, n_p, _ = _run(ops, t, shape, dtype, 0)
    assert n_f == "conv_block_dw_%s_x128" % BU.TAG[dtype], n_f
    assert not n_p.startswith("conv_block"), n_p
    tx, ty = BU.RECTANGLES[m][2:]
    assert grid == tx * ty * BU.FRAMES, (grid, BU.RECTANGLES[m])
    assert torch.isfinite(plain.float()).all() and float(plain.float().abs().max()) > 0
    assert torch.equal(fused, plain), "%d values differ, max |d| %g" % (
        int((fused != plain).sum()), float((fused.float() - plain.float()).abs().max()))


def test_block_dw_fills_the_chip_or_declines_and_needs_both_fragment_copies():
    """fuse_block = 3 takes the pair at 76^2 x 16 frames (256 rectangles) and declines it at two frames (the 70 % rule of
    fuse_block = 1); 4 takes it there; without either fragment-order copy both run two launches; 0, 1 and 2 never name it."""
    from yolov3 import _hip
    lib = _hip.lib()
    _hip.require_gpu()
    dev = torch.device("cuda:0")
    for batch in (16, 2):
        t, ops, _, _ = BU.random_pair(dev, "bf16", batch, 76, 76, 256, 256, True, seed=1)
        out = torch.zeros((batch, 76, 76, 256), dtype=torch.bfloat16, device=dev)

        def name(**options):
            plan = BU.make_plan(ops, t["zero"], out, **options)
            n = lib.y3_plan_op_kernel(plan, 0).decode()
            lib.y3_plan_destroy(plan)
            return n
        assert name(fuse_block=3).startswith("conv_block_dw") == (batch == 16), (batch, name(fuse_block=3))
        assert name(fuse_block=4) == "conv_block_dw_bf16_x128"
        for mode in (0, 1, 2):
            assert "block_dw" not in name(fuse_block=mode), (batch, mode)
        for n in (0, 1):
            keep = ops[n].d_weight_frag
            ops[n].d_weight_frag = None
            assert not name(fuse_block=4).startswith("conv_block"), (batch, n, name(fuse_block=4))
            ops[n].d_weight_frag = keep


def test_block_dw_against_the_float64_oracle_at_one_ulp():
    """38 x 38, Cin 256, shortcut, bf16: each conv in float64 from the operands the kernel reads, the intermediate rounded to
    bf16 once, at the gate of tests/test_gpu_bf16.py (one bf16 ulp, at most 2 % of the values on the other side of a rounding
    boundary, plus what a flipped rounding of the intermediate can move)."""
    import test_gpu_bf16 as TB
    from oracle import darknet_oracle as orc
    from yolov3 import _hip
    _hip.require_gpu()
    h = w = 38
    t, ops, x, convs = BU.random_pair(torch.device("cuda:0"), "bf16", BU.FRAMES, h, w, 256, 256, True, seed=77)
    got, name, _ = _run(ops, t, (BU.FRAMES, h, w, 256), "bf16", 4, "block_dw_oracle-bf16")
    assert name == "conv_block_dw_bf16_x128"
    F = torch.nn.functional
    xn = x.permute(0, 3, 1, 2).double()
    a1, b1 = convs[0]["scale"].double().reshape(1, -1, 1, 1), convs[0]["bias"].double().reshape(1, -1, 1, 1)
    a2, b2 = convs[1]["scale"].double().reshape(1, -1, 1, 1), convs[1]["bias"].double().reshape(1, -1, 1, 1)
    mid = F.leaky_relu(F.conv2d(xn, convs[0]["w"].double()) * a1 + b1, 0.1).float()
    slack = TB._flip_slack(mid, convs[1]["w"], convs[1]["scale"], 1, 1, "bf16")
    z = F.leaky_relu(F.conv2d(orc.bf16_round(mid).double(), convs[1]["w"].double(), padding=1) * a2 + b2, 0.1) + xn
    TB._close_bf16(got.float().cpu().permute(0, 3, 1, 2), orc.bf16_round(z.float()), "block_dw 38x38 bf16", slack, "bf16")


CONTENTION = [(True, "bf16"), (False, "bf16"), (True, "fp16")]


@pytest.mark.parametrize("res,dtype", CONTENTION)
def test_block_dw_beside_a_copy_kernel(res, dtype):
    """76^2 x 16 frames under fuse_block = 3 (the shipped shape: one rectangle per CU) beside the copy kernel, exactly as
    tests/test_gpu_contention.py runs the other run-ahead families: quiet output against contended output, bit for bit.
    Both compiled instances run here (tests/test_block_dw_host.py holds the census to that)."""
    import test_gpu_contention as TC
    from yolov3 import _hip
    lib = _hip.lib()
    _hip.require_gpu()
    dev = torch.device("cuda:0")
    t, ops, _, _ = BU.random_pair(dev, dtype, 16, 76, 76, 256, 256, res, seed=7)
    out = torch.zeros((16, 76, 76, 256), dtype=TDT[dtype], device=dev)
    handle = BU.make_plan(ops, t["zero"], out, fuse_block=3)
    try:
        assert lib.y3_plan_op_kernel(handle, 0).decode() == "conv_block_dw_%s_x128" % BU.TAG[dtype]
        TC._beside_a_copy(handle, out, "block_dw_%s-%s" % ("res" if res else "nores", dtype), library="block")
    finally:
        lib.y3_plan_destroy(handle)
