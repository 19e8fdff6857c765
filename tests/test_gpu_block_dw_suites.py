"""The direct-weights fused block kernel (csrc/conv_block_dw.hip, libyolov3_hip_block.so; y3_options.fuse_block = 3 / 4) in the
kernel-level suites, on every row of tests/block_dw_cases.py in both 16-bit storage types:

  footprint trio   tests/test_gpu_footprint.py's one-plan harness and its three gates.  Dense run against the oracle at the gate
                   of tests/test_gpu_bf16.py (one storage ulp, at most 2 % of the values, plus what a flipped rounding of the
                   intermediate can move).  Strided run: x and the output are channel slices of wider buffers of DIFFERENT pixel
                   strides, the shortcut reads x's slice, NaN round every input, NaN in the output slice -- it gives the dense
                   run's bits.  Not one byte outside the output slice (and the unused intermediate) changes.
  exact sums       the three plants of tests/exact_sums.py (unit, wide_x, wide_w): ``==`` on bit patterns against the int64
                   convolution's epilogue.
  below 2^32 bytes one bf16 row, x and z each one frame below 2^32 bytes behind a 4 GiB pad (the kernel keeps 32-bit byte
                   offsets; the chooser diverts the pair one frame later: tests/test_block_dw_host.py).

Every run asserts its launch set against tests/golden/kernel_instances_block.json (the "block" library of tests/kernel_census.py),
and the fragment-order copies -- made by y3_conv_make_fragment_weights inside the harness, which holds that call to its own operand
-- against the main census.  The epilogue pins of this kernel are tests/test_gpu_epilogue.py's, the network runs
tests/test_gpu_block_dw_network.py's.  Need an MI355X: -m gpu."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_dw_cases as BDC  # noqa: E402
import exact_sums as XS  # noqa: E402
import footprint_util as fu  # noqa: E402
import kernel_census as census  # noqa: E402

pytestmark = pytest.mark.gpu

MARKER = "(fused into the previous op)"
IDS = ["%s-%s" % p for p in BDC.case_ids()]


def assert_census(key, fragment_calls):
    """the logged plan runs launched the instance recorded for ``key`` in the block census and nothing else; the
    ``fragment_calls`` copies the harness made launched what the main census records for y3_conv_make_fragment_weights"""
    assert census.LAUNCHED and all(len(s) == 1 and "conv_block_dw_kernel" in s[0] for s in census.LAUNCHED), census.LAUNCHED
    census.assert_census(key, library="block")
    assert len(census.FRAGMENT_LAUNCHED) == fragment_calls, census.FRAGMENT_LAUNCHED
    census.assert_census(census.FRAGMENT_KEY, launched=census.FRAGMENT_LAUNCHED[:])
    del census.FRAGMENT_LAUNCHED[:]


@pytest.mark.parametrize("cid", IDS)
def test_block_dw_touches_exactly_its_operands(cid):
    import test_gpu_footprint as F
    from yolov3 import _hip
    _hip.require_gpu()
    cname, dtype = cid.rsplit("-", 1)
    case = BDC.case_by_id(cname)
    want = [fu.family_name(case, dtype), MARKER]
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
    dense, msg, names, ref, lay = F._run(case, dtype, "dense")
    assert names == want, (names, want)
    assert msg is None, "dense run: " + msg
    F._no_nan(dense, lay)
    F._check_dense_against_oracle(case, dtype, dense, ref, lay)

    strided, msg, names, _, slay = F._run(case, dtype, "strided")
    assert names == want, (names, want)
    x, z = slay["input"], slay["output"]
    assert x.slices[0][0] > 0 and z.slices[0][0] > 0 and x.ld != z.ld and x.ld > case["cin"] and z.ld > case["cout"], (x.ld, z.ld)
    assert msg is None, "strided run: " + msg
    F._no_nan(strided, slay)
    assert strided.keys() == dense.keys() == {"output/0"}
    differ = int((strided["output/0"] != dense["output/0"]).sum())
    assert differ == 0, "%d bytes of the strided, poisoned run differ from the dense run" % differ
    assert len(census.LAUNCHED) == 2
    assert_census(BDC.footprint_key(cname, dtype), 4)


@pytest.mark.parametrize("kind", BDC.PLANTS)
@pytest.mark.parametrize("cid", IDS)
def test_block_dw_sum_is_exact_on_planted_integers(cid, kind):
    import numpy as np

    import test_gpu_footprint as F
    from yolov3 import _hip
    _hip.require_gpu()
    cname, dtype = cid.rsplit("-", 1)
    case = BDC.case_by_id(cname)
    p = XS.plant(case, dtype, kind)
    _, want = XS.reference(case, dtype, p)
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
    outs, msg, names, _, _ = F._run(case, dtype, "dense", plant=p)
    assert names == [fu.family_name(case, dtype), MARKER], names
    assert msg is None, msg
    t = outs["output/0"]
    got = t.contiguous().view(fu.TORCH_DT[dtype]).reshape(t.shape[0], -1).float().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), XS.first_difference(got, want, case, dtype, p)
    assert_census(BDC.exact_key(cname, dtype, kind), 2)


def test_block_dw_one_frame_below_4_gib():
    """x and z each within one frame below 2^32 bytes, at one stride, behind the 4 GiB pad in one allocation; frame b of x is
    base frame b % 3.  The output equals, frame by frame and bit for bit, the same family on the three base frames; it holds no
    NaN; nothing outside the output slice changed (tests/test_gpu_big_operands.py ``big_operands_run``)."""
    import test_gpu_big_operands as TB
    import test_gpu_footprint as F
    row = BDC.big_row()
    case = fu.big_case(row, "bf16")
    assert case["same_ld"] and case["B"] > 3000
    TB.big_operands_run(row, "bf16", log=True)
    assert census.LAUNCHED and all(len(s) == 1 and "conv_block_dw_kernel" in s[0] for s in census.LAUNCHED), census.LAUNCHED
    census.assert_census(BDC.big_key("bf16"), library="block")
    del census.FRAGMENT_LAUNCHED[:]
