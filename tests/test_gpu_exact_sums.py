"""Every conv kernel, bit for bit, on operands whose float32 sum is one number in any order (tests/exact_sums.py has the plants,
the conditions that make them exact and the reference: an int64 convolution, then the epilogue rule of tests/epilogue_cases.py).

Per (case, storage type) of the footprint table whose group holds a conv -- every compiled conv instance the census ties to the
table, at the table's own shapes, tiny maps included -- and per plant (unit, wide_x, wide_w): one dense run through the one-op
harness of tests/test_gpu_footprint.py under the case's own option set, with the planted operands; the kernel is the family's,
the footprint is clean, and the output equals the reference in every bit.  No tolerance in any storage type.

The gates of the other suites (rtol 1e-4 in float32, a storage ulp in 16 bits) pass an accumulator narrowed between K-tiles, a
float32 operand that reaches the MFMA with half its significand, and one tap of one border column read twice; the suites that
hold kernels to EACH OTHER bit for bit pass whatever the families share.  Here each of those is a different bit pattern
(tests/test_exact_sums_host.py recomputes the reference under such faults).

Heads: the unit plant with |logit| <= 16.  The fused kernel equals conv + decode bit for bit on bbox, prob and cls, as the
footprint suite demands on random data, and the unfused conv's float32 logits -- the scratch operand between the two kernels --
equal the reference exactly.

The grouped and depthwise kernels are not rows of this table (tests/grouped_cases.py; tests/grouped_ordered.py restates their
sum order bit for bit).

Run time (profiles/exact_sums_gpu_tests.log): the file's 608 rows take 31 s together; a row takes hundredths of a second but for
the 96-pixel direct-weights 1x1 kernel, whose chooser wants 192 tiles -- 22496 pixels x 256 channels, 0.5 to 1.2 s, most of it
the reference's storage rounding on the CPU.  No plant was dropped for time.  Need an MI355X: -m gpu."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import exact_sums as XS
import footprint_util as fu

pytestmark = pytest.mark.gpu

IDS = ["%s-%s" % (c["id"], d) for c in fu.cases() if c["group"] in XS.GROUPS + ("head",) for d in c["dtypes"]]
# cases whose wide plants are not run to save time: none (the file takes about as long as the footprint suite's conv rows)
WIDE_DROPPED = ()


def _stored(outs, key, odt):
    dt = {"float32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[odt]
    t = outs[key]
    return t.contiguous().view(dt).reshape(t.shape[0], -1).float().numpy()


@pytest.mark.parametrize("cid", IDS)
def test_conv_sum_is_exact_on_planted_integers(cid):
    import kernel_census as census
    import test_gpu_footprint as F
    from yolov3 import _hip
    _hip.require_gpu()
    cname, dtype = cid.rsplit("-", 1)
    case = fu.case_by_id(cname)
    want_name = fu.family_name(case, dtype)
    odt = XS.out_dtype(case, dtype)
    for kind in XS.plants_of(case):
        p = XS.plant(case, dtype, kind)
        _, want = XS.reference(case, dtype, p)
        del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
        outs, msg, names, _, _ = F._run(case, dtype, "dense", plant=p)
        assert names[0] == want_name, (kind, names, want_name)
        assert msg is None, "%s plant: %s" % (kind, msg)
        if case["group"] == "head":
            plain, msg, pnames, _, _ = F._run(case, dtype, "dense", opt_name="head_unfused", plant=p)
            assert msg is None, msg
            assert pnames[0].startswith("conv_igemm_") and pnames[1] == "yolo_decode_f32", pnames
            for key in ("bbox/0", "prob/0", "cls/0"):
                assert torch.equal(outs[key], plain[key]), "%s: fused head differs from conv + decode in %s" % (cid, key)
                if key != "cls/0":
                    assert bool(torch.isfinite(plain[key].contiguous().view(torch.float32)).all()), key
            got = _stored(plain, "logits/0", "float32")
        else:
            got = _stored(outs, "output/0", odt)
        assert got.shape == want.shape, (got.shape, want.shape)
        diff = XS.first_difference(got, want, case, dtype, p)
        assert diff is None, "%s, %s plant (%s): %s" % (cid, kind, names[0], diff)
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
