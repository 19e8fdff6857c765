"""tests/exact_sums.py without a GPU: the plants meet the conditions that make the float32 sum one number, the reference is the
int64 convolution and the oracle's float64 one, every conv row of the footprint table is planted or excluded by name, and the
comparison would see each of four planted faults on every case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import epilogue_cases as EC
import exact_sums as XS
import footprint_util as fu

# Rows of the footprint table that hold a conv and are NOT planted, each with its reason.  None: every conv row of cases() and
# tiny_cases() is planted, the heads on the unit plant.  (The grouped and depthwise kernels are not rows of this table: they have
# tests/grouped_cases.py and their bit-for-bit restatement, tests/grouped_ordered.py.)
EXCLUDED = {}

CONV_GROUPS = XS.GROUPS + ("head",)


def _cases():
    return [c for c in fu.cases() if c["group"] in CONV_GROUPS]


def _ids():
    return [(c["id"], d) for c in _cases() for d in c["dtypes"]]


def test_every_conv_row_is_planted_or_excluded_by_name():
    """a new row of the table whose group holds a conv is in the GPU test's parametrisation, or named in EXCLUDED"""
    import test_gpu_exact_sums as G
    planted = set(G.IDS)
    holds_conv = lambda c: c["group"] not in ("layer", "reorg", "spp", "yolo")
    for c in fu.cases():
        for d in c["dtypes"]:
            cid = "%s-%s" % (c["id"], d)
            if holds_conv(c):
                assert (cid in planted) != (c["id"] in EXCLUDED), "%s is neither planted nor excluded (or both)" % cid
                assert c["group"] in CONV_GROUPS, "%s: a conv group tests/exact_sums.py does not know" % cid
            else:
                assert cid not in planted
    assert all(k in {c["id"] for c in fu.cases()} and reason for k, reason in EXCLUDED.items())
    # the wide plants are run on every case that has them: none was dropped for time
    assert G.WIDE_DROPPED == ()


def test_conv_specs_are_the_harness_own():
    import test_gpu_footprint as F
    for c in _cases():
        mine = [(s["cin"], s["cout"], s["k"], s["s"], s["leaky"]) for s in XS.conv_specs(c)]
        assert mine == [t[1:] for t in F._conv_specs(c)], c["id"]
        assert XS.conv_specs(c)[-1]["pad"] == c.get("pad", fu.conv_pad(XS.conv_specs(c)[-1]["k"]))


def test_the_bounds_are_the_formats_own():
    """2^24, 256 and 2048: the largest range in which float32, bf16 and fp16 hold EVERY integer"""
    for dtype, n in XS.EXACT_INT.items():
        r = EC.RND[dtype]
        ints = np.arange(-n, n + 1, dtype=np.float64) if n < (1 << 20) else np.asarray([n - 1, n, 1 - n, -n], dtype=np.float64)
        assert np.array_equal(r(ints.astype(np.float32)).astype(np.float64), ints)
        assert float(r(np.float32(n + 1))) != n + 1                   # the first integer the type does not hold
    assert XS.EXACT_F32 == 1 << 24 and float(np.float32(XS.EXACT_F32 + 1)) != XS.EXACT_F32 + 1
    assert XS.OUTSIDE_CAP == 0.01
    # the wide plants' amplitudes need exactly the type's significand: 8, 11 and 12 bits
    assert XS.WIDE == {"bf16": 255, "fp16": 2047, "float32": 4095}
    assert float(EC.rne_bf16(np.float32(255))) == 255 and float(EC.rne_bf16(np.float32(257))) != 257
    assert float(EC.rne_f16(np.float32(2047))) == 2047 and float(EC.rne_f16(np.float32(2049))) != 2049
    assert float(EC.rne_f16(np.float32(4095))) != 4095 and float(EC.rne_bf16(np.float32(4095))) != 4095
    assert float(np.float32(4095).astype(np.float32)) == 4095


def test_the_trial_behind_the_one_percent_cap():
    """20000 sums of 4608 products of {-1, 0, 1} x {-1, +1}: sigma about 56, none beyond 256"""
    rng = np.random.RandomState(4608)
    sums = np.zeros(20000, dtype=np.int64)
    for k0 in range(0, 4608, 512):
        sums += (rng.randint(-1, 2, (20000, 512)) * (rng.randint(0, 2, (20000, 512)) * 2 - 1)).sum(axis=1)
    assert 53 < sums.std() < 58 and np.abs(sums).max() <= 256, (sums.std(), np.abs(sums).max())


@pytest.mark.parametrize("cid", ["%s-%s" % p for p in _ids()])
def test_plants_meet_the_conditions_and_show_every_fault(cid):
    """(a), (b), (c) on every plant; then each fault, on a sample of the output pixels that holds the whole last column, must
    change at least one expected bit pattern on at least one plant of the case"""
    cname, dtype = cid.rsplit("-", 1)
    _conditions_and_faults(fu.case_by_id(cname), cid, dtype)


def _conditions_and_faults(case, cid, dtype):
    seen = dict.fromkeys((f for f in XS.FAULTS if XS.fault_applies(f, case, dtype)), 0)
    assert {"tap_shift", "drop_k"} <= set(seen)
    for kind in XS.plants_of(case):
        p = XS.plant(case, dtype, kind)
        last = XS.Last(case, dtype, p)
        XS.conditions(case, dtype, kind, p, last)
        rows = XS.sample_rows(last)
        for f in seen:
            n = XS.fault_changes(last, f, rows)
            seen[f] += n
            # a one-unit fault must show on the unit plant alone
            assert n > 0 or kind != "unit" or f not in ("tap_shift", "drop_k"), "%s: the unit plant does not see %s" % (cid, f)
    for f, n in seen.items():
        assert n > 0, "%s: no plant sees %s" % (cid, f)


def _block_dw_ids():
    import block_dw_cases as BDC
    return ["%s-%s" % p for p in BDC.case_ids()]


@pytest.mark.parametrize("cid", _block_dw_ids())
def test_block_dw_rows_meet_the_conditions_and_show_every_fault(cid):
    """the rows of tests/block_dw_cases.py (the direct-weights fused block: a table of its own), all three plants in both types
    as tests/test_gpu_block_dw_suites.py runs them: the same conditions -- (b): at most 1 % of the unit plant's pre-activations
    outside the output type's exact-integer range -- and each planted reference fault that applies (the three that a 16-bit
    activation conv has) changes an expected bit pattern"""
    import block_dw_cases as BDC
    import test_gpu_block_dw_suites as G
    assert cid in G.IDS and BDC.PLANTS == XS.PLANTS
    cname, dtype = cid.rsplit("-", 1)
    case = BDC.case_by_id(cname)
    assert XS.plants_of(case) == XS.PLANTS and XS.shortcut_kind(case) == ("input" if case["res"] else None)
    assert {f for f in XS.FAULTS if XS.fault_applies(f, case, dtype)} == {"tap_shift", "drop_k", "bf16_per_64"}
    _conditions_and_faults(case, cid, dtype)


SMALL = 3e8          # multiply-adds: the rows below it are held to a literal int64 sum and to the oracle (the rest share the code)


def _macs(case):
    sp = XS.conv_specs(case)[-1]
    ho, wo = XS.out_hw(case["h"], case["w"], sp)
    return case["B"] * ho * wo * sp["k"] ** 2 * sp["cin"] * sp["cout"]


@pytest.mark.parametrize("cname", [c["id"] for c in _cases() if len(XS.conv_specs(c)) == 1 and _macs(c) < SMALL])
def test_reference_is_the_int64_sum_and_the_oracles_float64_conv(cname):
    """unit plant: the pre-activation sum equals an int64 accumulation and oracle.darknet_oracle.conv_block(accumulate="f64")"""
    import torch
    from oracle import darknet_oracle as orc
    case = fu.case_by_id(cname)
    dtype = case["dtypes"][0]
    p = XS.plant(case, dtype, "unit")
    last = XS.Last(case, dtype, p)
    sp = last.sp
    acc = XS.to_int64(last.cols @ last.wm)
    literal = np.zeros_like(acc)
    cols, wm = last.cols.astype(np.int64), last.wm.astype(np.int64)
    for k in range(cols.shape[1]):
        literal += cols[:, k:k + 1] * wm[k:k + 1]
    assert np.array_equal(acc, literal)
    x = torch.from_numpy(np.ascontiguousarray(p["x"].transpose(0, 3, 1, 2)).astype(np.float32))
    zero = np.zeros(sp["cout"], dtype=np.float32)
    y = orc.conv_block(x, {"weight": p["convs"][0]["w"].astype(np.float32), "bias": zero}, sp["s"], sp["pad"], False, accumulate="f64")
    want = y.permute(0, 2, 3, 1).reshape(-1, sp["cout"]).numpy().astype(np.float64)
    assert np.array_equal(acc.astype(np.float64), want)
    # and the whole expectation, where the scale is 1 and no shortcut is added: the oracle's bias and leaky, rounded to storage
    t, stored = XS.reference(case, dtype, p)
    if XS.shortcut_kind(case) is None:
        one = p["convs"][0]["scale"] == 1.0
        yb = orc.conv_block(x, {"weight": p["convs"][0]["w"].astype(np.float32), "bias": p["convs"][0]["bias"]}, sp["s"], sp["pad"],
                            sp["leaky"], accumulate="f64")
        yb = yb.permute(0, 2, 3, 1).reshape(-1, sp["cout"]).numpy()
        got = EC.RND[XS.out_dtype(case, dtype)](yb)
        assert np.array_equal(EC.bits(got[:, one]), EC.bits(stored[:, one]))
