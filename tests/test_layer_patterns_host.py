"""tests/layer_patterns.py held to itself and to the existing oracles (CPU only): the two statements of each reference agree on
every case; on the maps without NaN and without a tie of the two zeros the pool reference is torch's pool (oracle.maxpool,
darknet_pool_restate.pool) bit for bit; the expected outputs of every form and dtype contain the values and situations that the
GPU tests (tests/test_gpu_layer_patterns.py) are there for; and every wrong rule a kernel could plausibly implement gives other
bits than the reference on at least one case, so the cases can tell."""
import numpy as np
import pytest
import torch

from oracle import darknet_oracle as orc

import darknet_pool_restate as DP
import layer_patterns as L

FORMS = ("maxpool", "maxpool_dk", "spp", "spp_dk")


def _cases(form, dtype):
    for label, m in L.pool_inputs(form, dtype):
        for k, s in L.pool_ks(form):
            yield label, m, k, s


def test_sort_key_is_the_maximum_order():
    for dtype in L.DTYPES:
        o = L.ordered(dtype)
        k = L.key(o, dtype)
        assert np.array_equal(L.unkey(k, dtype), o) and np.unique(k).size == o.size
        f = L.to_float(o, dtype)[np.argsort(k)].astype(np.float64)
        assert (np.diff(f) >= 0).all()                                                    # key order is value order ...
        assert L.key(L.sign_bit(dtype), dtype) == -1 and L.key(0, dtype) == 0             # ... with -0 just below +0
        assert not L.is_nan(o, dtype).any() and L.is_nan(L.nans(dtype), dtype).all()
        assert np.array_equal(L.rne(L.to_float(o, dtype), dtype), o)
        if L.bits(dtype) == 16:
            assert o.size + L.nans(dtype).size == 1 << 16
        else:
            assert set(L.planted_f32().tolist()) <= set(o.tolist()) and o.size >= 4096
            quiet = (L.nans(dtype) & 0x00400000) != 0
            assert quiet.any() and (~quiet).any() and len(set((L.nans(dtype) >> 31).tolist())) == 2
        for kind in ("perm", "neighbours"):                                               # the ordered maps hold the whole set
            for shape in (L.WIDE, L.ELEM, (L.spp_frames(dtype),) + L.SPP_FRAME):
                have = set(L.input_map(kind, dtype, shape).ravel().tolist())
                missing = set(o.tolist()) - have
                assert missing <= ({L.sign_bit(dtype)} if kind == "neighbours" else set()), (dtype, kind, shape)


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_two_statements_of_each_reference_agree(dtype):
    for form in FORMS:
        for label, m, k, s in _cases(form, dtype):
            a = L.pool_expected(form, dtype, label, k, s)
            b = L.pool_taps(m, dtype, k, s, form.endswith("_dk"))
            assert np.array_equal(a, b), (dtype, form, label, k, s)
    for shape in (L.WIDE_UP, L.ELEM_UP):
        m = L.input_map("all", dtype, shape)
        for s in L.UPSAMPLE_STRIDES:
            assert np.array_equal(L.upsample_gather(m, s), L.upsample_repeat(m, s))
    for shape in (L.WIDE, L.ELEM):
        for name, a, b in L.add_cases(dtype, shape):
            x, y = L.add_torch(a, b, dtype), L.add_numpy(a, b, dtype)
            assert np.array_equal(L.canon_nan(x, dtype), L.canon_nan(y, dtype)), (dtype, name)
            assert np.array_equal(L.is_nan(x, dtype), L.is_nan(y, dtype))


def _oracle(m, dtype, k, s, darknet):
    """torch's pool on the map, through the oracle the existing tests use -> patterns (B, Ho, Wo, C)"""
    x = L.to_torch(m, dtype).float().permute(0, 3, 1, 2).contiguous()
    y = DP.pool(x, k, s) if darknet else orc.maxpool(x, k, s)
    return L.from_torch(y.permute(0, 2, 3, 1).to(L.torch_dtype(dtype)))


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_reference_is_the_oracles_pool_where_torch_has_the_same_rule(dtype):
    """torch keeps a NaN tap and resolves a tie of -0 and +0 by scan order; everywhere else it must agree with the reference in
    every bit.  The ordered maps have no such window at all; on the zeros and NaN maps the share left out is printed."""
    for form in FORMS:
        darknet = form.endswith("_dk")
        for label, m, k, s in _cases(form, dtype):
            st = L.pool_stats(m, dtype, k, s, darknet)
            left_out = st["nan"] | st["tie"]
            want, got = L.pool_expected(form, dtype, label, k, s), _oracle(m, dtype, k, s, darknet)
            assert got.shape == want.shape
            assert np.array_equal(got[~left_out], want[~left_out]), (dtype, form, label, k, s)
            share = float(left_out.mean())
            print("%s %s %s k=%d s=%d: %d of %d windows left out (%.1f %%)" % (dtype, form, label, k, s, left_out.sum(), left_out.size, 100 * share))
            kind = label.split("/")[1]
            if kind in ("perm", "neighbours"):
                assert not st["tie"].any() and not st["nan"].any(), (dtype, form, label, k, s)
            else:
                # some windows are what the map is for; some compare (a 9 or 13 window of the NaN map always holds a NaN)
                assert share > 0 and (share < 1 or k > 5), (dtype, form, label, k, s, share)
            if kind == "zeros":
                assert st["tie"].any() and not st["nan"].any()
            if kind == "nan":
                assert st["nan"].any()


def _in_range(pat, dtype, lo, hi):
    mag = pat.astype(np.int64) & (L.sign_bit(dtype) - 1)
    return (mag >= lo) & (mag <= hi)


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("form", FORMS)
def test_expected_outputs_cover_what_the_gpu_tests_are_for(form, dtype):
    darknet = form.endswith("_dk")
    bd = L.boundary(dtype)
    seen = set()
    all_nan_gives_neg_inf = False
    adjacent = {"normal": 0, "subnormal": 0, "across zero": 0}
    lone_positions = set()
    sub_max, norm_min, fin_max = bd["+sub_max"], bd["+norm_min"], bd["+max"]
    for label, m, k, s in _cases(form, dtype):
        want = L.pool_expected(form, dtype, label, k, s)
        seen |= set(np.unique(want).tolist()) & set(bd.values())
        small = k <= 5
        st = L.pool_stats(m, dtype, k, s, darknet, taps=small)
        all_nan_gives_neg_inf |= bool((st["empty"] & (want == L.neg_inf(dtype))).any())
        if small:
            adj = st["adjacent"] == 1
            win, run = L.unkey(st["winner"][adj], dtype), L.unkey(st["winner"][adj] - 1, dtype)
            adjacent["across zero"] += int(((win == 0) & (run == L.sign_bit(dtype))).sum())
            adjacent["subnormal"] += int((_in_range(win, dtype, 1, sub_max) & _in_range(run, dtype, 1, sub_max)).sum())
            adjacent["normal"] += int((_in_range(win, dtype, norm_min, fin_max) & _in_range(run, dtype, norm_min, fin_max)).sum())
        if k == 2:
            lone_positions |= set(np.unique(st["lone"]).tolist()) - {-1}
    for name in ("+zero", "-zero", "+sub_min", "-sub_min", "+sub_max", "-sub_max", "+inf", "-inf", "+max", "-max"):
        assert bd[name] in seen, (form, dtype, name)
    assert all_nan_gives_neg_inf
    print(form, dtype, "windows whose winner and runner-up are adjacent patterns:", adjacent)
    assert all(n > 0 for n in adjacent.values()), adjacent
    if not form.startswith("spp"):
        assert lone_positions == {0, 1, 2, 3}, lone_positions


def test_other_inputs_cover_their_sets():
    for dtype in L.DTYPES:
        every = set(L.ordered(dtype).tolist()) | set(L.nans(dtype).tolist())
        for shape in (L.WIDE, L.ELEM, L.WIDE_UP, L.ELEM_UP):
            assert set(L.input_map("all", dtype, shape).ravel().tolist()) == every
        for shape in (L.WIDE, L.ELEM):
            cases = L.add_cases(dtype, shape)
            if L.bits(dtype) == 16:
                assert [c[0] for c in cases] == list(L.SECOND) and len(cases) == 16
                assert set(cases[0][1].ravel().tolist()) == set(L.ordered(dtype).tolist())
            want = np.concatenate([L.add_torch(a, b, dtype).ravel() for _, a, b in cases])
            bd = L.boundary(dtype)
            have = set(np.unique(want).tolist())
            # subnormal results, overflow to both infinities, both zeros, and NaN from inf - inf and from a NaN operand
            assert {bd[n] for n in ("+zero", "-zero", "+sub_min", "-sub_min", "+sub_max", "-sub_max", "+inf", "-inf", "+max", "-max")} <= have
            assert L.is_nan(want, dtype).any()
        if L.bits(dtype) == 16:
            # the tie-making operands make ties: the exact sum lies half way between two patterns, for both parities of a
            a = L.ordered(dtype)
            a = a[_in_range(a, dtype, bd["+norm_min"], bd["+max"] - 2)]
            for which in ("+half_ulp", "-half_ulp", "+3half_ulp", "-3half_ulp"):
                exact = L.to_float(a, dtype).astype(np.float64) + L.to_float(L.add_second(a, which, dtype), dtype).astype(np.float64)
                got = L.to_float(L.add_numpy(a, L.add_second(a, which, dtype), dtype), dtype).astype(np.float64)
                ulp = np.abs(L.to_float(a + np.uint16(1), dtype).astype(np.float64) - L.to_float(a, dtype).astype(np.float64))
                ties = np.abs(np.abs(got - exact) - ulp / 2) < ulp * 1e-9
                ties |= np.abs(np.abs(got - exact) - ulp / 4) < ulp * 1e-9        # below a power of two the lower neighbour is half as far
                assert ties.mean() > 0.95, (dtype, which, ties.mean())
                assert (L.add_numpy(a, L.add_second(a, which, dtype), dtype) & 1 == 0)[ties].all()      # ... broken to even


# ---- teeth: a wrong rule gives other bits on at least one case of every dtype it applies to ----------------------------------

def _pool_differs(dtype, **wrong):
    n = 0
    for form in ("maxpool", "maxpool_dk", "spp"):
        for label, m, k, s in _cases(form, dtype):
            if k > 5:
                continue
            got = L.pool_taps(m, dtype, k, s, form.endswith("_dk"), **wrong)
            n += int(not np.array_equal(got, L.pool_expected(form, dtype, label, k, s)))
    return n


WRONG_POOLS = {
    "x >= y ? x : y in a cascade": (dict(rule=L.wrong_ge_cascade), L.DTYPES),
    "a > b ? a : b": (dict(rule=L.wrong_gt), L.DTYPES),
    "NaN propagating": (dict(rule=L.wrong_nan_propagates), L.DTYPES),
    "subnormal inputs flushed to zero": (dict(flush=True), L.DTYPES),
    "winner taken from a fixed tap": (dict(fixed_tap=(0, 0)), L.DTYPES),
    "comparison after narrowing float32 to bf16": (dict(rule=L.wrong_bf16_compare), ("float32",)),
}
WRONG_ADDS = {
    "sum rounded twice, through fp16": (L.wrong_add_through_fp16, ("float32", "bf16")),
    "operands narrowed through fp16": (L.wrong_add_operands_through_fp16, ("float32", "bf16")),
    "in place, reading its own output": (L.wrong_add_rereads_output, L.DTYPES),
}


@pytest.mark.parametrize("name", sorted(WRONG_POOLS))
def test_cases_tell_a_wrong_pool_rule(name):
    wrong, dtypes = WRONG_POOLS[name]
    for dtype in dtypes:
        n = _pool_differs(dtype, **wrong)
        print("%s, %s: %d cases give other bits" % (name, dtype, n))
        assert n > 0, (name, dtype)


@pytest.mark.parametrize("name", sorted(WRONG_ADDS))
def test_cases_tell_a_wrong_add(name):
    wrong, dtypes = WRONG_ADDS[name]
    for dtype in dtypes:
        n = 0
        for shape in (L.WIDE, L.ELEM):
            for _, a, b in L.add_cases(dtype, shape):
                got = wrong(a, b, dtype)
                n += int(not np.array_equal(L.canon_nan(got, dtype), L.canon_nan(L.add_torch(a, b, dtype), dtype)))
        print("%s, %s: %d cases give other bits" % (name, dtype, n))
        assert n > 0, (name, dtype)
