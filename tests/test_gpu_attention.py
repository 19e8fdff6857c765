"""The attention kernels one op at a time (-m gpu): avgpool_<dtype>, scale_channels_<dtype> and sam_<dtype> (csrc/attention.hip)
through the C ABI, in float32, bf16 and fp16, every result compared bit for bit (NaN as NaN-ness) with the statement of
include/yolov3_hip.h.  Every operand is a channel slice of a wider NaN-poisoned body between guards (tests/attention_util.py on
tests/footprint_util.py's layout), so each run is a footprint case as well: nothing outside the output slice may change."""
import numpy as np
import pytest
import torch

from yolov3 import _hip

import attention_util as AU
import kernel_census as census
import layer_patterns as L

pytestmark = pytest.mark.gpu

P_EDGES = (31, 32, 33, 63, 64, 65, 127, 128, 129)      # around the 32 partial sums, two rows of them, and the loop's unroll of 4 rows
# (batch, h, w, channels): maps 1x1, 1x5, 5x1, 13x10, 19x19, 76x76; batches 1, 3, 37; several workgroups per frame (1280 channels)
VEC_SHAPES = [(1, 1, 1, 8), (3, 1, 5, 24), (37, 5, 1, 8), (3, 13, 10, 256), (1, 19, 19, 1280), (3, 76, 76, 24), (37, 13, 10, 24)]
ELEM_SHAPES = [(1, 1, 1, 7), (3, 1, 5, 12), (37, 5, 1, 20), (3, 13, 10, 7), (1, 19, 19, 20), (1, 76, 76, 12), (3, 13, 10, 24)]
SHAPES = {"vec": VEC_SHAPES + [(2, 1, p, 24) for p in P_EDGES], "elem": ELEM_SHAPES + [(2, 1, p, 7) for p in P_EDGES]}


def _finish(failures):
    if failures:
        print("\n".join(failures))
    assert not failures, "%d cases differ; the first: %s" % (len(failures), failures[0])


def _report(what, got, want, ok):
    bad = np.argwhere(~ok)
    first = tuple(bad[0])
    return "%s: %d of %d differ, first at %s got %r (0x%08X) want %r (0x%08X)" % (
        what, len(bad), ok.size, first, float(got[first]), int(np.float32(got[first]).view(np.uint32)),
        float(want[first]), int(np.float32(want[first]).view(np.uint32)))


def _check(failures, what, got, want):
    ok = AU.same_bits(got, want)
    if not ok.all():
        failures.append(_report(what, got, want, ok))


# ---- avgpool ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["vec", "elem"])
@pytest.mark.parametrize("dtype", AU.DTYPES)
def test_avgpool_sums_in_the_stated_order_divides_and_rounds_once(dtype, form):
    """(a) random inputs: the ordered float32 restatement, bit for bit; (b) integer-valued inputs whose sums stay below 2^24:
    round(S / float32(P)) from an int64 sum, bit for bit -- exact in any order, so it pins the division and the rounding apart
    from the order; (c) the random inputs against the float64 mean inside the derived gate (attention_util.avgpool_gate)."""
    failures = []
    for n, shape in enumerate(SHAPES[form]):
        b, h, w, c = shape
        what = "avgpool %s %s %s" % (dtype, form, shape)
        x = AU.random_storage(shape, dtype, n)
        r = AU.run_op("avgpool", dtype, x, form=form)
        assert r["kernel"] == "avgpool_" + AU.TAG[dtype] and len(r["symbols"][0]) == 1, what
        assert AU.symbol_matches(r["symbols"][0][0], "avgpool", form, dtype), (what, r["symbols"])
        vec = AU.vec_of(dtype) if form == "vec" else 1
        assert r["dims"] == (b * -(-(c // vec) // 8), 256, 0), (what, r["dims"])
        _check(failures, what + " (a) ordered", r["out"], AU.avgpool_ordered_expected(x, dtype))
        mean = x.astype(np.float64).reshape(b, h * w, c).mean(axis=1).reshape(b, 1, 1, c)
        gap = np.abs(r["out"].astype(np.float64) - mean)
        gate = AU.avgpool_gate(x, dtype)
        if not (gap <= gate).all():
            failures.append("%s (c): off the float64 mean by up to %.3g x the gate" % (what, float((gap / gate).max())))
        ints = AU.integer_storage(shape, dtype, n)
        assert np.abs(ints).astype(np.int64).reshape(b, h * w, c).sum(axis=1).max() < 2 ** 24          # every partial sum is exact
        s = ints.astype(np.int64).reshape(b, h * w, c).sum(axis=1)
        want = AU.to_storage(s.astype(np.float32) / np.float32(h * w), dtype).reshape(b, 1, 1, c)
        _check(failures, what + " (b) integers", AU.run_op("avgpool", dtype, ints, form=form)["out"], want)
    _finish(failures)


# ---- scale_channels and sam ------------------------------------------------------------------------------------------------

def _pattern_cases(kind, dtype, form):
    """[(name, src, prev)] float32 arrays: in the 16-bit modes every ordered pattern against each second operand of
    layer_patterns.SECOND (zeros of both signs, subnormals, ties, +-65504 and the largest bf16 -- products that overflow fp16 --,
    infinities, NaN), as layer_patterns builds them for add; in float32 the planted list against itself, every pair.  For
    scale_channels the second operand is per frame and channel, so one more case pairs every pattern as the SCALE with a few sources."""
    shape = L.WIDE if form == "vec" else L.ELEM
    cases = []
    if kind == "sam" or L.bits(dtype) == 16:
        for name, a, second in L.add_cases(dtype, shape):
            src, prev = L.to_float(a, dtype).reshape(shape), L.to_float(second, dtype).reshape(shape)
            if kind == "scale_channels":
                prev = np.ascontiguousarray(prev[:, 7:8, 5:6, :])
            cases.append((name, src, prev))
    if kind == "scale_channels":
        c = shape[3]
        if L.bits(dtype) == 16:
            pats = L.ordered(dtype)
        else:
            pats = L.planted_f32()
        nb = -(-pats.size // c)
        prev = L.to_float(L.lay(pats, (nb, 1, 1, c)), dtype).reshape(nb, 1, 1, c)
        few = L.to_float(L.lay(pats[:: max(1, pats.size // 61)], (nb, 2, 3, c)), dtype).reshape(nb, 2, 3, c)
        cases.append(("every pattern as the scale", few, prev))
        if L.bits(dtype) == 32:
            # planted x planted: frame b holds scale planted[b] in every channel, its pixels the whole planted list
            n = pats.size
            px = -(-n // c)
            src = np.broadcast_to(L.to_float(L.lay(pats, (1, 1, px, c)), dtype).reshape(1, 1, px, c), (n, 1, px, c))
            prev = np.repeat(L.to_float(pats, dtype).reshape(n, 1, 1, 1), c, axis=3)
            cases.append(("planted x planted", np.ascontiguousarray(src), np.ascontiguousarray(prev)))
    return cases


@pytest.mark.parametrize("form", ["vec", "elem"])
@pytest.mark.parametrize("dtype", AU.DTYPES)
@pytest.mark.parametrize("kind", ["scale_channels", "sam"])
def test_products_round_the_exact_product_once(kind, dtype, form):
    failures = []
    for name, src, prev in _pattern_cases(kind, dtype, form):
        what = "%s %s %s, %s" % (kind, dtype, form, name)
        r = AU.run_op(kind, dtype, prev, src, form=form)
        assert r["kernel"] == "%s_%s" % (kind, AU.TAG[dtype]) and len(r["symbols"][0]) == 1, what
        assert AU.symbol_matches(r["symbols"][0][0], kind, form, dtype), (what, r["symbols"])
        _check(failures, what, r["out"], AU.product_expected(src, prev, dtype))
    _finish(failures)


@pytest.mark.parametrize("form", ["vec", "elem"])
@pytest.mark.parametrize("dtype", AU.DTYPES)
@pytest.mark.parametrize("kind", ["scale_channels", "sam"])
def test_products_on_every_shape_and_inside_one_buffer(kind, dtype, form):
    """the maps, batches and channel counts of the avgpool cases; then ``src`` and the output as two channel slices of ONE body"""
    failures = []
    shapes = VEC_SHAPES if form == "vec" else ELEM_SHAPES
    for n, shape in enumerate(shapes):
        b, h, w, c = shape
        src = AU.random_storage(shape, dtype, 40 + n)
        prev = AU.random_storage((b, 1, 1, c) if kind == "scale_channels" else shape, dtype, 80 + n)
        want = AU.product_expected(src, prev, dtype)
        for same in ((False, True) if n % 3 == 0 else (False,)):
            r = AU.run_op(kind, dtype, prev, src, form=form, same_buffer=same)
            vec = AU.vec_of(dtype) if form == "vec" else 1
            assert r["dims"] == (-(-b * h * w * (c // vec) // 256), 256, 0), (shape, r["dims"])
            _check(failures, "%s %s %s %s%s" % (kind, dtype, form, shape, " in one buffer" if same else ""), r["out"], want)
    _finish(failures)


# ---- equality of code paths --------------------------------------------------------------------------------------------------

def _operands(kind, dtype, shape=(3, 13, 10, 24)):
    b, _, _, c = shape
    x = AU.random_storage(shape, dtype, 5)
    if kind == "avgpool":
        return x, None
    return AU.random_storage((b, 1, 1, c) if kind == "scale_channels" else shape, dtype, 6), x


@pytest.mark.parametrize("dtype", AU.DTYPES)
@pytest.mark.parametrize("kind", AU.KINDS)
def test_forms_cu_counts_and_graph_replay_give_the_same_bits(kind, dtype):
    prev, src = _operands(kind, dtype)
    base = AU.run_op(kind, dtype, prev, src, form="vec")
    elem = AU.run_op(kind, dtype, prev, src, form="elem")
    assert AU.symbol_matches(base["symbols"][0][0], kind, "vec", dtype) and AU.symbol_matches(elem["symbols"][0][0], kind, "elem", dtype)
    assert AU.same_bits(base["out"], elem["out"]).all(), "the 16-byte and the element form differ"
    for n in (1, 32, 256):
        with _hip.device_cus(n):
            r = AU.run_op(kind, dtype, prev, src, form="vec")
        assert r["dims"] == base["dims"] and r["symbols"] == base["symbols"], n
        assert AU.same_bits(r["out"], base["out"]).all(), "device_cus %d" % n
    # use_graph on a side stream: eager, then captured and launched, then replayed; the output slice is NaN again before each run,
    # so what is compared is what the replay wrote
    g = AU.run_op(kind, dtype, prev, src, form="vec", options={"use_graph": 1}, stream=torch.cuda.Stream(), runs=3)
    assert g["symbols"] == base["symbols"], g["symbols"]
    assert AU.same_bits(g["out"], base["out"]).all(), "graph replay"


# ---- footprint and census ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", AU.CENSUS_KEYS)
def test_every_compiled_instance_is_launched_where_the_census_says(key):
    """one case per compiled instance of libyolov3_hip_attn.so on the strided, poisoned, guarded layout: right values, nothing
    written outside the output slice, and the launch log names exactly the symbol tests/golden/kernel_instances_attn.json records"""
    census.assert_census(key, library="attn", launched=[AU.run_census_case(key)])
