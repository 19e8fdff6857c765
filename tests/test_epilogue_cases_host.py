"""The planted epilogue cases (tests/epilogue_cases.py) checked on the CPU: the two bit-level storage roundings against the
oracle's, every tag true, the expected-value functions against torch, the condition on the either-side rule, and the
channel layout of tests/test_gpu_epilogue.py."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import darknet_oracle as orc

import epilogue_cases as E
from test_gpu_yolov4_families import FAMILY_CFG, FAMILY_RUNS

ORC = {"bf16": orc.bf16_round, "fp16": orc.f16_round}
CHANNELS = [int(m) for m in re.findall(r"filters=(\d+)", FAMILY_CFG)]      # of conv blocks 0-4, 6-8, 10-12
CONV_BLOCKS = [0, 1, 2, 3, 4, 6, 7, 8, 10, 11]
CH = dict(zip(CONV_BLOCKS, CHANNELS))


def _same(a, b):
    a, b = E.f32(a), E.f32(b)
    return (E.bits(a) == E.bits(b)) | (np.isnan(a) & np.isnan(b))


def _all_values():
    return np.asarray(sorted(set(float(c.t) for act in E.ACTS for c in E.cases(act) if not np.isnan(c.t))) + [np.nan],
                      dtype=np.float32)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_bit_level_rounding_against_oracle(dtype):
    mine, theirs = E.RND[dtype], ORC[dtype]
    rng = np.random.RandomState(11)
    x = np.concatenate([_all_values(), E.from_bits(rng.randint(0, 1 << 32, 1000000, dtype=np.uint64).astype(np.uint32))])
    assert _same(mine(x), theirs(torch.from_numpy(x)).numpy()).all()
    # every 16-bit pattern widened and narrowed again is itself
    p = np.arange(65536, dtype=np.uint32)
    wide = E.from_bits(p << 16) if dtype == "bf16" else p.astype(np.uint16).view(np.float16).astype(np.float32)
    assert _same(mine(wide), wide).all()
    assert _same(theirs(torch.from_numpy(wide)).numpy(), wide).all()


def _result(act, c):
    return E.act_exact(act, c.t)


@pytest.mark.parametrize("act", ["linear", "leaky"])
def test_tags_are_true(act):
    cs = E.cases(act)
    by_tag = {c.tag: c for c in cs}
    assert len(by_tag) == len(cs) <= E.LIST_LEN
    n_tie = 0
    for c in cs:
        dtype = "bf16" if "bf16" in c.tag else ("fp16" if "fp16" in c.tag else None)
        if c.kind != "tie" or (act == "leaky" and c.t < 0 and not c.tag.startswith("leaky")):
            continue                  # (a common negative tie is a tie of the linear result; leaky has ties of its own)
        n_tie += 1
        res = _result(act, c)
        assert E.is_tie(dtype, res), c
        rnd = E.RND[dtype]
        # halfway in float64 between the storage values its float32 neighbours round to, which differ
        below, above = rnd(E.step(res, -1)), rnd(E.step(res, 1))
        assert below != above and (float(res) == (float(below) + float(above)) / 2 or np.isinf(above)), c
        assert rnd(res) in (below, above)
        if "even below" in c.tag or "to 0" in c.tag:
            assert rnd(res) == (below if res > 0 else above), c
        if "odd below" in c.tag or "to inf" in c.tag or "to 2^-14" in c.tag or "above max" in c.tag:
            assert rnd(res) == (above if res > 0 else below), c
        if c.tag + " -1 step" in by_tag:
            lo, hi = by_tag[c.tag + " -1 step"], by_tag[c.tag + " +1 step"]
            assert lo.t == E.step(c.t, -1) and hi.t == E.step(c.t, 1)
            assert rnd(_result(act, lo)) != rnd(_result(act, hi)), c      # the neighbours round apart
    assert n_tie == (10 if act == "linear" else 13)
    # the named storage results
    f16, b16 = E.rne_f16, E.rne_bf16
    t = {k: by_tag[k].t for k in by_tag}
    assert f16(t["fp16 max 65504"]) == 65504 and f16(t["fp16 overflow: largest float32 below 65520"]) == 65504
    assert t["fp16 overflow: largest float32 below 65520"] < 65520 and np.isinf(f16(t["fp16 overflow: 65520 (tie, to inf)"]))
    assert f16(t["fp16 subnormal 2^-24"]) == 2.0 ** -24 and f16(t["fp16 subnormal tie 2^-25 (to 0)"]) == 0
    assert f16(t["fp16 subnormal: just above 2^-25"]) == 2.0 ** -24 and f16(t["fp16 subnormal tie 3*2^-25 (odd below)"]) == 2.0 ** -23
    assert f16(t["fp16 subnormal tie 1023.5*2^-24 (to 2^-14)"]) == 2.0 ** -14 and f16(t["fp16 -3e-5 (subnormal, negative)"]) != 0
    assert b16(t["bf16 max 3.3895314e38"]) == t["bf16 max 3.3895314e38"] == np.float32(3.3895314e38)
    assert b16(t["bf16 overflow: below the tie above max"]) == t["bf16 max 3.3895314e38"]
    assert np.isinf(b16(t["bf16 overflow: tie above max"])) and np.isinf(b16(t["+FLT_MAX"])) and np.isinf(f16(t["+FLT_MAX"]))
    assert np.isnan(b16(t["NaN"])) and np.isnan(f16(t["NaN"]))
    assert E.bits(t["-0"]) == 0x80000000 and E.bits(t["+smallest subnormal"]) == 1 and t["+FLT_MIN"] == np.finfo(np.float32).tiny


def test_leaky_slope_witnesses_and_max_form():
    cs = {c.tag: c.t for c in E.cases("leaky")}
    for dtype in ("float32", "bf16"):
        t = cs["leaky: float slope 0.1f against a double 0.1, differs after %s rounding" % dtype]
        assert t < 0 and E.RND[dtype](E.leaky_f32(t)) != E.RND[dtype](E.leaky_double_slope(t)), (dtype, t)
    # fp16 has no witness (the search is exhaustive: epilogue_cases.slope_witnesses), and on ordinary data bf16 has none either
    assert E.slope_witnesses("fp16").size == 0
    rng = np.random.RandomState(5)
    x = -np.abs(rng.standard_normal(200000)).astype(np.float32)
    d32 = E.leaky_f32(x) != E.leaky_double_slope(x)
    assert 0.1 < d32.mean() < 0.3 and not (E.rne_bf16(E.leaky_f32(x)) != E.rne_bf16(E.leaky_double_slope(x))).any()
    # max(t, 0.1f t) is the select for every t that is not NaN, signs of zero and infinities included; NaN gives NaN in both
    pat = np.concatenate([np.asarray([c.t for c in E.cases("leaky")], dtype=np.float32),
                          E.from_bits(rng.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32))])
    a, b = E.leaky_f32(pat), E.leaky_max(pat)
    assert (E.bits(a) == E.bits(b))[~np.isnan(pat)].all() and np.isnan(a[np.isnan(pat)]).all() and np.isnan(b[np.isnan(pat)]).all()
    for v in (0.0, -0.0, np.inf, -np.inf):
        assert E.bits(E.leaky_max(v)) == E.bits(E.leaky_f32(v)) == E.bits(F.leaky_relu(torch.tensor(v), 0.1).numpy())


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("act", ["linear", "leaky"])
def test_exact_expectations_against_torch(act, dtype):
    t = np.asarray([c.t for c in E.cases(act)], dtype=np.float32)
    rnd = ORC.get(dtype, lambda v: v)
    a = torch.from_numpy(t) if act == "linear" else F.leaky_relu(torch.from_numpy(t), 0.1)
    lo, hi, nan = E.expect(act, dtype, t)
    assert _same(lo, rnd(a).numpy()).all() and _same(lo, hi).all() and (nan == np.isnan(lo)).all()
    rng = np.random.RandomState(3)
    r = E.RND[dtype]((rng.standard_normal(t.size) * 4).astype(np.float32))
    lo, hi, nan = E.expect(act, dtype, t, r, fused=True)
    assert _same(lo, rnd(a + torch.from_numpy(r)).numpy()).all() and _same(lo, hi).all()
    lo, hi, nan = E.expect(act, dtype, t, r, fused=False)
    assert _same(lo, rnd(rnd(a) + torch.from_numpy(r)).numpy()).all() and _same(lo, hi).all()


@pytest.mark.parametrize("act", ["mish", "logistic"])
def test_float64_functions_against_torch(act):
    t = np.asarray([c.t for c in E.cases(act)], dtype=np.float32)
    fn = F.mish if act == "mish" else torch.sigmoid
    w = E.want64(act, t)
    ref = fn(torch.from_numpy(t).double()).numpy()
    fin = np.isfinite(t)
    assert (np.abs(w[fin] - ref[fin]) <= 1e-12 * np.abs(ref[fin])).all()
    # the non-finite classes, as torch's float32 functions
    ref32 = fn(torch.from_numpy(t)).numpy()
    for dtype in E.DTYPES:
        lo, hi, nan = E.expect(act, dtype, t)
        assert (nan[~fin] == np.isnan(ref32[~fin])).all()
        k = ~fin & ~nan
        assert _same(lo[k], ref32[k]).all() and _same(hi[k], ref32[k]).all()        # mish(inf) = inf; logistic(+-inf) = 1, 0
    assert np.isnan(ref32[np.isneginf(t)]).all() == (act == "mish")                  # mish(-inf) is NaN, as torch's
    # saturated entries are demanded exactly, and the float64 function agrees with the demand within the bound
    sat, val = E.saturated(act, t)
    tags = [c for c in E.cases(act) if c.kind == "sat"]
    assert tags and all(sat[[i for i, c in enumerate(E.cases(act)) if c.kind == "sat"]])
    k = sat & fin
    assert (np.abs(val[k].astype(np.float64) - w[k]) <= E.bound(w[k])).all()
    for dtype in E.DTYPES:
        lo, hi, nan = E.expect(act, dtype, t)
        assert _same(lo[sat], E.RND[dtype](val[sat])).all() and _same(hi[sat], lo[sat]).all()
    # the float32 gate is |got - want64| <= b: torch's own float32 result passes it where the function is tame
    lo, hi, nan = E.expect(act, "float32", t)
    tame = fin & (np.abs(t) < 15)
    assert not E.check(lo, hi, nan, ref32)[tame].any()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("act", ["mish", "logistic"])
def test_either_side_rule_is_mostly_one_value(act, dtype):
    cs = E.cases(act)
    t = np.asarray([c.t for c in cs], dtype=np.float32)
    lo, hi, nan = E.expect(act, dtype, t)
    multi = ~nan & (E.bits(lo) != E.bits(hi))
    assert 4 * int(multi.sum()) <= len(cs), (int(multi.sum()), len(cs), [c.tag for c, m in zip(cs, multi) if m])
    assert (lo[~nan] <= hi[~nan]).all()
    for c, m in zip(cs, multi):
        if c.kind in ("threshold", "sat", "tie"):
            assert not m, c                # exact by the saturation rule, or one allowed storage value
    assert sum(c.kind in ("threshold", "sat") for c in cs) >= (9 if act == "mish" else 7)


def test_required_values_are_planted():
    def has(act, v):
        return any(c.t == np.float32(v) or (np.isnan(v) and np.isnan(c.t)) for c in E.cases(act))
    flt_max, flt_min, sub = np.finfo(np.float32).max, np.finfo(np.float32).tiny, E.from_bits(1)
    for act in E.ACTS:
        for v in (0.0, sub, 1e-40, flt_min, 0.5, 1.0, flt_max, np.inf):
            assert has(act, v) and has(act, -v), (act, v)
        assert has(act, np.nan) and any(E.bits(c.t) == 0x80000000 for c in E.cases(act))
    for v in (20.0, E.step(np.float32(20), 1), E.step(np.float32(20), -1), 30, 43, 44, 44.5, 88, 89, 1e30, E.MISH_MIN, -0.3, -5, -10,
              -17, -20, -50, -87, -88, -90, -103, -104, -200, -1e30):
        assert has("mish", v), v
    m = E.want64("mish", np.asarray([E.step(E.MISH_MIN, -64), E.MISH_MIN, E.step(E.MISH_MIN, 64)], dtype=np.float32))
    assert m[1] < -0.3088 and abs(m[0] - m[1]) < 1e-9 and abs(m[2] - m[1]) < 1e-9        # the minimum, flat to float32
    for v in (16.6, 17, 20, 87, 88.7, 89, 104):
        assert has("logistic", v) and has("logistic", -v), v


def test_channel_layout_covers_every_entry():
    runs = range(len(FAMILY_RUNS))
    for act in E.ACTS:
        n = len(E.cases(act))
        for layer, ch in CH.items():
            seen = [set(E.layer_values(act, run, layer, ch)[1].tolist()) for run in runs]
            if ch >= E.LIST_LEN:
                assert all(s == set(range(n)) for s in seen), (act, layer)
            else:
                assert set().union(*seen) == set(range(n)), (act, layer)
            t, idx = E.layer_values(act, 0, layer, ch)
            assert _same(t, np.asarray([E.cases(act)[i].t for i in idx], dtype=np.float32)).all()
    assert CH[0] == 32 and CH[1] == 64 and min(CH[b] for b in CONV_BLOCKS[2:]) >= E.LIST_LEN
    assert all(CH[a] == CH[b] for a, b in E.RESIDUAL_FROM.items())
    # the layers before the checked one carry nothing that is stored non-finite: an entry is replaced by the filler if and
    # only if its stored result (either end of its allowed interval) is NaN or infinite
    for act in E.ACTS:
        for dtype in E.DTYPES:
            full = E.padded(act)[0]
            lo, hi, nan = E.expect(act, dtype, full)
            bad = nan | ~np.isfinite(lo) | ~np.isfinite(hi)
            t = E.finite_only(act, dtype, full)
            assert (t[bad] == E.FILLER).all() and (E.bits(t[~bad]) == E.bits(full[~bad])).all() and bad.any()
            lo, hi, nan = E.expect(act, dtype, t)
            assert not nan.any() and np.isfinite(lo).all() and np.isfinite(hi).all()


@pytest.mark.parametrize("dtype", E.DTYPES)
@pytest.mark.parametrize("act", ["linear", "leaky"])
def test_shortcut_cases_hold(act, dtype):
    kinds = {}
    for run in range(len(FAMILY_RUNS)):
        for layer in E.RESIDUAL_FROM:
            t, tags, r = E.residual_layer(act, dtype, run, layer, CH[layer])
            assert np.isfinite(r).all() and len(tags) == t.size == CH[layer]
            for tag, tc, rc in zip(tags, t, r):
                assert E.shortcut_tag_holds(tag, act, dtype, tc, rc), (tag, tc, rc)
                kinds[tag] = kinds.get(tag, 0) + 1
            # a witness separates the two orders in the expectation itself
            one, two = E.expect(act, dtype, t, r, fused=True)[0], E.expect(act, dtype, t, r, fused=False)[0]
            w = np.asarray([tag.startswith("shortcut: witness") for tag in tags])
            assert (one[w] != two[w]).all()
    want = set("shortcut: " + k for k in E.SHORTCUT_KINDS)
    if dtype == "float32":          # one rounding only: no two orders, no ties
        want -= {"shortcut: witness", "shortcut: witness negative a", "shortcut: tie"}
    assert want <= set(kinds), (sorted(want - set(kinds)), kinds)
