"""The planner's graph decisions on the CPU (not ``gpu``): tests/plan_interp.py runs ``build_plan``'s ops literally on a byte
arena and compares every block, bit for bit, with a forward by block index that knows nothing of the planner.

* tests/golden/cfg/graph_*.cfg, batch 2: every cfg in both interpreter modes, at both element sizes, with and without arena
  reuse; per cfg, the plan properties its comments promise (``DECISIONS``), so that a planner change which makes a case vacuous
  fails by name.
* The shipped tiny networks at 64 x 64.
* The refusals of ``plan.check_head_readers`` and their messages; with the refusal bypassed the interpreter fails on each of
  those graphs, which is what shows that it finds the class.

Rounding points at es=2 (fp16 storage on the CPU): the reference's (``Restatement.rounding_points``: every block but a head
conv and a conv whose only reader is the shortcut after it) are the plan's at every block of these cfgs -- a shortcut the plan
does not fuse is rounded twice on both sides, because the reference counts readers as the planner does -- so every block is
compared in free run, none teacher-forced.
"""
import os

import pytest

from oracle import darknet_oracle as orc
from yolov3 import plan as P
from yolov3.plan import build_plan

import plan_interp as PI
from golden_util import MODELS

MODES = ("literal", "as_fused")


def _plan(case, es, reuse, batch=PI.BATCH, height=PI.HEIGHT, width=PI.WIDTH):
    return build_plan(case["blocks"], case["net_info"], batch, height, width, es, reuse=reuse, fuse=True)


_refs = {}


def _want(name, es):
    """the reference of one graph cfg at one element size, computed once and left unchanged"""
    if (name, es) not in _refs:
        case = PI.graph_case(name)
        _refs[name, es] = PI.reference_blocks(case["path"], case["params"], case["x"], PI.EMULATE[es])
    return _refs[name, es]


# ---------------------------------------------------------------------------------------------------------------------------
# the decision table: cfg -> [(decision, predicate on the plan)]
# ---------------------------------------------------------------------------------------------------------------------------

def _ops(plan, kind, block=None):
    return [o for o in plan["ops"] if o["kind"] == kind and (block is None or o["block"] == block)]


def _one(plan, kind, block):
    ops = _ops(plan, kind, block)
    assert len(ops) == 1, (kind, block, ops)
    return ops[0]


def _no_op(plan, block):
    return not [o for o in plan["ops"] if o["block"] == block]


def _producer(plan, tensor):
    """the op that writes exactly this channel slice"""
    hits = [o for o in plan["ops"] if o.get("out") is not None and (o["out"].buf, o["out"].off, o["out"].c) ==
            (tensor.buf, tensor.off, tensor.c)]
    assert len(hits) == 1, (tensor, hits)
    return hits[0]


def _same(a, b):
    return (a.buf, a.off, a.ld, a.c) == (b.buf, b.off, b.ld, b.c)


def _placed(plan, block, cat, off):
    """block's producer writes straight into channel ``off`` of the concat buffer of route block ``cat``"""
    t = plan["tensor_of"][block]
    return t.buf == "cat%d" % cat and t.off == off and t.ld == plan["tensor_of"][cat].ld and _producer(plan, t)["kind"] != "copy"


def _copies(plan, route):
    return [(o["inp"].buf, o["inp"].off, o["out"].off) for o in _ops(plan, "copy", route)]


DECISIONS = {
    "graph_shortcuts": [
        ("shortcut behind a maxpool gives an add",
         lambda p: _same(_one(p, "add", 3)["inp"], _one(p, "maxpool", 2)["out"]) and _one(p, "add", 3)["res"].buf == "t1"),
        ("shortcut behind a single-source route gives an add",
         lambda p: _no_op(p, 4) and _one(p, "add", 5)["inp"] is _one(p, "add", 3)["out"] and _one(p, "add", 5)["res"].buf == "t1"),
        ("shortcut behind a conv with a second reader gives an unfused add",
         lambda p: _one(p, "conv", 6)["res"] is None and _one(p, "add", 7)["inp"] is _one(p, "conv", 6)["out"]),
        ("from=-1 gives an add with inp and res the same tensor",
         lambda p: _one(p, "add", 8)["inp"] is _one(p, "add", 8)["res"] is _one(p, "add", 7)["out"]),
        ("an add whose output is placed in a concat",
         lambda p: _one(p, "add", 8)["out"].buf == "cat9" and _placed(p, 8, 9, 0) and _placed(p, 6, 9, 64) and not _copies(p, 9)),
        ("a shortcut of a shortcut",
         lambda p: _one(p, "add", 7)["res"] is _one(p, "add", 5)["out"] and
         _one(p, "conv", 13)["res"] is _one(p, "conv", 11)["out"] and _one(p, "conv", 11)["res"] is _one(p, "conv", 10)["out"]
         and not _ops(p, "add", 12) and not _ops(p, "add", 14)),
        ("fuse_next on the stem only: the shortcuts of blocks 7 and 12 read convs 6 and 10 as well",
         lambda p: _one(p, "conv", 0)["fuse_next"] and not _one(p, "conv", 10)["fuse_next"] and not _one(p, "conv", 6)["fuse_next"]),
    ],
    "graph_concat": [
        ("fused shortcut whose res is a slice of a concat buffer",
         lambda p: (lambda o: o["res"].buf == "cat3" and o["res"].off == 32 and o["res"].ld == 64 and
                    o["res"].ld != o["out"].ld and o["res"].off > 0)(_one(p, "conv", 5))),
        ("grouped route of a concat buffer, on the grain: an alias and no op",
         lambda p: _no_op(p, 7) and (lambda t: (t.buf, t.off, t.ld, t.c) == ("cat3", 32, 64, 32))(p["tensor_of"][7])),
        ("fused shortcut whose res is a grouped-route alias",
         lambda p: _one(p, "conv", 8)["res"] is p["tensor_of"][7] and _one(p, "conv", 8)["inp"] is p["tensor_of"][7]),
        ("fused shortcuts whose output is placed in a concat",
         lambda p: _one(p, "conv", 8)["out"].buf == "cat10" and _one(p, "conv", 8)["out"].off == 0 and
         _one(p, "conv", 5)["out"].buf == "cat10" and _one(p, "conv", 5)["out"].off == 32 and _one(p, "conv", 5)["out"].ld == 96
         and _placed(p, 4, 10, 64) and not _copies(p, 10)),
        ("grouped route on the grain gives an alias and no op",
         lambda p: _no_op(p, 12) and (lambda t: (t.buf, t.off, t.ld, t.c) == ("t11", 0, 64, 32))(p["tensor_of"][12])),
        ("grouped route off the grain gives a copy from a slice",
         lambda p: (lambda o: (o["inp"].buf, o["inp"].off, o["inp"].ld, o["inp"].c, o["out"].buf, o["out"].ld) ==
                    ("t13", 20, 40, 20, "t14", 24))(_one(p, "copy", 14)) and
         (lambda o: (o["inp"].buf, o["inp"].off, o["inp"].c, o["out"].buf) == ("t13", 0, 20, "t15"))(_one(p, "copy", 15))),
        ("a member at a channel offset off the 8-element grain gives a copy",
         lambda p: _copies(p, 16) == [("t14", 0, 0), ("t13", 0, 20), ("t15", 0, 60)] and p["tensor_of"][13].buf == "t13"),
    ],
    "graph_routes": [
        ("both members of a plain concat are placed",
         lambda p: _placed(p, 2, 3, 0) and _placed(p, 1, 3, 32) and not _copies(p, 3)),
        ("one block named twice gives one placement and one copy; a member placed in an earlier concat gives a copy",
         lambda p: _placed(p, 4, 5, 0) and _copies(p, 5) == [("cat5", 0, 32), ("cat3", 0, 64)]),
        ("a member that is itself a multi-source route gives a copy",
         lambda p: _copies(p, 7) == [("cat3", 0, 0)] and _one(p, "copy", 7)["inp"].c == 64 and _placed(p, 6, 7, 64)),
        ("a member reached through two single-source routes is resolved and placed",
         lambda p: _placed(p, 8, 19, 0) and p["tensor_of"][10] is p["tensor_of"][9] is p["tensor_of"][8]),
        ("a maxpool, a reorg3d and an upsample placed as members",
         lambda p: _placed(p, 12, 19, 32) and _placed(p, 15, 19, 64) and _placed(p, 18, 19, 128) and not _copies(p, 19) and
         _one(p, "reorg", 15).get("form3d") is True and _one(p, "maxpool", 12)["out"].ld == 144),
        ("a route to block 0",
         lambda p: _no_op(p, 13) and p["tensor_of"][13] is p["tensor_of"][0] and _one(p, "maxpool", 14)["inp"] is p["tensor_of"][0]),
        ("two heads, one on 64 and one on 32 channels",
         lambda p: len(_ops(p, "yolo")) == 2 and _one(p, "conv", 21)["inp"].c == 64 and _one(p, "conv", 24)["inp"].c == 32 and _one(p, "conv", 24)["inp"].ld == 96),
    ],
    "graph_pools": [
        ("pools 13 / 9 / 5 read one tensor, in that order",
         lambda p: [o["ksize"] for o in p["ops"][2:5]] == [13, 9, 5] and all(o["kind"] == "maxpool" and
                                                                           _same(o["inp"], p["ops"][2]["inp"]) for o in p["ops"][2:5])
         and p["ops"][2]["inp"].c == 32),
        ("pools 5 / 9 / 9 read one tensor",
         lambda p: [_one(p, "maxpool", b)["ksize"] for b in (9, 11, 13)] == [5, 9, 9] and
         all(_same(_one(p, "maxpool", b)["inp"], p["tensor_of"][8]) for b in (9, 11, 13))),
        ("a cascade 5 -> 5 -> 5, each pool reading the previous one",
         lambda p: _one(p, "maxpool", 17)["inp"] is _one(p, "maxpool", 16)["out"] and
         _one(p, "maxpool", 18)["inp"] is _one(p, "maxpool", 17)["out"]),
        ("a 5 / 9 / 13 pyramid on 24 channels",
         lambda p: [_one(p, "maxpool", b)["ksize"] for b in (21, 23, 25)] == [5, 9, 13] and
         all(_same(_one(p, "maxpool", b)["inp"], p["tensor_of"][20]) and _one(p, "maxpool", b)["inp"].c == 24 for b in (21, 23, 25))),
        ("a 64 -> 32 1x1 and 32 -> 64 3x3 with the shortcut from a tensor that is not the pair's input",
         lambda p: _one(p, "conv", 33)["fuse_next"] and _one(p, "conv", 34)["res"] is p["tensor_of"][31] and
         _one(p, "conv", 33)["inp"] is p["tensor_of"][32] and p["tensor_of"][31] is not p["tensor_of"][32]),
        ("the same pair with the shortcut from its input",
         lambda p: _one(p, "conv", 37)["fuse_next"] and _one(p, "conv", 38)["res"] is _one(p, "conv", 37)["inp"] is p["tensor_of"][32]),
        ("the same pair where the 1x1 has a second reader: fuse_next is false and the plan has two ops",
         lambda p: not _one(p, "conv", 41)["fuse_next"] and _one(p, "conv", 42)["res"] is _one(p, "conv", 41)["inp"] and
         _placed(p, 41, 44, 0) and _one(p, "conv", 42)["out"].buf == "cat44"),
        ("three fused shortcuts written into one concat",
         lambda p: [(_one(p, "conv", b)["out"].buf, _one(p, "conv", b)["out"].off) for b in (42, 38, 34)] ==
         [("cat44", 32), ("cat44", 96), ("cat44", 160)] and not _copies(p, 44)),
    ],
    "graph_heads": [
        ("a route and a max-pool read a head conv's float32 logits",
         lambda p: _one(p, "maxpool", 5)["inp"] is _one(p, "conv", 2)["out"] and _one(p, "conv", 2)["out"].buf == "t2"),
        ("a [yolo] behind a max-pool and one behind a shortcut",
         lambda p: _one(p, "yolo", 6)["inp"] is _one(p, "maxpool", 5)["out"] and _one(p, "yolo", 10)["inp"] is _one(p, "conv", 8)["out"]),
        ("a fused shortcut whose from names a head conv",
         lambda p: _one(p, "conv", 8)["res"] is _one(p, "conv", 2)["out"]),
    ],
}


def _element_sizes(name):
    return (4,) if name in PI.F32_ONLY else (4, 2)


@pytest.mark.parametrize("name", PI.GRAPH_CFGS)
def test_graph_cfg_reaches_its_decisions(name):
    case = PI.graph_case(name)
    for es in _element_sizes(name):
        for reuse in (False, True):
            plan = _plan(case, es, reuse)
            for what, holds in DECISIONS[name]:
                assert holds(plan), "%s (es=%d, reuse=%s): %s" % (name, es, reuse, what)
    kinds = [o["kind"] for o in _plan(case, 4, True)["ops"]]
    print(name, {k: kinds.count(k) for k in sorted(set(kinds))})


def test_the_graph_cfgs_hold_what_the_shipped_plans_lack():
    kinds = []
    for name in PI.GRAPH_CFGS:
        kinds += [o["kind"] for o in _plan(PI.graph_case(name), 4, True)["ops"]]
    assert kinds.count("add") == 4 and kinds.count("copy") == 8 and kinds.count("reorg") == 1 and kinds.count("upsample") == 1


@pytest.mark.parametrize("name", PI.GRAPH_CFGS)
def test_reference_by_block_is_the_oracle_forward(name):
    """``reference_blocks`` against ``OracleDarknet.forward(collect=...)`` where the oracle can walk the cfg: the same bits"""
    case = PI.graph_case(name)
    if not PI.plain_oracle_can_walk(case["path"]):
        assert name in ("graph_concat", "graph_routes")       # grouped routes, [reorg3d]
        return
    for es in _element_sizes(name):
        got = {}
        orc.OracleDarknet(case["path"]).set_params(case["params"]).forward(case["x"], collect=got, emulate=PI.EMULATE[es])
        want = _want(name, es)
        assert sorted(got) == sorted(want)
        for i in got:
            assert PI.bit_equal(got[i], want[i]), (name, es, i)


@pytest.mark.parametrize("reuse", [False, True])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", PI.GRAPH_CFGS)
def test_graph_cfg_through_the_interpreter(name, mode, reuse):
    case = PI.graph_case(name)
    for es in _element_sizes(name):
        n = PI.check_plan(case, _plan(case, es, reuse), es, mode, _want(name, es))
        assert n >= len(case["blocks"]) - 6


@pytest.mark.parametrize("model,size", [("yolov3-tiny", 64), ("yolov4-tiny", 64), ("yolov2-tiny", 64)])
def test_shipped_tiny_cfgs_through_the_interpreter(model, size):
    case = PI.synth_case(os.path.join(os.path.dirname(MODELS["yolov3-tiny"]), model + ".cfg"), size, size, batch=1)
    for es in (4, 2):
        want = PI.reference_blocks(case["path"], case["params"], case["x"], PI.EMULATE[es])
        for mode in MODES:
            PI.check_plan(case, _plan(case, es, True, 1, size, size), es, mode, want)


# ---------------------------------------------------------------------------------------------------------------------------
# the refusals
# ---------------------------------------------------------------------------------------------------------------------------

NET = "[net]\nwidth=48\nheight=32\nchannels=3\n"
CONV = "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=leaky\n"
HEAD = "[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n"
YOLO = "[yolo]\nmask=0,1,2\nanchors=6,8, 12,10, 20,24\nclasses=1\nnum=3\n"
TAIL = CONV % (32, 1) + HEAD + YOLO
REGION = ("[convolutional]\nfilters=30\nsize=1\nstride=1\npad=1\nactivation=linear\n"
          "[region]\nanchors=1,1, 2,2, 3,3, 4,4, 5,5\nclasses=1\ncoords=4\nnum=5\nsoftmax=1\n")

# name -> (cfg text, element sizes that refuse it, words of the message)
REFUSED = {
    "maxpool behind a route to the yolo": (
        NET + CONV % (32, 3) + HEAD + YOLO + "[route]\nlayers=-1\n[maxpool]\nsize=2\nstride=1\n" + YOLO,
        (4, 2), ("yolo block 2", "block 3 (route)", "activated output")),
    "conv straight after the yolo": (
        NET + CONV % (32, 3) + HEAD + YOLO + TAIL, (4, 2), ("yolo block 2", "block 3 (convolutional)")),
    "shortcut from the yolo": (
        NET + CONV % (32, 3) + HEAD + YOLO + "[route]\nlayers=0\n" + HEAD + "[shortcut]\nfrom=-3\nactivation=linear\n" + YOLO,
        (4, 2), ("yolo block 2", "block 5 (shortcut)")),
    "route to the region": (
        NET + CONV % (32, 3) + REGION + "[route]\nlayers=-1\n" + REGION, (4, 2), ("region block 2", "block 3 (route)")),
    "route to the head conv": (
        NET + CONV % (32, 3) + HEAD + YOLO + "[route]\nlayers=-2\n" + TAIL,
        (2,), ("conv block 1", "block 3 (route)", "yolo block 2", "float32")),
    "shortcut from the head conv": (
        NET + CONV % (32, 3) + HEAD + YOLO + "[route]\nlayers=0\n" + CONV % (18, 1) + "[shortcut]\nfrom=-4\nactivation=linear\n" +
        TAIL, (2,), ("conv block 1", "block 5 (shortcut)", "yolo block 2")),
    "route to a region's head conv": (
        NET + CONV % (32, 3) + REGION + "[route]\nlayers=-2\n" + REGION, (2,), ("conv block 1", "block 3 (route)", "region block 2")),
    "yolo behind a maxpool": (
        NET + CONV % (32, 3) + HEAD + "[maxpool]\nsize=2\nstride=1\n" + YOLO, (2,), ("yolo block 3", "block 2", "[maxpool]", "not a conv")),
    "yolo behind a route": (
        NET + HEAD + CONV % (32, 3) + "[route]\nlayers=0\n" + YOLO, (2,), ("yolo block 3", "block 2", "[route]")),
    "yolo behind a shortcut": (
        NET + HEAD + HEAD + "[shortcut]\nfrom=-2\nactivation=linear\n" + YOLO, (2,), ("yolo block 3", "block 2", "[shortcut]")),
}


def _text_case(tmp_path, text, height=PI.HEIGHT, width=PI.WIDTH):
    path = tmp_path / "refused.cfg"
    path.write_text(text)
    return PI.synth_case(str(path), height, width)


@pytest.mark.parametrize("what", sorted(REFUSED))
def test_head_readers_are_refused_by_name(tmp_path, what):
    text, refused_es, words = REFUSED[what]
    case = _text_case(tmp_path, text)
    for es in (4, 2):
        if es in refused_es:
            with pytest.raises(ValueError) as err:
                _plan(case, es, True)
            for word in words:
                assert word in str(err.value), (what, word, str(err.value))
        else:
            # float32 keeps running these graphs, and the plan computes them: literally and as the executor runs it
            for mode in MODES:
                for reuse in (False, True):
                    PI.check_plan(case, _plan(case, es, reuse), es, mode)


def test_graph_heads_cfg_is_refused_in_16_bit_and_names_the_block():
    case = PI.graph_case("graph_heads")
    with pytest.raises(ValueError, match=r"conv block 2: block 4 \(route\) reads the logits of the head conv of yolo block 3"):
        _plan(case, 2, True)


@pytest.mark.parametrize("what", sorted(REFUSED) + ["graph_heads"])
def test_interpreter_fails_where_the_refusal_is_bypassed(tmp_path, monkeypatch, what):
    """Without ``check_head_readers`` every refused graph must fail in the interpreter's ``as_fused`` mode at the element size
    that refuses it.  A reader of a [yolo] block's output gets, at es=4, the raw logits the planner aliases it to; the reference
    by block index hands it the same (neither computes Darknet's activated tensor), so those four are shown at es=2 only."""
    if what == "graph_heads":
        case, refused_es = PI.graph_case(what), (2,)
    else:
        case, refused_es = _text_case(tmp_path, REFUSED[what][0]), REFUSED[what][1]
    monkeypatch.setattr(P, "check_head_readers", lambda *a, **k: None)
    for reuse in (False, True):
        with pytest.raises(PI.PlanError):
            PI.check_plan(case, _plan(case, 2, reuse), 2, "as_fused")
    assert 2 in refused_es


def test_fallback_graph_op_by_op_and_through_the_interpreter(tmp_path):
    """the graph of tests/test_host_logic.py::test_plan_fallbacks_for_unfusable_graphs, which asserts that the words ``add`` and
    ``copy`` appear: here op by op, and through the interpreter"""
    case = _text_case(tmp_path, (
        "[net]\nwidth=32\nheight=32\nchannels=3\n" + CONV % (8, 3) + CONV % (8, 3) +
        "[shortcut]\nfrom=-2\nactivation=linear\n"
        "[route]\nlayers=-2,-1\n"            # conv 1 has a second reader -> shortcut cannot be fused
        "[route]\nlayers=-1,-3\n"            # block 1 already placed in the first concat -> copy
        "[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n"
        "[yolo]\nmask=0\nanchors=10,14\nclasses=13\nnum=1\n"), 32, 32)
    plan = build_plan(case["blocks"], case["net_info"], 1, 32, 32, 4)
    assert [(o["kind"], o["block"]) for o in plan["ops"]] == [
        ("conv", 0), ("conv", 1), ("add", 2), ("copy", 4), ("copy", 4), ("conv", 5), ("yolo", 6)]
    assert _one(plan, "conv", 1)["res"] is None and _one(plan, "conv", 1)["out"].buf == "cat3"
    assert _one(plan, "add", 2)["out"].buf == "cat3" and _one(plan, "add", 2)["out"].off == 8
    assert _copies(plan, 4) == [("cat3", 0, 0), ("cat3", 0, 16)]
    assert P.infer_shapes(case["blocks"], case["net_info"], 32, 32)[4] == (24, 32, 32)
    for es in (4, 2):
        for mode in MODES:
            for reuse in (False, True):
                PI.check_plan(case, build_plan(case["blocks"], case["net_info"], PI.BATCH, 32, 32, es, reuse=reuse, fuse=True), es, mode)
