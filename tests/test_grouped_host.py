"""Grouped and depthwise convs without a GPU: what the cfg reader accepts and refuses, Darknet's stream order for ``groups=``, the
two device weight layouts, [dropout] as an alias, the ``groups`` field of ``y3_op`` and what the library's chooser and plan
creation say about it.  tests/grouped_restate.py is held to ``torch.nn.functional.conv2d(..., groups=G)`` here, and the one-op
cases of tests/test_gpu_grouped.py are shown to fit their gates on the CPU first: the restatement accumulating in float32 against
the same restatement accumulating in float64, on the inputs the GPU test uses.  The ordered float32 restatement the GPU test demands
bit for bit (tests/grouped_ordered.py) is held to the same gates and shown to see the order.  Last, the kernel-level suites'
tables (tests/grouped_suites.py): the lock against the library's census, the rows past 4 GiB and their refusals at the pixel and
launch limits, and the epilogue forms, all on fake addresses."""
import ctypes
import os

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.plan import build_plan
from yolov3.plan_ops import fill_ops, padded_weight_dims

import grouped_cases as GC
import grouped_restate as GR
import kernel_choice_util as kc
from golden_util import GOLDEN, MODELS

CFG = os.path.join(GOLDEN, "cfg", "grouped.cfg")
# block -> (groups, runs on the depthwise kernel) of grouped.cfg
GROUPED_BLOCKS = {2: (48, True), 7: (64, True), 9: (24, True), 11: (20, False), 14: (4, False), 18: (3, False), 20: (2, False),
                  22: (16, True), 24: (32, True), 26: (80, True)}
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")

HEAD = """[net]
width=32
height=32
channels=3

[convolutional]
batch_normalize=1
filters=12
size=3
stride=1
pad=1
activation=leaky
"""
TAIL = """
[convolutional]
filters=18
size=1
stride=1
pad=1
activation=linear

[yolo]
mask=0,1,2
anchors=6,8, 12,10, 20,24
classes=1
num=3
"""


def _conv(filters, groups=None, extra=""):
    g = "groups=%s\n" % groups if groups is not None else ""
    return "\n[convolutional]\nbatch_normalize=1\nfilters=%d\n%ssize=3\nstride=1\npad=1\nactivation=leaky\n%s" % (filters, g, extra)


def _write(tmp_path, text):
    p = tmp_path / "net.cfg"
    p.write_text(text)
    return str(p)


# ---------------------------------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("cin,cout,groups,k,s,pad,act,bn", [
    (12, 12, 12, 3, 1, 1, "leaky", True), (12, 12, 12, 5, 2, 2, "mish", True), (8, 16, 4, 3, 1, 1, "linear", True),
    (24, 48, 3, 3, 2, 0, "leaky", True), (40, 48, 2, 1, 1, 0, "logistic", False), (20, 20, 1, 3, 1, 1, "leaky", False)])
def test_restatement_is_conv2d_with_groups(cin, cout, groups, k, s, pad, act, bn):
    gen = torch.Generator().manual_seed(cin * 131 + cout * 7 + groups)
    x = torch.rand((2, cin, 9, 11), generator=gen) - 0.5
    p = {"weight": (torch.rand((cout, cin // groups, k, k), generator=gen) - 0.5).numpy()}
    if bn:
        p.update(bn_gamma=(torch.rand(cout, generator=gen) + 0.5).numpy(), bn_beta=(torch.rand(cout, generator=gen) - 0.5).numpy(),
                 bn_mean=(torch.rand(cout, generator=gen) - 0.5).numpy(), bn_var=(torch.rand(cout, generator=gen) + 0.5).numpy())
    else:
        p["bias"] = (torch.rand(cout, generator=gen) - 0.5).numpy()
    got = GR.grouped_conv_block(x, p, s, pad, act, groups, accumulate="f64")
    want = GR.conv2d_f64(x, p, s, pad, act, groups)
    assert got.shape == want.shape and got.shape[1] == cout
    # the oracle rounds its float64 conv to float32 before batch norm and activation run in float32
    torch.testing.assert_close(got.double(), want, rtol=2e-6, atol=2e-6)
    if groups > 1:      # ... and the groups matter: the dense conv of the first group's filters alone is another tensor
        assert not torch.allclose(got[:, :cout // groups].double(), want[:, cout // groups:2 * cout // groups])


@pytest.mark.parametrize("cid", sorted(GC.CASES))
def test_gates_fit_the_one_op_cases_on_the_cpu(cid):
    """float32 accumulation against float64 accumulation in the restatement, on the GPU test's inputs, under the GPU test's
    gates: a kernel that sums in float32 in any order can pass them"""
    import test_gpu_bf16 as G
    case = GC.CASES[cid]
    for dtype in GC.DTYPES:
        data = GC.make(case, dtype)
        f32, f64 = GC.reference(case, dtype, data, "f32"), GC.reference(case, dtype, data, "f64")
        assert f32.shape == (3, case["cout"]) + GC.out_hw(case) and bool(torch.isfinite(f64).all())
        if dtype == "float32":
            np.testing.assert_allclose(f32.numpy(), f64.numpy(), err_msg=cid, **G.F32_BLOCK_TOL)
        else:
            rnd = G.MODES[dtype]["rnd"]
            G._close_bf16(rnd(f32), rnd(f64), "%s %s" % (cid, dtype), None, dtype)


@pytest.mark.parametrize("cid", sorted(GC.CASES))
def test_ordered_restatement_is_the_same_operation(cid):
    """tests/grouped_ordered.py (float32, the kernels' sum order, every operation rounded) against ``GC.reference`` under the GPU
    test's own gates: the values the GPU test demands bit for bit are values of the operation the toleranced gates describe"""
    import grouped_ordered as GO
    import test_gpu_bf16 as G
    case = GC.CASES[cid]
    for dtype in GC.DTYPES:
        data = GC.make(case, dtype)
        got = torch.from_numpy(GO.of_case(case, dtype, data))
        want = GC.reference(case, dtype, data)
        assert got.shape == want.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
        if dtype == "float32":
            np.testing.assert_allclose(got.numpy(), want.numpy(), err_msg=cid, **G.F32_BLOCK_TOL)
        else:
            assert torch.equal(got, G.MODES[dtype]["rnd"](got)), (cid, dtype, "not storage values")
            G._close_bf16(got, G.MODES[dtype]["rnd"](want), "%s %s" % (cid, dtype), None, dtype)


def test_ordered_restatement_sees_the_order():
    """the same sums with taps and channels visited in descending order differ from the stated order in stored bits: an equality
    with the ordered restatement is a statement about the order.  In float32 every case shows it, and fp16 shows it on the grouped
    shapes.  A product of two bf16 values has 16 significant bits and is exact in float32, and so are these sums of up to 72 such
    products nearly everywhere; what inexactness is left disappears in the rounding to 8 bits.  In bf16 the equality therefore
    holds the products, the epilogue and the one rounding, and the float32 runs hold the order (the kernels are one template)."""
    import grouped_ordered as GO
    seen = {d: 0 for d in GC.DTYPES}
    for cid in ("dw_c24", "dw_linear", "gr_4x8", "gr_4x4", "gr_dw_c20_k5_res"):
        case = GC.CASES[cid]
        assert case.get("act", "leaky") in GO.EXACT_ACTS
        for dtype in GC.DTYPES:
            data = GC.make(case, dtype)
            stated, reverse = GO.of_case(case, dtype, data), GO.of_case(case, dtype, data, reverse=True)
            differ = int((stated.view(np.uint32) != reverse.view(np.uint32)).sum())
            print("%s %s: %d of %d stored values differ between the two orders" % (cid, dtype, differ, stated.size))
            seen[dtype] += differ > 0
            assert differ > 0 or dtype != "float32", (cid, dtype)
    assert seen["float32"] == 5 and seen["fp16"] >= 1, seen


def test_ordered_gate_leaves_out_mish_and_logistic_only():
    import grouped_ordered as GO
    left_out = sorted(c["id"] for c in GC.DWISE + GC.GROUPED if c.get("act", "leaky") not in GO.EXACT_ACTS)
    assert left_out == sorted(GC.NOT_ORDERED) == ["dw_logistic", "dw_mish", "dw_res_mish", "gr_4x4_wide_res", "gr_4x8_wide_res"]


# ---------------------------------------------------------------------------------------------- the cfg reader

@pytest.mark.parametrize("body,msg", [
    (_conv(16, 5), r"conv block 1: grouped convolution: groups=5 does not divide 12 input channels and filters=16"),
    (_conv(16, 3), r"conv block 1: grouped convolution: groups=3 does not divide 12 input channels and filters=16"),
    (_conv(12, 0), r"conv block 1: grouped convolution with groups=0"),
    (_conv(12, -2), r"conv block 1: grouped convolution with groups=-2"),
    (_conv(12, 12, "dilation=2\n"), r"dilated convolution"),
])
def test_refuses_by_message(tmp_path, body, msg):
    cfg = _write(tmp_path, HEAD + body + TAIL)
    with pytest.raises(ValueError, match=msg):
        yolov3.Darknet(cfg)
    blocks, net_info = parse_config(cfg)
    with pytest.raises(ValueError, match=msg):
        build_plan(blocks, net_info, 1, 32, 32, 4)


def test_refuses_a_grouped_stem_and_a_grouped_head_conv(tmp_path):
    stem = HEAD.replace("filters=12\n", "filters=12\ngroups=3\n") + TAIL
    with pytest.raises(ValueError, match=r"conv block 0: grouped convolution \(groups=3\) is not supported on the conv that reads the network input"):
        yolov3.Darknet(_write(tmp_path, stem))
    head = HEAD + _conv(18) + TAIL.replace("filters=18\n", "filters=18\ngroups=3\n")
    with pytest.raises(ValueError, match=r"conv block 2: grouped convolution \(groups=3\) is not supported directly in front of yolo block 3"):
        yolov3.Darknet(_write(tmp_path, head))


def test_accepts_groups_that_divide_both_counts(tmp_path):
    for groups, filters in ((1, 16), (2, 16), (4, 16), (12, 12), (12, 24)):
        net = yolov3.Darknet(_write(tmp_path, HEAD + _conv(filters, groups) + TAIL))
        assert net._convs[1]["groups"] == groups and net._convs[1]["cin"] == 12


def test_mini_cfg_groups_on_the_first_conv_stays_refused(tmp_path):
    text = open(MODELS["mini"]).read()
    head = "[convolutional]\n"
    i = text.index(head) + len(head)
    cfg = _write(tmp_path, text[:i] + "groups=2\n" + text[i:])
    with pytest.raises(ValueError, match=r"grouped convolution \(groups=2\) is not supported"):
        yolov3.Darknet(cfg)
    blocks, net_info = parse_config(cfg)
    with pytest.raises(ValueError, match=r"grouped convolution \(groups=2\) is not supported"):
        build_plan(blocks, net_info, 1, 64, 64, 4)


def test_dropout_was_an_unsupported_block_and_is_an_alias_now():
    net = yolov3.Darknet(CFG)
    assert net.blocks[5]["type"] == "dropout"
    for reuse in (True, False):
        d = build_plan(net.blocks, net.net_info, 2, 64, 96, 2, reuse=reuse)
        assert all(op["block"] != 5 for op in d["ops"]) and "t5" not in d["buffers"]
        assert d["tensor_of"][5] is d["tensor_of"][4] and d["shapes"][5] == d["shapes"][4] == (16, 64, 96)
        conv6 = next(op for op in d["ops"] if op["block"] == 6)
        assert conv6["inp"] is d["tensor_of"][4]
        # the shortcut in front of it is still fused into conv 3, which a second reader of conv 3 would forbid
        conv3 = next(op for op in d["ops"] if op["block"] == 3)
        assert conv3["res"] is d["tensor_of"][0] and conv3["out"] is d["tensor_of"][4]


def test_plan_of_grouped_cfg():
    net = yolov3.Darknet(CFG)
    d = build_plan(net.blocks, net.net_info, 2, 64, 96, 2)
    convs = {op["block"]: op for op in d["ops"] if op["kind"] == "conv"}
    assert {b: op.get("groups") for b, op in convs.items() if "groups" in op} == {b: g for b, (g, _) in GROUPED_BLOCKS.items()}
    # operands that are channel slices of concat buffers: conv 22 reads one slice of route 23's buffer and writes the other;
    # conv 24 writes into route 25's; conv 26's fused shortcut operand is route 25 itself
    t = convs[22]
    assert (t["inp"].buf, t["inp"].off, t["inp"].ld, t["inp"].c) == ("cat23", 0, 32, 16)
    assert (t["out"].buf, t["out"].off, t["out"].ld, t["out"].c) == ("cat23", 16, 32, 16)
    assert (convs[24]["out"].buf, convs[24]["out"].off, convs[24]["out"].ld) == ("cat25", 0, 80)
    assert (convs[18]["out"].buf, convs[18]["out"].off, convs[18]["out"].ld) == ("cat25", 32, 80)
    assert convs[26]["res"] is d["tensor_of"][25] and d["tensor_of"][27] is convs[26]["out"]
    assert not any(op["kind"] in ("add", "copy") for op in d["ops"])


# ---------------------------------------------------------------------------------------------- the weight stream

def test_stream_length_and_round_trip(tmp_path):
    blocks, net_info = parse_config(CFG)
    _, convs = W.conv_layout(blocks, net_info)
    want = 0
    for c in convs:
        blk = blocks[c["block_idx"]]
        g = int(blk.get("groups", 1))
        assert c["groups"] == g and c["cin"] % g == 0
        want += (4 if blk.get("batch_normalize") else 1) * blk["filters"] + blk["filters"] * (c["cin"] // g) * blk["size"] ** 2
    assert W.stream_length(blocks, net_info) == want == 25374
    params = W.synth_params(blocks, net_info, seed=3)
    for c, p in zip(convs, params):
        assert p["weight"].shape == (c["cout"], c["cin"] // c["groups"], c["k"], c["k"])
    path = str(tmp_path / "grouped.weights")
    W.write_darknet_weights(path, params)
    assert os.path.getsize(path) == 20 + 4 * want
    _, back = W.read_darknet_weights(path, blocks, net_info)
    assert len(back) == len(params)
    for a, b in zip(params, back):
        assert sorted(a) == sorted(b)
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key


def test_stream_order_is_cout_cin_over_groups_k_k(tmp_path):
    """a hand-made stream: bias first (no batch norm), then filters * (c / groups) * size * size values, filter-major"""
    cfg = _write(tmp_path, HEAD + "\n[convolutional]\nfilters=4\ngroups=2\nsize=3\nstride=1\npad=1\nactivation=linear\n" + _conv(18) + TAIL)
    blocks, net_info = parse_config(cfg)
    n0 = 4 * 12 + 12 * 3 * 9
    n1 = 4 + 4 * 6 * 9
    total = W.stream_length(blocks, net_info)
    assert total == n0 + n1 + (4 * 18 + 18 * 4 * 9) + (18 + 18 * 18)
    stream = np.arange(total, dtype=np.float32)
    path = str(tmp_path / "hand.weights")
    with open(path, "wb") as fh:
        np.array([0, 2, 0, 0, 0], dtype=np.int32).tofile(fh)
        stream.tofile(fh)
    _, params = W.read_darknet_weights(path, blocks, net_info)
    p = params[1]
    assert np.array_equal(p["bias"], n0 + np.arange(4, dtype=np.float32))
    assert p["weight"].shape == (4, 6, 3, 3)
    for co in range(4):
        for c in range(6):
            for ky in range(3):
                for kx in range(3):
                    assert p["weight"][co, c, ky, kx] == n0 + 4 + ((co * 6 + c) * 3 + ky) * 3 + kx


def test_ungrouped_synth_params_are_unchanged():
    """groups == 1 leaves every hashed value where it was: the shipped cfgs' goldens do not move"""
    blocks, net_info = parse_config(MODELS["mini"])
    _, convs = W.conv_layout(blocks, net_info)
    assert all(c["groups"] == 1 for c in convs)
    p = W.synth_params(blocks, net_info, seed=0)[1]
    c = convs[1]
    fan = c["cin"] * c["k"] ** 2
    a = np.sqrt(3.0 * 2.0 / (1.01 * fan))
    want = (-a + 2 * a * W.hash_uniform(0, 8, c["cout"] * fan)).astype(np.float32).reshape(c["cout"], c["cin"], c["k"], c["k"])
    assert np.array_equal(p["weight"], want)


# ---------------------------------------------------------------------------------------------- device layouts

def test_device_layouts_element_by_element():
    net = yolov3.Darknet(CFG, dtype="float32")
    net.set_params(W.synth_params(net.blocks, net.net_info, seed=1))
    slot_of = {c["block_idx"]: s for s, c in enumerate(net._convs)}
    for block, path in ((2, _hip.PATH_DWISE), (9, _hip.PATH_DWISE), (14, _hip.PATH_GROUPED), (18, _hip.PATH_GROUPED),
                        (20, _hip.PATH_GROUPED), (11, _hip.PATH_GROUPED), (2, _hip.PATH_GROUPED)):
        slot = slot_of[block]
        c = net._convs[slot]
        w = net._params[slot]["weight"]
        cout, cg, k = c["cout"], c["cin"] // c["groups"], c["k"]
        entry = net._device_weights(slot, path, "float32", "cpu")
        host = entry["weight"].numpy()
        scale, bias = net._fold_bn(slot)
        assert (entry["cout_pad"], entry["k_ld"]) == padded_weight_dims(path, cout, c["cin"], k, 4, c["groups"])
        assert entry["cout_pad"] == (cout + 7) // 8 * 8 and entry["scale"].numel() == entry["bias"].numel() == entry["cout_pad"]
        assert np.array_equal(entry["scale"].numpy()[:cout], scale) and np.array_equal(entry["bias"].numpy()[:cout], bias)
        seen = np.zeros(host.shape, dtype=bool)
        if path == _hip.PATH_DWISE:
            assert host.shape == (k * k, (cout + 7) // 8 * 8) and cg == 1
            for ky in range(k):
                for kx in range(k):
                    for co in range(cout):
                        assert host[ky * k + kx, co] == w[co, 0, ky, kx]
                        seen[ky * k + kx, co] = True
        else:
            assert host.shape == (entry["cout_pad"], entry["k_ld"]) and entry["k_ld"] >= k * k * cg and entry["k_ld"] % 8 == 0
            for co in range(cout):
                for ky in range(k):
                    for kx in range(k):
                        for ci in range(cg):
                            assert host[co, (ky * k + kx) * cg + ci] == w[co, ci, ky, kx]
                            seen[co, (ky * k + kx) * cg + ci] = True
        assert not host[~seen].any()                                  # the padding is zero
        want, cp, k_ld = GC.device_weights(None, path, w)            # the GPU test's own layout code agrees
        assert (cp, k_ld) == (entry["cout_pad"], entry["k_ld"]) and np.array_equal(want, host)
    bits = net._device_weights(slot_of[2], _hip.PATH_DWISE, "bf16", "cpu")["weight"]
    assert bits.dtype == torch.int16 and bits.shape == (9, 48)
    assert torch.equal(bits.view(torch.bfloat16).float(), torch.from_numpy(net._params[slot_of[2]]["weight"].reshape(48, 9).T.copy()).bfloat16().float())


# ---------------------------------------------------------------------------------------------- the C ABI

def test_y3_op_keeps_its_size_and_offsets():
    assert ctypes.sizeof(_hip.Y3Op) == 248
    assert _hip.Y3Op.groups.offset == _hip.Y3Op.n_anchor.offset == 120 and _hip.Y3Op.n_attr.offset == 124
    op = _hip.Y3Op()
    op.groups = 7
    assert op.n_anchor == 7
    assert _hip.capabilities() & _hip.CAP_GROUPED_CONV == 16384


def test_conv_path_sends_misaligned_depthwise_ops_to_the_grouped_kernel():
    """the depthwise kernel loads and stores 16 bytes at a time: an op on 8-channel strides whose input, output or shortcut
    operand does not start on a 16-byte boundary is answered 4, not 5 (and so runs instead of being refused)"""
    lib = _hip.lib()
    fake = kc._Fake()
    ops = _one_op(fake, cin=24, cout=24, groups=24)
    assert lib.y3_conv_path(ctypes.byref(ops[0])) == _hip.PATH_DWISE
    for field in ("d_in", "d_out"):
        ops = _one_op(fake, cin=24, cout=24, groups=24)
        setattr(ops[0], field, getattr(ops[0], field) + 8)
        assert lib.y3_conv_path(ctypes.byref(ops[0])) == _hip.PATH_GROUPED, field
    ops = _one_op(fake, cin=24, cout=24, groups=24, flags=_hip.F_LEAKY | _hip.F_RESIDUAL, res_ld=24, d_res=fake(1 << 16) + 8)
    assert lib.y3_conv_path(ctypes.byref(ops[0])) == _hip.PATH_GROUPED
    ops = _one_op(fake, cin=24, cout=24, groups=24, flags=_hip.F_LEAKY | _hip.F_RESIDUAL, res_ld=24, d_res=fake(1 << 16))
    assert lib.y3_conv_path(ctypes.byref(ops[0])) == _hip.PATH_DWISE


def _fill(dtype, batch=2):
    net = yolov3.Darknet(CFG, dtype=dtype)
    es = kc.DTYPES[net.dtype][1]
    desc = build_plan(net.blocks, net.net_info, batch, 64, 96, es, reuse=True, fuse=True)
    fake = kc._Fake(net._convs, es)
    ops, needs, frag = fill_ops(desc, net.net_info, net._convs, net.dtype, batch, "u8", net.scores, None, fake)
    return net, ops, needs, frag, fake


@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_fill_ops_sets_groups_paths_and_the_capability(dtype):
    lib = _hip.lib()
    net, ops, needs, frag, _ = _fill(dtype)
    assert needs == _hip.CAP_GROUPED_CONV | _hip.CAP_MISH
    es = kc.DTYPES[net.dtype][1]
    for op in ops:
        if op.kind != _hip.OP_CONV:
            continue
        groups, dwise = GROUPED_BLOCKS.get(op.block_idx, (0, False))
        assert op.groups == groups, op.block_idx
        path = lib.y3_conv_path(ctypes.byref(op))
        if groups:
            assert path == (_hip.PATH_DWISE if dwise else _hip.PATH_GROUPED), op.block_idx
            assert lib.y3_conv_fragment_weight_bytes(ctypes.byref(op), None) == 0
            c = next(c for c in net._convs if c["block_idx"] == op.block_idx)
            assert (op.cout_pad, op.k_ld) == padded_weight_dims(path, c["cout"], c["cin"], c["k"], es, groups)
            _hip.check(lib.y3_set_tuning(b"grouped_generic", 1))
            try:
                assert lib.y3_conv_path(ctypes.byref(op)) == _hip.PATH_GROUPED
            finally:
                _hip.check(lib.y3_set_tuning(b"grouped_generic", 0))
            assert lib.y3_conv_path(ctypes.byref(op)) == path
        else:
            assert path in (_hip.PATH_IGEMM, _hip.PATH_STEM, _hip.PATH_DIRECT, _hip.PATH_STEM_MFMA)
    assert lib.y3_set_tuning(b"grouped_generic", 2) != 0 and b"grouped_generic" in lib.y3_last_error()
    # a stale library is refused by name
    real = _hip.capabilities
    _hip.capabilities = lambda: real() & ~_hip.CAP_GROUPED_CONV
    try:
        with pytest.raises(_hip.HipLibraryError, match="grouped convolution"):
            _hip.require_capabilities(needs, CFG)
    finally:
        _hip.capabilities = real


@no_gpu
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_plan_of_grouped_cfg_names_the_kernels(dtype):
    """plan creation on fake addresses: which op runs which kernel, its FLOPs divided by groups, its weight bytes the group's"""
    lib = _hip.lib()
    net, ops, _, _, fake = _fill(dtype)
    tag = {"float32": "f32", "bf16": "bf16", "fp16": "f16"}[dtype]
    es = kc.DTYPES[net.dtype][1]
    want = {2: "conv_dwise_%s_k3s1", 7: "conv_dwise_%s_k3s2", 9: "conv_dwise_%s_kn", 11: "conv_grouped_%s_oc1", 14: "conv_grouped_%s_oc8",
            18: "conv_grouped_%s_oc8", 20: "conv_grouped_%s_oc8", 22: "conv_dwise_%s_k3s1", 24: "conv_dwise_%s_k3s1", 26: "conv_dwise_%s_k3s1"}
    for generic in (0, 1):
        _hip.check(lib.y3_set_tuning(b"grouped_generic", generic))
        try:
            if generic:
                net, ops, _, _, fake = _fill(dtype)        # (the weight layout follows the path)
            handle = ctypes.c_void_p()
            _hip.check(lib.y3_plan_create(ops, len(ops), fake(4096), ctypes.byref(handle)))
        finally:
            _hip.check(lib.y3_set_tuning(b"grouped_generic", 0))
        try:
            for i, op in enumerate(ops):
                name = lib.y3_plan_op_kernel(handle, i).decode()
                if op.block_idx in want:
                    first = want[op.block_idx] % tag
                    if generic and "dwise" in first:
                        first = "conv_grouped_%s_oc1" % tag
                    assert name == first, (op.block_idx, name)
                    dense = 2.0 * op.ksize ** 2 * op.in_c * op.out_c * op.out_h * op.out_w * op.batch
                    assert lib.y3_plan_op_flops(handle, i) == dense / op.groups
                    px_in, px_out = op.batch * op.in_h * op.in_w, op.batch * op.out_h * op.out_w
                    nbytes = (px_in * op.in_c + px_out * op.out_c * (2 if op.flags & _hip.F_RESIDUAL else 1) +
                              op.ksize ** 2 * (op.in_c // op.groups) * op.out_c) * es
                    assert lib.y3_plan_op_bytes(handle, i) == nbytes
                    assert _hip.plan_op_dims(handle, i)[1] % 64 == 0
                else:
                    assert "dwise" not in name and "grouped" not in name, (op.block_idx, name)
        finally:
            lib.y3_plan_destroy(handle)


def _one_op(fake, cin=16, cout=16, groups=16, k=3, flags=_hip.F_LEAKY, **over):
    ops = (_hip.Y3Op * 1)()
    op = ops[0]
    op.kind, op.dtype, op.flags, op.batch, op.block_idx = _hip.OP_CONV, _hip.Y3_BF16, flags, 1, 7
    op.in_h = op.in_w = op.out_h = op.out_w = 8
    op.in_c, op.in_ld, op.out_c, op.out_ld = cin, cin, cout, cout
    op.ksize, op.stride, op.pad = k, 1, (k - 1) // 2
    op.groups = groups
    op.cout_pad, op.k_ld = 128, 1024
    op.d_in, op.d_out, op.d_weight, op.d_scale, op.d_bias = (fake(1 << 16) for _ in range(5))
    for key, val in over.items():
        setattr(op, key, val)
    return ops


@no_gpu
def test_plan_creation_refuses_the_bad_ops():
    lib = _hip.lib()
    fake = kc._Fake()

    def create(ops):
        handle = ctypes.c_void_p()
        rc = lib.y3_plan_create(ops, 1, fake(4096), ctypes.byref(handle))
        if rc == 0:
            lib.y3_plan_destroy(handle)
        return rc, lib.y3_last_error().decode()

    assert create(_one_op(fake))[0] == 0
    assert create(_one_op(fake, cin=24, cout=48, groups=3))[0] == 0
    for ops, words in (
            (_one_op(fake, groups=-1), "conv block 7: groups=-1"),
            (_one_op(fake, cin=16, cout=16, groups=3), "conv block 7: groups=3 does not divide 16 input and 16 output channels"),
            (_one_op(fake, cin=16, cout=20, groups=8), "conv block 7: groups=8 does not divide 16 input and 20 output channels"),
            (_one_op(fake, flags=_hip.F_PLAN_INPUT | _hip.F_IN_NCHW_F32), "conv block 7: a grouped conv (groups=16) cannot read the network input"),
            (_one_op(fake, flags=_hip.F_PLAN_INPUT | _hip.F_IN_NHWC_U8BGR), "cannot read the network input"),
            (_one_op(fake, flags=_hip.F_PLAN_INPUT), "cannot read the network input"),
            (_one_op(fake, flags=_hip.F_OUT_F32), "conv block 7: a grouped conv (groups=16) cannot store float32"),
            (_one_op(fake, k_ld=8), "conv block 7: depthwise weights"),
            (_one_op(fake, cin=32, cout=32, groups=4, k_ld=64), "conv block 7: grouped weights need k_ld >= 72"),
            (_one_op(fake, cin=32, cout=32, groups=4, cout_pad=24), "conv block 7: grouped weights need")):
        rc, err = create(ops)
        assert rc == -1 and words in err, (words, rc, err)
    # zero-initialised callers: groups 0 and 1 are the ordinary conv they always were
    for g in (0, 1):
        ops = _one_op(fake, cin=128, cout=128, groups=g, k_ld=9 * 128)
        assert lib.y3_conv_path(ctypes.byref(ops[0])) == _hip.PATH_IGEMM
        opt = _hip.options(auto_mask=_hip.AM_IGEMM_ONLY)     # (no kernel that would make a fragment-order weight copy here)
        handle = ctypes.c_void_p()
        _hip.check(lib.y3_plan_create_ex(ops, 1, fake(4096), ctypes.byref(opt), ctypes.byref(handle)))
        assert lib.y3_plan_op_kernel(handle, 0).decode().startswith("conv_igemm")
        lib.y3_plan_destroy(handle)


# ---------------------------------------------------------------------------------------------- the grouped library's device code

def test_grouped_library_code_objects_and_census():
    """libyolov3_hip_grouped.so, the dependency of libyolov3_hip.so that holds conv_dwise and conv_grouped: 15 instances, no LDS,
    blocks of whole waves; and its census (tests/golden/kernel_instances_grouped.json, recorded on an MI355X by
    tools/make_kernel_instances.py --library grouped): one key per instance and dtype.  What every library is held to -- gfx950
    code only, no spills, budgets inside a CU, every compiled instance launched by a recorded footprint case, no recorded symbol
    missing, no kernel shared with the main library -- is tests/test_code_object.py's."""
    import kernel_census as census
    kernels = census.kernels("grouped")          # (asserts: built, device code for gfx950 only)
    names = sorted(k[".name"] for k in kernels)
    assert len(names) == 15 and sum("conv_dwise_kernel" in n for n in names) == 9 and sum("conv_grouped_kernel" in n for n in names) == 6
    for k in kernels:
        assert k[".group_segment_fixed_size"] == 0 and k[".max_flat_workgroup_size"] % 64 == 0, k[".name"]
    fixture = census.load("grouped")
    assert sorted(fixture["footprint"]) == sorted("grouped_%s-%s" % (i, d) for i in (
        "dwise_k3s1", "dwise_k3s2", "dwise_kn", "grouped_oc1", "grouped_oc8") for d in GC.DTYPES)
    assert all(len(v) == 1 for v in fixture["footprint"].values())
    assert len({v[0] for v in fixture["footprint"].values()}) == 15        # one key per (kernel instance, dtype)


# ---------------------------------------------------------------------------------------------- the kernel-level suites
# tests/grouped_suites.py: the epilogue forms of tests/test_gpu_grouped_epilogue.py and the rows past 4 GiB of
# tests/test_gpu_grouped_big.py, on fake addresses

def test_every_compiled_instance_has_an_epilogue_form_and_a_big_row():
    """no skip list: every (instance, dtype) of the grouped library's census has an epilogue form and, fp16 aside (it shares
    bf16's address code), a row past 4 GiB; an instance compiled later fails here until both suites hold it"""
    import epilogue_cases as E
    import grouped_suites as GS
    import kernel_census as census
    keys = sorted(census.load("grouped")["footprint"])
    assert len(keys) == 15
    pinned = {GS.census_key(f["instance"], d) for f in GS.EPILOGUE_FORMS.values() for d in E.DTYPES}
    big = {GS.census_key(i, d) for i in GS.BIG_ROWS for d in GS.BIG_DTYPES}
    assert set(keys) - pinned == set(), "instances without an epilogue form: %s" % sorted(set(keys) - pinned)
    need_big = {k for k in keys if not k.endswith("-fp16")}
    assert need_big - big == set(), "instances without a row past 4 GiB: %s" % sorted(need_big - big)
    assert pinned - set(keys) == set() and big - set(keys) == set()          # ... and neither table names an instance that is gone
    # each form and each row is a shape of the instance it is listed under
    for form in GS.EPILOGUE_FORMS:
        GS.epilogue_case(form)
    for instance, case in GS.BIG_ROWS.items():
        assert GS.instance_of(case) == instance and case.get("res") and case.get("act", "leaky") == "leaky"
    assert [f["instance"] for f in GS.EPILOGUE_FORMS.values()].count("grouped_oc8") == 2      # 16-byte stores, and element by element


@no_gpu
@pytest.mark.parametrize("instance", ["dwise_k3s1", "dwise_k3s2", "dwise_kn", "grouped_oc8", "grouped_oc1"])
def test_big_rows_span_4_gib_on_odd_maps_and_keep_their_instance(instance):
    import footprint_util as fu
    import grouped_suites as GS
    case = GS.BIG_ROWS[instance]
    ho, wo = GC.out_hw(case)
    assert (ho % 2 == 1 and wo % 2 == 1) if case["s"] == 2 else (case["h"] % 2 == 1 and case["w"] % 2 == 1)
    assert case["k"] == (5 if instance == "dwise_kn" else 3)
    for dtype in GS.BIG_DTYPES:
        B = GS.big_batch(case, dtype)
        ops, lay = GS.build(case, dtype, B, "strided", lead=[fu.pad_operand()])
        op = ops[0]
        name, dims, err = GS.create(ops, lay)
        assert name == GS.kernel_name(instance, dtype), (instance, dtype, name, err)
        assert lay.operands[0].name == "pad" and lay.operands[0].body_bytes >= (1 << 32)
        assert max(B * op.in_h * op.in_w, B * op.out_h * op.out_w) <= fu.MAX_PIXELS
        spans = GS.span_operands(lay)
        assert [o.name for o in spans] == ["input", "output", "residual"]
        assert len({op.in_ld, op.out_ld, op.res_ld}) == 3 and all(o.slices[0][0] > 0 for o in spans)
        for o in spans:
            frame = o.body_bytes // B
            assert frame * B == o.body_bytes == o.pixels * o.ld * o.es
            assert o.body_bytes > fu.SPAN + frame, (instance, dtype, o.name, o.body_bytes)
            assert frame & (frame - 1) != 0, (instance, o.name, frame)
        # ... and the batch is no larger than that takes
        assert any(o.body_bytes - 2 * (o.body_bytes // B) <= fu.SPAN + o.body_bytes // B for o in spans)
        # the launch, restated: batch x out_h x ceil(out_w / 4) x out_c / 8 lanes, or pixels x out_c / bn, in blocks of 256
        assert dims[1] == 256 and dims[0] * dims[1] == GS.launch_threads(case, B) <= fu.MAX_THREADS, (dims, GS.launch_threads(case, B))
        assert lay.total < 32 << 30


def _largest_batch(case):
    """(the largest batch plan creation takes, "pixels" or "threads": what refuses the next one), from the restated launch"""
    import footprint_util as fu
    import grouped_suites as GS
    ok = fu.MAX_PIXELS // GS.frame_pixels(case)
    if GS.launch_threads(case, ok) <= fu.MAX_THREADS:
        return ok, "pixels"
    lo, hi = 1, ok
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if GS.launch_threads(case, mid) <= fu.MAX_THREADS else (lo, mid - 1)
    return lo, "threads"


# the same instances with so few channels that a launch holds at most two threads per pixel: there the pixel limit comes first
NARROW_ROWS = {"dwise_k3s1": dict(cin=8, cout=8, groups=8), "dwise_k3s2": dict(cin=8, cout=8, groups=8),
               "dwise_kn": dict(cin=8, cout=8, groups=8), "grouped_oc8": dict(cin=16, cout=16, groups=2),
               "grouped_oc1": dict(cin=2, cout=2, groups=2)}
# (the stride-2 row has 81 input pixels and 5 x 2 x 15 lanes a frame, so its input pixels come first; at 240 channels its launch does)
WIDE_ROWS = {"dwise_k3s2": dict(cin=240, cout=240, groups=240)}


@no_gpu
@pytest.mark.parametrize("instance", ["dwise_k3s1", "dwise_k3s2", "dwise_kn", "grouped_oc8", "grouped_oc1"])
def test_big_rows_are_refused_at_the_pixel_and_the_launch_limit(instance):
    """plan creation takes each row at its true limit and refuses it one frame later: by check_size's message where 2^31 pixels
    less one tile come first, by check_launch's message naming the kernel where 2^32 - 256 threads do.  The rows themselves meet
    the launch limit first (120 / 8 chunks, 8 or 16 threads a pixel; not the stride-2 row); their narrow forms meet the pixel limit."""
    import footprint_util as fu
    import grouped_suites as GS
    seen = set()
    row = GS.BIG_ROWS[instance]
    for case in [row, dict(row, **NARROW_ROWS[instance])] + ([dict(row, **WIDE_ROWS[instance])] if instance in WIDE_ROWS else []):
        assert GS.instance_of(case) == instance
        ok, why = _largest_batch(case)
        seen.add(why)
        for dtype in GS.BIG_DTYPES:
            want = GS.kernel_name(instance, dtype)
            ops, lay = GS.build(case, dtype, ok, "strided")
            name, dims, err = GS.create(ops, lay)
            assert name == want, (instance, dtype, ok, name, err)
            assert dims[0] * dims[1] == GS.launch_threads(case, ok) <= fu.MAX_THREADS
            ops, lay = GS.build(case, dtype, ok + 1, "strided")
            name, dims, err = GS.create(ops, lay)
            assert name is None and "block 1" in err, (instance, dtype, ok + 1, name)
            if why == "pixels":
                assert ok == fu.MAX_PIXELS // GS.frame_pixels(case) and (ok + 1) * GS.frame_pixels(case) > fu.MAX_PIXELS
                assert "pixels" in err and "limit is %d" % fu.MAX_PIXELS in err, err
            else:
                assert (ok + 1) * GS.frame_pixels(case) <= fu.MAX_PIXELS
                assert "threads" in err and "limit is %d" % fu.MAX_THREADS in err and want in err, err
                assert "launch of %d threads" % GS.launch_threads(case, ok + 1) in err, err
    assert seen == {"pixels", "threads"}, (instance, seen)


@no_gpu
@pytest.mark.parametrize("form", ["dwise_k3s1", "dwise_k3s2", "dwise_kn", "grouped_oc8_vec", "grouped_oc8_elem", "grouped_oc1"])
def test_epilogue_forms_name_their_kernels(form):
    """the one-op plans of tests/test_gpu_grouped_epilogue.py on fake addresses laid out as the GPU test lays them out"""
    import grouped_suites as GS
    assert sorted(GS.EPILOGUE_FORMS) == sorted(["dwise_k3s1", "dwise_k3s2", "dwise_kn", "grouped_oc8_vec", "grouped_oc8_elem", "grouped_oc1"])
    case = GS.epilogue_case(form)
    fake = kc._Fake()
    for dtype in GC.DTYPES:
        es = 4 if dtype == "float32" else 2
        (in_off, in_ld), (out_off, out_ld) = GC.strides(case, case["cin"], dtype), GC.strides(case, case["cout"], dtype)
        res_off, res_ld = (out_off + 8, out_ld + 16) if case.get("wide") else (out_off, out_ld)
        code = {"float32": _hip.Y3_F32, "bf16": _hip.Y3_BF16, "fp16": _hip.Y3_F16}[dtype]
        ops = _one_op(fake, cin=case["cin"], cout=case["cout"], groups=case["groups"], k=case["k"], dtype=code,
                      flags=_hip.F_LEAKY | _hip.F_RESIDUAL, batch=case["B"], in_h=case["h"], in_w=case["w"], in_ld=in_ld, out_ld=out_ld,
                      res_ld=res_ld, stride=case["s"], pad=case["pad"], out_h=GC.out_hw(case)[0], out_w=GC.out_hw(case)[1])
        op = ops[0]
        op.d_in, op.d_out, op.d_res = fake(1 << 16) + in_off * es, fake(1 << 16) + out_off * es, fake(1 << 16) + res_off * es
        path = _hip.lib().y3_conv_path(ctypes.byref(op))
        _, op.cout_pad, op.k_ld = GC.device_weights(case, path, np.zeros((case["cout"], case["cin"] // case["groups"], case["k"], case["k"]), dtype=np.float32))
        handle = ctypes.c_void_p()
        _hip.check(_hip.lib().y3_plan_create(ops, 1, fake(4096), ctypes.byref(handle)))
        name = _hip.lib().y3_plan_op_kernel(handle, 0).decode()
        _hip.lib().y3_plan_destroy(handle)
        assert name == GS.kernel_name(case["instance"], dtype), (form, dtype, name)
        if case.get("off"):
            assert op.d_in % 16 == op.d_out % 16 == op.d_res % 16 == 8       # vec_in == vec_out == 0 in launch_conv_grouped
        else:
            assert op.d_in % 16 == op.d_out % 16 == op.d_res % 16 == 0
