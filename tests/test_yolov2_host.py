"""YOLOv2 without a GPU: the cfg reader on fractional anchors, the plan of [reorg] / [region] blocks, every refusal, the C ABI's
reorg bits and its op validation on fake addresses, the two weight-file headers, the shipped cfgs, and the restatement of
tests/yolov2_restate.py pinned by properties that do not depend on the package."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.plan import build_plan, infer_shapes

import yolov2_restate as R
from golden_util import MODEL_DIR

V2 = os.path.join(MODEL_DIR, "yolov2.cfg")
V2_TINY = os.path.join(MODEL_DIR, "yolov2-tiny.cfg")
ANCHORS = [[0.57273, 0.677385], [1.87446, 2.06253], [3.33843, 5.47434], [7.88282, 3.52778], [9.77052, 9.16828]]


def _conv(f, k, act="leaky", bn=True):
    return "[convolutional]\n%sfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=%s\n\n" % (
        "batch_normalize=1\n" if bn else "", f, k, act)


def mini_cfg(classes=20, reorg="[reorg]\nstride=2\n\n", region_extra="", head_filters=None, num=5, width=64, height=64,
             drop=()):
    """A YOLOv2 in miniature: trunk to /8, a 1x1 on the /4 map, reorg, route with the trunk, 3x3, head, region."""
    anchors = ", ".join("%g, %g" % tuple(a) for a in (ANCHORS + [[1.5, 2.5]] * 4)[:max(num, 1)])
    region = "[region]\nanchors = %s\nclasses=%d\ncoords=4\nnum=%d\nsoftmax=1\n" % (anchors, classes, num)
    for key in drop:
        region = re.sub(r"%s=.*\n" % key, "", region)
    f = num * (5 + classes) if head_filters is None else head_filters
    return ("[net]\nwidth=%d\nheight=%d\nchannels=3\n\n" % (width, height) +
            _conv(16, 3) + "[maxpool]\nsize=2\nstride=2\n\n" +          # 0, 1
            _conv(32, 3) + "[maxpool]\nsize=2\nstride=2\n\n" +          # 2, 3   (32, H/4, W/4)
            _conv(64, 3) + "[maxpool]\nsize=2\nstride=2\n\n" +          # 4, 5
            _conv(64, 3) +                                              # 6      (64, H/8, W/8)
            "[route]\nlayers=-3\n\n" +                                  # 7 -> block 4
            _conv(8, 1) +                                               # 8      (8, H/4, W/4)
            reorg +                                                     # 9      (32, H/8, W/8)
            "[route]\nlayers=-1,-4\n\n" +                               # 10     (96, H/8, W/8)
            _conv(64, 3) +                                              # 11
            _conv(f, 1, "linear", False) +                              # 12
            region + region_extra)                                      # 13


def _write(tmp_path, text, name="mini_v2.cfg"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _blocks(path):
    blocks, net_info = parse_config(path)
    for i, blk in enumerate(blocks):
        if blk["type"] == "route":
            blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
    return blocks, net_info


# ------------------------------------------------------------------ cfg and plan

def test_parse_config_keeps_fractional_anchors(tmp_path):
    blocks, _ = parse_config(_write(tmp_path, mini_cfg()))
    region = blocks[-1]
    assert region["type"] == "region" and region["anchors"] == ANCHORS
    assert all(isinstance(v, float) for a in region["anchors"] for v in a)
    assert (region["num"], region["classes"], region["coords"], region["softmax"]) == (5, 20, 4, 1)
    assert parse_config(V2)[0][-1]["anchors"] == ANCHORS and parse_config(V2_TINY)[0][-1]["anchors"] == ANCHORS


@pytest.mark.parametrize("kind", ["reorg", "reorg3d"])
def test_plan_shapes_and_reorg_lands_in_the_route_slice(tmp_path, kind):
    blocks, net_info = _blocks(_write(tmp_path, mini_cfg(reorg="[%s]\nstride=2\n\n" % kind)))
    shapes = infer_shapes(blocks, net_info, 64, 96)
    assert shapes[8] == (8, 16, 24) and shapes[9] == (32, 8, 12) and shapes[10] == (96, 8, 12) and shapes[13] == (125, 8, 12)
    d = build_plan(blocks, net_info, 2, 64, 96, 2, reuse=True, fuse=True)
    ops = {o["block"]: o for o in d["ops"]}
    ro = ops[9]
    assert ro["kind"] == "reorg" and ro["stride"] == 2 and bool(ro.get("form3d")) == (kind == "reorg3d")
    assert (ro["inp"].c, ro["inp"].h, ro["inp"].w) == (8, 16, 24) and ro["inp"].buf == ops[8]["out"].buf
    # no copy: the reorg writes channels [0, 32) and the trunk conv (block 6) channels [32, 96) of the route's buffer
    assert not [o for o in d["ops"] if o["kind"] == "copy"]
    out, trunk, cat = ro["out"], ops[6]["out"], d["tensor_of"][10]
    assert out.buf == trunk.buf == cat.buf == "cat10"
    assert (out.off, out.c, out.ld, out.h, out.w) == (0, 32, 96, 8, 12) and (trunk.off, trunk.c, trunk.ld) == (32, 64, 96)
    assert (cat.off, cat.c, cat.ld) == (0, 96, 96) and ops[11]["inp"] is cat
    # the head: one decode over all five anchors, no new flag, the head conv keeps float32 logits
    yolo = ops[13]
    assert yolo["kind"] == "yolo" and yolo["region"] is True and yolo["n_attr"] == 25 and len(yolo["anchors"]) == 5
    assert "scale_x_y" not in yolo and "new_coords" not in yolo
    assert ops[12]["out"].f32 and d["rows_total"] == yolo["rows_total"] == 5 * 8 * 12 and yolo["row_offset"] == 0


@pytest.mark.parametrize("hw", [(64, 64), (64, 96), (128, 32)])
def test_region_pixel_anchors_are_cells_times_net_over_grid_rounded_once(tmp_path, hw):
    """a * cfg_net / grid in float64, one rounding to float32: after the decode's division by the cfg's net size that is
    Darknet's exp(tw) * a / grid.  The cfg's own net size (64 x 64) enters, whatever size the plan runs at."""
    blocks, net_info = _blocks(_write(tmp_path, mini_cfg()))
    h, w = hw
    yolo = build_plan(blocks, net_info, 1, h, w, 4)["ops"][-1]
    gh, gw = h // 8, w // 8
    for (aw, ah), (cw, ch) in zip(yolo["anchors"], ANCHORS):
        assert np.float32(aw) == aw and np.float32(ah) == ah            # float32 values already
        assert aw == float(np.float32(np.float64(cw) * 64 / gw)) and ah == float(np.float32(np.float64(ch) * 64 / gh))


def test_decode_flags_of_a_region_head_do_not_depend_on_the_scores_mode(tmp_path):
    from yolov3.darknet import yolo_decode_flags
    blocks, net_info = _blocks(_write(tmp_path, mini_cfg()))
    yolo = build_plan(blocks, net_info, 1, 64, 64, 4)["ops"][-1]
    assert yolo_decode_flags(yolo, "reference") == (0, 0) and yolo_decode_flags(yolo, "darknet") == (0, 0)
    cfg = _write(tmp_path, mini_cfg())
    assert yolov3.Darknet(cfg, scores="darknet").scores == "darknet"
    assert yolov3.Darknet(cfg).nms_hint is None


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("text,match", [
    (mini_cfg(reorg="[reorg]\nstride=2\nreverse=1\n\n"), r"reorg block 9: reverse=1"),
    (mini_cfg(reorg="[reorg3d]\nstride=2\nreverse=1\n\n"), r"reorg3d block 9: reverse=1"),
    (mini_cfg(region_extra="softmax_tree=data/9k.tree\n"), r"region block 13: softmax_tree"),
    (mini_cfg(region_extra="tree=data/9k.tree\n"), r"region block 13: tree"),
    (mini_cfg(region_extra="softmax=0\n"), r"region block 13: softmax=0"),
    (mini_cfg(drop=("softmax",)), r"region block 13: softmax=0"),
    (mini_cfg(region_extra="coords=5\n"), r"region block 13: coords=5"),
    (mini_cfg(num=9, classes=1), r"region block 13: num=9"),
    (mini_cfg(head_filters=126), r"region block 13: .*filters = num \* \(5 \+ classes\) = 125"),
])
def test_refusals_name_block_and_key(tmp_path, text, match):
    cfg = _write(tmp_path, text)
    with pytest.raises(ValueError, match=match):
        yolov3.Darknet(cfg)
    blocks, net_info = _blocks(cfg)
    with pytest.raises(ValueError, match=match):
        infer_shapes(blocks, net_info, 64, 64)


def test_reorg_refuses_sizes_its_stride_does_not_divide(tmp_path):
    blocks, net_info = _blocks(_write(tmp_path, mini_cfg()))
    with pytest.raises(ValueError, match=r"reorg block 9: stride=2 does not divide the 9x9 map"):
        infer_shapes(blocks, net_info, 36, 36)
    text = mini_cfg().replace(_conv(8, 1), _conv(6, 1))
    blocks, net_info = _blocks(_write(tmp_path, text, "c6.cfg"))
    with pytest.raises(ValueError, match=r"reorg block 9: 6 channels"):
        infer_shapes(blocks, net_info, 64, 64)
    blocks, net_info = _blocks(_write(tmp_path, text.replace("[reorg]", "[reorg3d]"), "c6_3d.cfg"))
    assert infer_shapes(blocks, net_info, 64, 64)[9] == (24, 8, 8)     # the 3d form has no such condition


def test_multi_label_on_a_region_head_is_refused(tmp_path):
    cfg = _write(tmp_path, mini_cfg())
    for scores in ("reference", "darknet"):
        with pytest.raises(ValueError, match=r"region block 13: multi_label"):
            yolov3.Darknet(cfg, scores=scores, multi_label=True)


# ------------------------------------------------------------------ C ABI

def test_library_reports_reorg_and_a_stale_one_is_refused(monkeypatch):
    lib = _hip.lib()
    assert (_hip.OP_REORG, _hip.F_REORG_3D, _hip.CAP_REORG) == (7, 4096, 1024)
    assert lib.y3_capabilities() & 1024 and _hip.capabilities() & _hip.CAP_REORG
    assert ctypes.sizeof(_hip.Y3Op) == 248 and _hip.ABI_VERSION == 6 and lib.y3_abi_version() == 6
    monkeypatch.setattr(_hip, "capabilities", lambda: _hip.CAP_REORG - 1)
    with pytest.raises(_hip.HipLibraryError, match=r"yolov2.cfg: .* cannot compute reorg "):
        _hip.require_capabilities(_hip.CAP_REORG | _hip.CAP_MISH, "yolov2.cfg")
    _hip.require_capabilities(_hip.CAP_MISH, "yolov4.cfg")


def _reorg_op(c=8, h=4, w=6, s=2, flags=0, kind=None, **over):
    op = _hip.Y3Op()
    op.kind = _hip.OP_REORG if kind is None else kind
    op.dtype, op.flags, op.batch, op.block_idx = _hip.Y3_BF16, flags, 2, 27
    op.in_c, op.in_h, op.in_w, op.in_ld = c, h, w, c
    op.out_c, op.out_h, op.out_w, op.out_ld = c * s * s, h // max(s, 1), w // max(s, 1), c * s * s
    op.ksize, op.stride = 1, s
    op.d_in, op.d_out = 0x10000, 0x20000          # never dereferenced: plans are only created here
    for key, val in over.items():
        setattr(op, key, val)
    return op


def _create(op):
    lib = _hip.lib()
    ops = (_hip.Y3Op * 1)(op)
    handle = ctypes.c_void_p()
    rc = lib.y3_plan_create_ex(ops, 1, ctypes.c_void_p(0x1000), None, ctypes.byref(handle))
    if rc != 0:
        return rc, lib.y3_last_error().decode()
    name = lib.y3_plan_op_kernel(handle, 0).decode()
    lib.y3_plan_destroy(handle)
    return 0, name


def test_plan_creation_validates_reorg_ops_and_names_the_block():
    assert _create(_reorg_op()) == (0, "reorg_bf16")
    assert _create(_reorg_op(flags=_hip.F_REORG_3D)) == (0, "reorg3d_bf16")
    assert _create(_reorg_op(c=6, flags=_hip.F_REORG_3D)) == (0, "reorg3d_bf16")
    assert _create(_reorg_op(in_ld=16, out_ld=40)) == (0, "reorg_bf16")
    for op, needle in ((_reorg_op(h=5), "does not divide the 5 x 6 map"),
                       (_reorg_op(w=7), "does not divide the 4 x 7 map"),
                       (_reorg_op(c=6), "6 channels are not a multiple of stride^2 = 4"),
                       (_reorg_op(s=0), "stride 0"),
                       (_reorg_op(out_c=16), "output shape mismatch"),
                       (_reorg_op(out_h=4), "output shape mismatch"),
                       (_reorg_op(in_ld=7), "pixel stride below the channel count"),
                       (_reorg_op(out_ld=31), "pixel stride below the channel count")):
        rc, msg = _create(op)
        assert rc != 0 and msg.startswith("reorg block 27: ") and needle in msg, msg
    rc, msg = _create(_reorg_op(kind=_hip.OP_COPY, flags=_hip.F_REORG_3D, out_c=8, out_h=4, out_w=6))
    assert rc != 0 and "block 27: Y3_F_REORG_3D on an op of kind 5" in msg


# ------------------------------------------------------------------ weight files

def test_weights_header_of_four_and_of_five_words(tmp_path):
    """Darknet 0.1 files (the published yolov2 weights) carry major, minor, revision and a 32-bit `seen`; from 0.2 on `seen` has
    64 bits.  The same parameters behind either header load identically."""
    blocks, net_info = _blocks(_write(tmp_path, mini_cfg()))
    params = W.synth_params(blocks, net_info, seed=3)
    new, old = str(tmp_path / "v02.weights"), str(tmp_path / "v01.weights")
    W.write_darknet_weights(new, params)
    W.write_darknet_weights(old, params, header=np.array([0, 1, 0, 32013312], dtype=np.int32))
    n = W.stream_length(blocks, net_info)
    assert os.path.getsize(new) == 20 + 4 * n and os.path.getsize(old) == 16 + 4 * n
    h_new, p_new = W.read_darknet_weights(new, blocks, net_info)
    h_old, p_old = W.read_darknet_weights(old, blocks, net_info)
    assert h_new.tolist() == [0, 2, 0, 0, 0] and h_old.tolist() == [0, 1, 0, 32013312]
    assert h_new.dtype == h_old.dtype == np.int32
    assert len(p_new) == len(p_old) == len(params)
    for a, b, c in zip(p_new, p_old, params):
        assert sorted(a) == sorted(b) == sorted(c)
        for key in a:
            assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], c[key]), key
    # major 1 and later, and minor 2 and later, have the 64-bit counter
    for header in ([1, 0, 0, 7, 0], [0, 3, 0, 7, 0]):
        path = str(tmp_path / "h.weights")
        W.write_darknet_weights(path, params, header=np.array(header, dtype=np.int32))
        got, p = W.read_darknet_weights(path, blocks, net_info)
        assert got.tolist() == header and np.array_equal(p[-1]["weight"], params[-1]["weight"])
    net = yolov3.Darknet(_write(tmp_path, mini_cfg(), "again.cfg")).load_weights(old)
    assert net.header.tolist() == [0, 1, 0, 32013312] and np.array_equal(net._params[0]["weight"], params[0]["weight"])


# ------------------------------------------------------------------ the restatement

def _ramp(b, c, h, w):
    return np.arange(b * c * h * w, dtype=np.int64).reshape(b, c, h, w)


@pytest.mark.parametrize("chw,s", [((4, 2, 2), 2), ((8, 4, 6), 2), ((12, 6, 4), 2), ((16, 8, 8), 4), ((64, 26, 26), 2)])
def test_restated_flat_reorg_is_a_bijection(chw, s):
    x = _ramp(2, *chw)
    y = R.reorg_flat(x, s)
    c, h, w = chw
    assert y.shape == (2, c * s * s, h // s, w // s)
    for b in range(2):
        assert np.array_equal(np.sort(y[b].ravel()), x[b].ravel())        # every element of the frame, once
    assert np.array_equal(y[1] - y[0], np.full(y[0].shape, c * h * w))  # the same permutation for every frame


@pytest.mark.parametrize("chw,s", [((4, 2, 2), 2), ((8, 4, 6), 2), ((12, 6, 4), 2), ((16, 8, 8), 4), ((6, 4, 4), 2)])
def test_restated_reorg3d_is_the_reshape_permute_space_to_depth(chw, s):
    c, h, w = chw
    x = _ramp(2, c, h, w)
    want = x.reshape(2, c, h // s, s, w // s, s).transpose(0, 3, 5, 1, 2, 4).reshape(2, s * s * c, h // s, w // s)
    assert np.array_equal(R.reorg_3d(x, s), want)


@pytest.mark.parametrize("chw,s", [((4, 2, 2), 2), ((8, 4, 6), 2), ((64, 26, 26), 2), ((16, 8, 8), 4)])
def test_the_two_restated_forms_differ(chw, s):
    x = _ramp(1, *chw)
    a, b = R.reorg_flat(x, s), R.reorg_3d(x, s)
    assert a.shape == b.shape and not np.array_equal(a, b)


def test_restated_flat_reorg_by_hand():
    """(4, 2, 2), s = 2: oc = 1, so c2 = 0 and off = k; the source of out_flat[i + 2 (j + 2 k)] is in_flat[(2 i + k % 2) +
    4 (2 j + k / 2)]: the input read as ONE 4 x 4 image and sampled with stride 2 from offset (k / 2, k % 2)."""
    x = _ramp(1, 4, 2, 2)
    img = x.reshape(4, 4)
    want = np.stack([img[k // 2::2, k % 2::2] for k in range(4)]).reshape(1, 16, 1, 1)
    assert np.array_equal(R.reorg_flat(x, 2), want)


def test_restated_region_decode_by_hand():
    """one cell of a 1 x 2 grid, one anchor, two classes, in float64 by hand"""
    t = torch.tensor([0.3, -0.2, 0.5, -0.4, 1.2, 2.0, 0.5], dtype=torch.float32)
    x = torch.zeros(1, 7, 1, 2)
    x[0, :, 0, 1] = t
    box, prob, cls = R.region_decode(x, [(1.5, 2.25)])
    sig = lambda v: 1.0 / (1.0 + np.exp(-v))      # noqa: E731
    want = [(1 + sig(0.3)) / 2, (0 + sig(-0.2)) / 1, np.exp(0.5) * 1.5 / 2, np.exp(-0.4) * 2.25 / 1]
    np.testing.assert_allclose(box[0, 1].numpy(), want, rtol=1e-6)
    np.testing.assert_allclose(float(prob[0, 1]), sig(1.2) * np.exp(2.0) / (np.exp(2.0) + np.exp(0.5)), rtol=1e-6)
    assert int(cls[0, 1]) == 0 and box.shape == (1, 2, 4)


# ------------------------------------------------------------------ the shipped cfgs

def _header_count(path):
    with open(path) as fh:
        head = "".join(line for line in fh if line.startswith("#"))
    return int(re.search(r"Weight stream this cfg describes: (\d+) float32 values", head).group(1))


@pytest.mark.parametrize("path,dim,other,n_blocks,floats", [(V2, 608, 320, 32, 50983561), (V2_TINY, 416, 608, 16, 11237145)])
def test_shipped_cfgs_plan_and_describe_the_counted_weight_stream(path, dim, other, n_blocks, floats):
    blocks, net_info = _blocks(path)
    assert len(blocks) == n_blocks and net_info["width"] == net_info["height"] == dim
    assert W.stream_length(blocks, net_info) == _header_count(path) == floats
    head, region = blocks[-2], blocks[-1]
    assert region["type"] == "region" and head["filters"] == 425 and head["activation"] == "linear"
    assert "batch_normalize" not in head and (region["num"], region["classes"]) == (5, 80)
    for size in (dim, other):
        g = size // 32
        for es in (4, 2):
            d = build_plan(blocks, net_info, 2, size, size, es, reuse=True, fuse=True)
            assert d["rows_total"] == 5 * g * g and d["shapes"][-1] == (425, g, g)
            yolo = d["ops"][-1]
            assert yolo["kind"] == "yolo" and yolo["n_attr"] == 85 and yolo["inp"].f32 and yolo["inp"].ld == 432
            assert yolo["anchors"][0] == (float(np.float32(0.57273 * dim / g)), float(np.float32(0.677385 * dim / g)))
            assert not [o for o in d["ops"] if o["kind"] == "copy"]
    net = yolov3.Darknet(path)
    assert len(net._convs) == sum(b["type"] == "convolutional" for b in blocks)


def test_yolov2_pass_through_layout():
    blocks, net_info = _blocks(V2)
    assert [i for i, b in enumerate(blocks) if b["type"] == "reorg"] == [27] and blocks[27]["stride"] == 2
    assert blocks[25]["layers"] == [16] and blocks[28]["layers"] == [27, 24]
    assert (blocks[26]["filters"], blocks[26]["size"]) == (64, 1)
    shapes = infer_shapes(blocks, net_info, 416, 416)
    assert shapes[26] == (64, 26, 26) and shapes[27] == (256, 13, 13) and shapes[28] == (1280, 13, 13)
    d = build_plan(blocks, net_info, 1, 416, 416, 2)
    ro = next(o for o in d["ops"] if o["kind"] == "reorg")
    assert (ro["out"].buf, ro["out"].off, ro["out"].c, ro["out"].ld) == ("cat28", 0, 256, 1280)


def test_yolov2_tiny_ends_in_the_stride_1_pool():
    blocks, net_info = _blocks(V2_TINY)
    assert (blocks[11]["type"], blocks[11]["size"], blocks[11]["stride"]) == ("maxpool", 2, 1)
    for pool in ("reference", "darknet"):
        shapes = infer_shapes(blocks, net_info, 416, 416, pool)
        assert shapes[10] == (512, 13, 13) and shapes[11] == (512, 13, 13) and shapes[-1] == (425, 13, 13)
