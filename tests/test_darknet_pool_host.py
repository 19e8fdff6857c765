"""Darknet max-pool semantics without a GPU: the witness (tests/darknet_pool_restate.py) pinned against itself and against
torch's centred pool, the size formula in ``plan.infer_shapes``, and the plumbing of ``pool="darknet"`` from the command line
down to the C ABI's op."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import yolov3
from yolov3 import _hip, plan
from yolov3.__main__ import build_parser, main
from yolov3.cfgparse import parse_config
from yolov3.darknet import fill_maxpool_op

import darknet_pool_restate as DP
from golden_util import MODEL_DIR

MAPS = [(13, 13), (16, 16), (19, 19), (20, 20), (17, 22)]
SHIPPED = {"yolov3": 608, "yolov3-spp": 608, "yolov3-tiny": 416, "yolov4": 608, "yolov4-tiny": 416, "yolov4-csp": 512}


def _signed(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float32)


# ---- the witness ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", MAPS)
@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("k", [2, 3, 5, 9, 13])
def test_witness_loop_equals_padded_torch_pool(k, s, hw):
    x = _signed((2, 3) + hw, 100 * k + 10 * s + hw[0])
    a, b = DP.pool_loop(x, k, s), DP.pool(x, k, s)
    assert a.shape == b.shape == (2, 3, (hw[0] + k - 1 - k) // s + 1, (hw[1] + k - 1 - k) // s + 1)
    assert torch.equal(a, b)
    assert torch.isfinite(b).all()              # every window holds a tap
    if k % 2 == 1 and s == 1:
        assert torch.equal(b, F.max_pool2d(x, k, 1, k // 2))


@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (3, 2, 1), (3, 1, 0), (5, 1, 2), (2, 1, 2)])
def test_witness_with_an_explicit_padding(k, s, p):
    x = _signed((1, 2, 15, 18), k + s + p)
    assert torch.equal(DP.pool_loop(x, k, s, p), DP.pool(x, k, s, p))


def test_witness_differs_from_the_reference_pool():
    """About three quarters of a 5 x 5 pool's outputs differ from the zero-padded down-right pool; on an all-negative map
    the border differs for certain (0.0 against a negative maximum)."""
    from oracle import darknet_oracle as orc
    x = _signed((1, 4, 19, 19), 3)
    frac = float((DP.pool(x, 5, 1) != orc.maxpool(x, 5, 1)).float().mean())
    assert 0.6 < frac < 0.9, frac
    neg = -x.abs() - 1.0
    assert (orc.maxpool(neg, 2, 1)[:, :, -1, :] == 0).all() and (DP.pool(neg, 2, 1)[:, :, -1, :] < 0).all()
    assert torch.equal(DP.pool(x, 2, 1)[:, :, :-1, :-1], orc.maxpool(x, 2, 1)[:, :, :-1, :-1])


# ---- shapes ----------------------------------------------------------------------------------------------------------------

def _blocks(path):
    blocks, net_info = parse_config(str(path))
    for i, blk in enumerate(blocks):
        if blk["type"] == "route":
            blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
    return blocks, net_info


@pytest.mark.parametrize("model", sorted(SHIPPED))
def test_shipped_cfgs_keep_their_shapes_at_their_own_size(model):
    blocks, net_info = _blocks(os.path.join(MODEL_DIR, model + ".cfg"))
    dim = SHIPPED[model]
    assert net_info["width"] == net_info["height"] == dim
    assert plan.infer_shapes(blocks, net_info, dim, dim, pool="darknet") == plan.infer_shapes(blocks, net_info, dim, dim)


THREE_BLOCKS = """[net]
width=32
height=32
channels=3

[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky

[maxpool]
size=2
stride=2
{extra}
[convolutional]
batch_normalize=1
filters=8
size=3
stride=1
pad=1
activation=leaky
"""


def _three(tmp_path, extra=""):
    path = tmp_path / "three.cfg"
    path.write_text(THREE_BLOCKS.format(extra=extra + "\n" if extra else ""))
    return path


def test_stride2_pool_of_an_odd_map_is_one_larger_in_darknet_mode(tmp_path):
    blocks, net_info = _blocks(_three(tmp_path))
    # 27 x 21 map: Darknet (27 + 1) / 2 = 14 and (21 + 1) / 2 = 11; the reference (27 - 2) / 2 + 1 = 13 and (21 - 2) / 2 + 1 = 10
    assert plan.infer_shapes(blocks, net_info, 27, 21, pool="darknet") == [(8, 27, 21), (8, 14, 11), (8, 14, 11)]
    assert plan.infer_shapes(blocks, net_info, 27, 21) == [(8, 27, 21), (8, 13, 10), (8, 13, 10)]
    assert plan.infer_shapes(blocks, net_info, 27, 21, pool="reference") == [(8, 27, 21), (8, 13, 10), (8, 13, 10)]
    # even maps: the same either way
    assert plan.infer_shapes(blocks, net_info, 32, 32, pool="darknet") == plan.infer_shapes(blocks, net_info, 32, 32)


def test_padding_key_is_read_in_darknet_mode_only(tmp_path):
    blocks, net_info = _blocks(_three(tmp_path, "padding=0"))
    assert plan.infer_shapes(blocks, net_info, 27, 27, pool="darknet")[1] == (8, 13, 13)      # (27 + 0 - 2) / 2 + 1
    assert plan.infer_shapes(blocks, net_info, 27, 27)[1] == (8, 13, 13)
    d = plan.build_plan(blocks, net_info, 1, 27, 27, 4, pool="darknet")
    assert [op["pad"] for op in d["ops"] if op["kind"] == "maxpool"] == [0]


def test_tiny_at_424_builds_by_default_and_is_refused_in_darknet_mode():
    """53 -> 26 -> 13 -> upsample 26 = 26 at the route by default; Darknet pools 53 -> 27 -> 14 -> upsample 28 against 27."""
    blocks, net_info = _blocks(os.path.join(MODEL_DIR, "yolov3-tiny.cfg"))
    shapes = plan.infer_shapes(blocks, net_info, 424, 424)
    assert (shapes[6][1], shapes[7][1]) == (53, 26)
    with pytest.raises(ValueError, match="route block 20"):
        plan.infer_shapes(blocks, net_info, 424, 424, pool="darknet")


def test_a_window_without_a_tap_is_refused(tmp_path):
    blocks, net_info = _blocks(_three(tmp_path, "padding=6"))        # padding / 2 = 3 > size - 1: the first window is all padding
    with pytest.raises(ValueError, match="maxpool block 1"):
        plan.infer_shapes(blocks, net_info, 32, 32, pool="darknet")
    plan.infer_shapes(blocks, net_info, 32, 32)                        # the default does not read the key


@pytest.mark.parametrize("extra,word", [("maxpool_depth=1", "maxpool_depth"), ("antialiasing=1", "antialiasing"),
                                        ("stride_x=1", "stride_x"), ("stride_y=3", "stride_y")])
def test_other_darknet_pools_are_refused_naming_the_block(tmp_path, extra, word):
    path = _three(tmp_path, extra)
    blocks, net_info = _blocks(path)
    for mode in plan.POOL_MODES:
        with pytest.raises(ValueError, match="maxpool block 1.*" + word):
            plan.infer_shapes(blocks, net_info, 32, 32, pool=mode)
    with pytest.raises(ValueError, match="maxpool block 1"):
        yolov3.Darknet(str(path), pool="darknet")
    ok = _three(tmp_path, "stride_x=2\nstride_y=2")                    # the same stride spelled three times is fine
    yolov3.Darknet(str(ok), pool="darknet")


# ---- plumbing --------------------------------------------------------------------------------------------------------------

def test_abi_additions():
    assert ctypes.sizeof(_hip.Y3Op) == 248 and _hip.ABI_VERSION == 6
    assert (_hip.F_POOL_DARKNET, _hip.CAP_POOL_DARKNET) == (1024, 32)
    assert _hip.lib().y3_capabilities() & 32


def test_stale_library_is_refused(monkeypatch):
    monkeypatch.setattr(_hip, "capabilities", lambda: 31)              # everything but bit 32
    with pytest.raises(_hip.HipLibraryError, match="Darknet max-pooling"):
        _hip.require_capabilities(_hip.CAP_MISH | _hip.CAP_POOL_DARKNET, "yolov4.cfg")
    _hip.require_capabilities(_hip.CAP_MISH, "yolov4.cfg")


def test_pool_argument_of_darknet():
    cfg = os.path.join(MODEL_DIR, "yolov3-spp.cfg")
    assert yolov3.Darknet(cfg).pool == "reference"
    assert yolov3.Darknet(cfg, pool="reference").pool == "reference"
    net = yolov3.Darknet(cfg, pool="darknet")
    assert net.pool == "darknet"
    with pytest.raises(AttributeError):
        net.pool = "reference"                                          # fixed by the constructor
    for bad in ("x", "Darknet", None, 1):
        with pytest.raises(ValueError, match="pool="):
            yolov3.Darknet(cfg, pool=bad)


@pytest.mark.parametrize("model", ["yolov3-spp", "yolov3-tiny", "yolov4-csp"])
def test_maxpool_ops_carry_the_mode(model):
    net = yolov3.Darknet(os.path.join(MODEL_DIR, model + ".cfg"), pool="darknet")
    dim = SHIPPED[model]
    dk = plan.build_plan(net.blocks, net.net_info, 2, dim, dim, 2, pool=net.pool)
    ref = plan.build_plan(net.blocks, net.net_info, 2, dim, dim, 2)
    pools = [op for op in dk["ops"] if op["kind"] == "maxpool"]
    assert len(pools) == sum(b["type"] == "maxpool" for b in net.blocks) > 0
    for od in pools:
        assert od["pool"] == "darknet" and od["pad"] == od["ksize"] - 1
        op = _hip.Y3Op()
        assert fill_maxpool_op(op, od) == _hip.CAP_POOL_DARKNET
        assert op.kind == _hip.OP_MAXPOOL and op.flags & _hip.F_POOL_DARKNET and op.pad == od["ksize"] - 1
        assert (op.ksize, op.stride) == (od["ksize"], od["stride"])
    for od in [op for op in ref["ops"] if op["kind"] == "maxpool"]:
        assert "pool" not in od and "pad" not in od
        op = _hip.Y3Op()
        assert fill_maxpool_op(op, od) == 0
        assert op.kind == _hip.OP_MAXPOOL and op.flags == 0 and op.pad == 0
    assert not any("pool" in op for op in dk["ops"] if op["kind"] != "maxpool")
    # same graph, same buffers: only the pools' rule differs at the cfg's own size
    assert dk["offsets"] == ref["offsets"] and dk["arena_bytes"] == ref["arena_bytes"] and dk["shapes"] == ref["shapes"]


def test_command_line_flag_reaches_darknet(monkeypatch):
    args = build_parser().parse_args(["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg", "--darknet-pool"])
    assert args.darknet_pool is True
    assert build_parser().parse_args(["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg"]).darknet_pool is False

    class Seen(Exception):
        pass

    def fake(*a, **kw):
        raise Seen(kw.get("pool"))

    monkeypatch.setattr(yolov3, "Darknet", fake)
    with pytest.raises(Seen, match="darknet"):
        main(["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg", "--darknet-pool"])
    with pytest.raises(Seen, match="reference"):
        main(["-c", "a.cfg", "-w", "a.weights", "-I", "x.jpg", "--letterbox"])
