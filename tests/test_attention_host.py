"""Darknet's attention blocks without a GPU: [avgpool], [scale_channels] and [sam].  The restatements (tests/attention_restate.py,
tests/attention_ordered.py) held to torch and to each other; every refusal with its message; the C ABI's new kinds and capability;
plan creation on fabricated addresses; the weight stream of tests/golden/cfg/attention.cfg against a count by hand; its plan, executed
literally on a NaN-filled arena, bit-equal to a forward by block index; and the code objects and census of libyolov3_hip_attn.so."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.plan import build_plan, infer_shapes
from yolov3.plan_ops import fill_ops

import attention_interp as AI
import attention_ordered as AO
import attention_restate as AR
import attention_util as AU
import code_object
import kernel_census as census
import kernel_choice_util as kc
import plan_interp as PI
from golden_util import GOLDEN, ROOT

CFG = os.path.join(GOLDEN, "cfg", "attention.cfg")
no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")
ATTENTION_BLOCKS = {2: "avgpool", 5: "scale_channels", 8: "avgpool", 11: "scale_channels", 15: "scale_channels", 19: "sam", 22: "sam"}

HEAD = "[net]\nwidth=32\nheight=32\nchannels=3\n\n[convolutional]\nbatch_normalize=1\nfilters=16\nsize=3\nstride=1\npad=1\nactivation=leaky\n\n"
TAIL = ("[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n\n[yolo]\nmask=0,1,2\nanchors=6,8, 12,10, 20,24\n"
        "classes=1\nnum=3\n")


def _conv(filters, act="leaky", size=1):
    return "[convolutional]\nbatch_normalize=1\nfilters=%d\nsize=%d\nstride=1\npad=1\nactivation=%s\n\n" % (filters, size, act)


def _write(tmp_path, text, name="attn.cfg"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def _blocks(path):
    blocks, net_info = parse_config(path)
    return PI.abs_routes(blocks), net_info


# ---------------------------------------------------------------------------------------------- the restatements

@pytest.mark.parametrize("shape", [(2, 5, 1, 1), (1, 7, 1, 5), (3, 8, 13, 10), (2, 20, 19, 19)])
def test_restated_avgpool_is_adaptive_avg_pool2d_in_float64(shape):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape)), dtype=torch.float64)
    got = AR.avgpool(x)
    want = F.adaptive_avg_pool2d(x, 1)
    assert got.dtype == torch.float64 and got.shape == want.shape == (shape[0], shape[1], 1, 1)
    torch.testing.assert_close(got, want, rtol=1e-14, atol=1e-15)
    assert AR.avgpool(x.float(), torch.float32).dtype == torch.float32


def test_restated_products_are_plain_broadcasting():
    g = torch.Generator().manual_seed(5)
    src, gate, mask = torch.randn((2, 6, 4, 3), generator=g), torch.randn((2, 6, 1, 1), generator=g), torch.randn((2, 6, 4, 3), generator=g)
    for dt in (torch.float64, torch.float32):
        assert torch.equal(AR.scale_channels(src, gate, dt), src.to(dt) * gate.to(dt))
        assert torch.equal(AR.sam(src, mask, dt), src.to(dt) * mask.to(dt))
        assert AR.scale_channels(src, gate, dt).shape == src.shape
    with pytest.raises(AssertionError):
        AR.scale_channels(src, mask)
    with pytest.raises(AssertionError):
        AR.sam(src, gate)


def test_ordered_sum_by_hand():
    """P = 35, one channel, powers of two spread so that the order shows: by the rule partial 0 = x0 + x32, partial 1 = x1 + x33,
    partial 2 = x2 + x34, and the tree adds s[r + 16] first."""
    x = np.zeros((35, 1), dtype=np.float32)
    x[0], x[32], x[16] = 2.0 ** 24, 1.0, 1.0
    # s[0] = 2^24 + 1 -> 2^24 (rounded, tie to even); + s[16] = 1 -> 2^24 again.  Sequential float64: 2^24 + 2.
    assert AO.ordered_sum(x)[0] == np.float32(2.0 ** 24)
    y = np.zeros((35, 1), dtype=np.float32)
    y[0], y[16], y[8] = 2.0 ** 24, 1.0, 1.0
    # s[0] = 2^24; + s[16] = 1 -> 2^24 (tie to even); s[8] stays 1 and arrives at the +8 step: 2^24 + 1 -> 2^24
    assert AO.ordered_sum(y)[0] == np.float32(2.0 ** 24)
    z = np.zeros((64, 1), dtype=np.float32)
    z[16], z[48], z[0] = 1.0, 1.0, 2.0 ** 24
    # partial 16 = x16 + x48 = 2, then s[0] += s[16]: 2^24 + 2, exactly
    assert AO.ordered_sum(z)[0] == np.float32(2.0 ** 24 + 2.0)


@pytest.mark.parametrize("p", [1, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 130, 361])
def test_ordered_sum_is_a_sum_and_sees_the_order(p):
    rng = np.random.default_rng(p)
    x = (rng.standard_normal((p, 64)) * 3).astype(np.float32)
    got = AO.ordered_sum(x).astype(np.float64)
    exact = x.astype(np.float64).sum(axis=0)
    assert (np.abs(got - exact) <= p * 2.0 ** -24 * np.abs(x).astype(np.float64).sum(axis=0)).all()      # (n - 1) u sum|x|
    ints = rng.integers(-128, 129, size=(p, 64)).astype(np.float32)
    for f in (AO.ordered_sum, AO.wrong_sixteen_lane_sum, AO.wrong_sequential_sum):
        assert np.array_equal(f(ints).astype(np.int64), ints.astype(np.int64).sum(axis=0))      # exact in any order
    if p >= 63:
        assert not np.array_equal(AO.ordered_sum(x), AO.wrong_sixteen_lane_sum(x))
        assert not np.array_equal(AO.ordered_sum(x), AO.wrong_sequential_sum(x))


@pytest.mark.parametrize("dtype", AU.DTYPES)
def test_gpu_inputs_fit_their_gates_on_the_cpu(dtype):
    """what tests/test_gpu_attention.py asks of the device holds for the ordered restatement on the same inputs: inside the derived
    gate of the float64 mean; and the integer inputs keep every partial sum below 2^24"""
    for shape in ((3, 13, 10, 24), (1, 76, 76, 8), (2, 1, 129, 13)):
        x = AU.random_storage(shape, dtype, 7)
        got = AU.avgpool_ordered_expected(x, dtype).astype(np.float64)
        mean = AR.avgpool(torch.from_numpy(x).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
        assert (np.abs(got - mean) <= AU.avgpool_gate(x, dtype)).all(), (dtype, shape)
        ints = AU.integer_storage(shape, dtype, 7)
        assert np.array_equal(AU.to_storage(ints, dtype), ints)                                    # held exactly by the type
        assert np.abs(ints).astype(np.int64).reshape(shape[0], -1, shape[3]).sum(axis=1).max() < 2 ** 24
        s = ints.astype(np.int64).reshape(shape[0], -1, shape[3]).sum(axis=1)
        exact = AU.to_storage((s.astype(np.float32) / np.float32(shape[1] * shape[2])), dtype).reshape(shape[0], 1, 1, shape[3])
        assert AU.same_bits(AU.avgpool_ordered_expected(ints, dtype), exact).all()


def test_product_expectation_rounds_once():
    """rnd64 of the float64 product against torch's float32 product narrowed once (exact for 16-bit operands), on values that
    tie, overflow fp16, underflow, and on zeros of both signs, infinities and NaN"""
    vals = np.array([0.0, -0.0, 1.0, -1.5, 3.0, 255.0, 257.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, 1.0 + 2.0 ** -7,
                     np.inf, -np.inf, np.nan, 0.333251953125, 1.0009765625], dtype=np.float32)
    a, b = np.repeat(vals, vals.size), np.tile(vals, vals.size)
    for dtype, tdt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        a16, b16 = AU.to_storage(a, dtype), AU.to_storage(b, dtype)
        want = (torch.from_numpy(a16) * torch.from_numpy(b16)).to(tdt).float().numpy()
        assert AU.same_bits(AU.product_expected(a16, b16, dtype), want).all(), dtype
    got = AU.product_expected(a, b, "float32")
    with np.errstate(all="ignore"):
        assert AU.same_bits(got, a * b).all()
    assert np.signbit(AU.product_expected(np.float32([0.0]), np.float32([-2.0]), "bf16"))[0]
    assert np.isnan(AU.product_expected(np.float32([0.0]), np.float32([np.inf]), "fp16"))[0]


# ---------------------------------------------------------------------------------------------- refusals

SE = _conv(16) + "[avgpool]\n\n" + _conv(4) + _conv(16, "logistic")          # blocks 1-4 behind HEAD's block 0


@pytest.mark.parametrize("body,msg", [
    (SE + "[scale_channels]\nfrom=-4\nscale_wh=1\n\n", r"scale_channels block 5: scale_wh=1 is not supported"),
    (SE + "[scale_channels]\nfrom=-4\nactivation=leaky\n\n", r"scale_channels block 5: activation 'leaky' is not supported \(linear only\)"),
    (SE + "[scale_channels]\nfrom=-4\nactivation=swish\n\n", r"scale_channels block 5: activation 'swish' is not supported"),
    (_conv(16) + _conv(16, "logistic") + "[sam]\nfrom=-2\nactivation=logistic\n\n", r"sam block 3: activation 'logistic' is not supported"),
    (_conv(16) + _conv(16, "logistic") + "[sam]\nfrom=-2\nscale_wh=1\n\n", r"sam block 3: scale_wh=1 is not supported"),
    (SE + "[scale_channels]\n\n", r"scale_channels block 5: from=None does not name an earlier block"),
    (SE + "[scale_channels]\nfrom=1\n\n", r"scale_channels block 5: from=1 does not name an earlier block"),
    (SE + "[scale_channels]\nfrom=-6\n\n", r"scale_channels block 5: from=-6 does not name an earlier block"),
    # shapes: the message holds both
    (SE + "[scale_channels]\nfrom=-2\n\n", r"scale_channels block 5 scales \(4, 1, 1\) by \(16, 1, 1\)"),
    (_conv(16) + _conv(16, "logistic") + "[scale_channels]\nfrom=-2\n\n", r"scale_channels block 3 scales \(16, 32, 32\) by \(16, 32, 32\)"),
    (_conv(16) + _conv(8, "logistic") + "[sam]\nfrom=-2\n\n", r"sam block 3 multiplies \(16, 32, 32\) by \(8, 32, 32\)"),
    (SE + "[sam]\nfrom=-4\n\n", r"sam block 5 multiplies \(16, 32, 32\) by \(16, 1, 1\)"),
    ("[local_avgpool]\nsize=2\nstride=2\n\n", r"unsupported block type 'local_avgpool' \(block 1\)"),
])
def test_refuses_by_message(tmp_path, body, msg):
    cfg = _write(tmp_path, HEAD + body + TAIL)
    blocks, net_info = _blocks(cfg)
    with pytest.raises(ValueError, match=msg):
        infer_shapes(blocks, net_info, 32, 32)
    with pytest.raises(ValueError, match=msg):
        build_plan(blocks, net_info, 1, 32, 32, 2)
    if "unsupported block type" not in msg and " by " not in msg:
        with pytest.raises(ValueError, match=msg):
            yolov3.Darknet(cfg)


@pytest.mark.parametrize("first", ["[avgpool]\n\n", "[scale_channels]\nfrom=-1\n\n", "[sam]\nfrom=-1\n\n"])
def test_refuses_an_attention_block_as_block_0(tmp_path, first):
    kind = first[1:first.index("]")]
    text = "[net]\nwidth=32\nheight=32\nchannels=3\n\n" + first + _conv(18, "linear") + TAIL
    cfg = _write(tmp_path, text)
    msg = r"%s block 0: only a conv reads the network input" % kind
    with pytest.raises(ValueError, match=msg):
        yolov3.Darknet(cfg)
    blocks, net_info = _blocks(cfg)
    with pytest.raises(ValueError, match=msg):
        build_plan(blocks, net_info, 1, 32, 32, 4)


def test_readers_of_a_head_stay_refused_through_the_new_roles(tmp_path):
    """check_head_readers sees the two inputs of an attention block: a [sam] that reads a [yolo] block, and in the 16-bit modes a
    second reader of a head conv"""
    head = "[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n\n"
    yolo = "[yolo]\nmask=0,1,2\nanchors=6,8, 12,10, 20,24\nclasses=1\nnum=3\n\n"
    blocks, net_info = _blocks(_write(tmp_path, HEAD + head + yolo + "[sam]\nfrom=-2\n\n" + TAIL))
    with pytest.raises(ValueError, match=r"yolo block 2: block 3 \(sam\) reads its output"):
        build_plan(blocks, net_info, 1, 32, 32, 4)
    text = HEAD + head + yolo + "[route]\nlayers=0\n\n" + _conv(18, "logistic") + "[sam]\nfrom=-4\n\n" + TAIL
    blocks, net_info = _blocks(_write(tmp_path, text, "second_reader.cfg"))
    with pytest.raises(ValueError, match=r"conv block 1: block 5 \(sam\) reads the logits of the head conv of yolo block 2"):
        build_plan(blocks, net_info, 1, 32, 32, 2)
    assert build_plan(blocks, net_info, 1, 32, 32, 4)["ops"]                 # float32 runs this graph


@pytest.mark.parametrize("edit,msg", [
    (lambda t: t.replace("activation=leaky", "activation=swish", 1), r"conv block 0: activation 'swish' is not supported"),
    (lambda t: t.replace("pad=1\n", "pad=1\ndilation=2\n", 1), r"conv block 0: dilated convolution \(dilation=2\)"),
    (lambda t: t.replace("[shortcut]\n", "[shortcut]\nweights_type=per_feature\n", 1), r"weighted shortcuts \(weights_type\)"),
    (lambda t: t.replace("[shortcut]\nfrom=-5\nactivation=linear", "[shortcut]\nfrom=-5\nactivation=leaky", 1),
     r"shortcut block 6: activation 'leaky' is not supported"),
])
def test_what_was_refused_stays_refused(tmp_path, edit, msg):
    with open(CFG) as fh:
        text = edit(fh.read())
    cfg = _write(tmp_path, text)
    with pytest.raises(ValueError, match=msg):
        yolov3.Darknet(cfg)
    blocks, net_info = parse_config(cfg)
    with pytest.raises(ValueError, match=msg):
        build_plan(PI.abs_routes(blocks), net_info, 1, 64, 64, 4)


# ---------------------------------------------------------------------------------------------- C ABI

def test_header_constants_and_capability(monkeypatch):
    with open(os.path.join(ROOT, "include", "yolov3_hip.h")) as fh:
        header = fh.read()
    defines = dict(re.findall(r"#define (Y3_\w+) (\d+)u?\b", header))
    assert (int(defines["Y3_OP_AVGPOOL"]), int(defines["Y3_OP_SCALE_CHANNELS"]), int(defines["Y3_OP_SAM"])) == (8, 9, 10)
    assert (_hip.OP_AVGPOOL, _hip.OP_SCALE_CHANNELS, _hip.OP_SAM) == (8, 9, 10)
    assert int(defines["Y3_CAP_ATTENTION"]) == _hip.CAP_ATTENTION == 32768
    assert int(defines["Y3_ABI_VERSION"]) == _hip.ABI_VERSION == 6
    lib = _hip.lib()
    assert lib.y3_capabilities() & 32768 and _hip.capabilities() & _hip.CAP_ATTENTION and lib.y3_abi_version() == 6
    assert ctypes.sizeof(_hip.Y3Op) == 248
    monkeypatch.setattr(_hip, "capabilities", lambda: _hip.CAP_ATTENTION - 1)
    with pytest.raises(_hip.HipLibraryError, match=r"attention.cfg: .* cannot compute attention blocks "):
        _hip.require_capabilities(_hip.CAP_ATTENTION | _hip.CAP_MISH, "attention.cfg")
    _hip.require_capabilities(_hip.CAP_MISH, "yolov4.cfg")


def test_main_library_names_the_attention_library_as_a_dependency():
    with open(code_object.LIB, "rb") as f:
        data = f.read()
    assert b"libyolov3_hip_attn.so" in data and b"$ORIGIN" in data
    assert b"avgpool_kernel" not in data and b"attn_mul_kernel" not in data          # its device code is not in the main library


def _op(kind, c=16, h=13, w=10, batch=3, dtype=None, **over):
    op = _hip.Y3Op()
    op.kind, op.dtype, op.batch, op.block_idx = kind, _hip.Y3_BF16 if dtype is None else dtype, batch, 27
    op.ksize = op.stride = 1
    op.in_c = op.in_ld = op.out_c = op.out_ld = op.res_ld = c
    op.in_h, op.in_w, op.out_h, op.out_w = h, w, h, w
    if kind == _hip.OP_AVGPOOL:
        op.out_h = op.out_w = 1
        op.res_ld = 0
    elif kind == _hip.OP_SCALE_CHANNELS:
        op.in_h = op.in_w = 1
    op.d_in, op.d_out = 0x10000000, 0x20000000          # never dereferenced: plans are only created here
    if kind != _hip.OP_AVGPOOL:
        op.d_res = 0x30000000
    for key, val in over.items():
        setattr(op, key, val)
    return op


def _create(op):
    lib = _hip.lib()
    ops = (_hip.Y3Op * 1)(op)
    handle = ctypes.c_void_p()
    rc = lib.y3_plan_create_ex(ops, 1, ctypes.c_void_p(0x1000), None, ctypes.byref(handle))
    if rc != 0:
        return rc, lib.y3_last_error().decode(), None
    name, dims = lib.y3_plan_op_kernel(handle, 0).decode(), _hip.plan_op_dims(handle, 0)
    lib.y3_plan_destroy(handle)
    return 0, name, dims


@no_gpu
def test_plan_creation_accepts_well_formed_ops_and_answers_their_launch():
    A, S, M = _hip.OP_AVGPOOL, _hip.OP_SCALE_CHANNELS, _hip.OP_SAM
    # 16 bf16 channels = two 16-byte chunks: one workgroup of 32 x 8 threads per frame; 3 * 130 * 2 chunk threads for the products
    assert _create(_op(A)) == (0, "avgpool_bf16", (3, 256, 0))
    assert _create(_op(S)) == (0, "scale_channels_bf16", (4, 256, 0))
    assert _create(_op(M)) == (0, "sam_bf16", (4, 256, 0))
    assert _create(_op(A, dtype=_hip.Y3_F32)) == (0, "avgpool_f32", (3, 256, 0))
    assert _create(_op(M, dtype=_hip.Y3_F16)) == (0, "sam_f16", (4, 256, 0))
    # 72 chunks of 8: nine workgroups a frame; the element form: one channel per column, 13 channels = two workgroups a frame
    assert _create(_op(A, c=576)) == (0, "avgpool_bf16", (27, 256, 0))
    assert _create(_op(A, c=13)) == (0, "avgpool_bf16", (6, 256, 0))
    assert _create(_op(A, d_in=0x10000002)) == (0, "avgpool_bf16", (6, 256, 0))              # base off the grain: 16 elements
    assert _create(_op(A, in_ld=20)) == (0, "avgpool_bf16", (6, 256, 0))                      # stride off the grain
    assert _create(_op(S, c=13)) == (0, "scale_channels_bf16", (20, 256, 0))                  # 3 * 130 * 13 = 5070 elements
    assert _create(_op(M, d_res=0x30000004)) == (0, "sam_bf16", (25, 256, 0))                 # 3 * 130 * 16 = 6240 elements
    assert _create(_op(S, in_ld=24, res_ld=40, out_ld=48)) == (0, "scale_channels_bf16", (4, 256, 0))
    # the launch does not depend on the CU count planned for
    for n in (1, 32, 256):
        with _hip.device_cus(n):
            assert _create(_op(A, c=576)) == (0, "avgpool_bf16", (27, 256, 0))


@no_gpu
def test_plan_creation_refuses_the_bad_ops_by_name():
    A, S, M = _hip.OP_AVGPOOL, _hip.OP_SCALE_CHANNELS, _hip.OP_SAM
    for op, words in (
            (_op(A, out_h=2), "avgpool block 27: output shape mismatch (2 x 1; a global pool gives 1 x 1)"),
            (_op(A, out_c=8), "avgpool block 27: channel count changes (16 in, 8 out)"),
            (_op(S, in_h=13, in_w=10), "scale_channels block 27: shape mismatch: the scale is 16 x 13 x 10, not 16 x 1 x 1"),
            (_op(M, in_h=1, in_w=1), "sam block 27: shape mismatch: 16 x 1 x 1 times 16 x 13 x 10"),
            (_op(M, in_c=8, in_ld=8), "sam block 27: channel count changes (8 in, 16 out)"),
            (_op(M, d_res=None), "sam block 27: no source tensor (d_res)"),
            (_op(S, res_ld=8), "scale_channels block 27: pixel stride of the source below the channel count (8 < 16)"),
            (_op(A, in_ld=8), "avgpool block 27: pixel stride below the channel count"),
            (_op(A, flags=_hip.F_LEAKY), "op for block 27: flags 0x1 on an attention op of kind 8"),
            (_op(S, flags=_hip.F_RESIDUAL), "op for block 27: flags 0x2 on an attention op of kind 9"),
            (_op(M, flags=_hip.F_OUT_F32), "op for block 27: flags 0x4 on an attention op of kind 10"),
            (_op(A, flags=_hip.F_PLAN_INPUT), "op for block 27: flags 0x20 on an attention op of kind 8"),
            (_op(M, flags=_hip.F_POOL_DARKNET), "Y3_F_POOL_DARKNET on an op of kind 10"),
            # the pixel limit, input and output side, and the launch limit
            (_op(A, h=46341, w=46341, batch=1), "op for block 27: 2147488281 input pixels (1 x 46341 x 46341); the limit is 2147483391"),
            (_op(M, h=46341, w=46341, batch=1), "input pixels (1 x 46341 x 46341); the limit is 2147483391"),
            (_op(S, h=46341, w=46341, batch=1), "op for block 27: 2147488281 output pixels (1 x 46341 x 46341); the limit is 2147483391"),
            (_op(M, h=32768, w=32768, batch=1, c=64), "op for block 27: sam_bf16 would be a launch of 8589934592 threads; the limit is 4294967040"),
            (_op(A, h=1, w=1, batch=1 << 21, c=1024), "op for block 27: avgpool_bf16 would be a launch of 8589934592 threads; the limit is 4294967040")):
        rc, err, _ = _create(op)
        assert rc == -1 and words in err, (words, rc, err)
    # just inside both limits
    assert _create(_op(A, h=46340, w=46340, batch=1, c=8))[:2] == (0, "avgpool_bf16")
    assert _create(_op(M, h=32768, w=32767, batch=1, c=32))[:2] == (0, "sam_bf16")


# ---------------------------------------------------------------------------------------------- the cfg

def test_stream_length_and_conv_layout_against_a_count_by_hand():
    blocks, net_info = parse_config(CFG)
    assert len(blocks) == 25 and {i: b["type"] for i, b in enumerate(blocks) if b["type"] in AR.KINDS} == ATTENTION_BLOCKS
    out_ch, convs = W.conv_layout(blocks, net_info)
    # channels by hand: after [scale_channels] / [sam] the count is that of `from`'s block
    assert out_ch == [32, 64, 64, 16, 64, 64, 64, 20, 20, 6, 20, 20, 24, 20, 24, 24, 16, 40, 16, 16, 32, 32, 32, 18, 18]
    # (block, cin, cout, k) of every conv, then Darknet's stream: 4 * cout for a BN conv (1 * cout for the head) + cout * cin * k * k
    by_hand = [(0, 3, 32, 3), (1, 32, 64, 3), (3, 64, 16, 1), (4, 16, 64, 1), (7, 64, 20, 1), (9, 20, 6, 1), (10, 6, 20, 1),
               (12, 20, 24, 3), (14, 20, 24, 1), (16, 24, 16, 1), (18, 40, 16, 1), (20, 16, 32, 3), (21, 32, 32, 1), (23, 32, 18, 1)]
    assert [(c["block_idx"], c["cin"], c["cout"], c["k"]) for c in convs] == by_hand
    floats = sum((1 if b == 23 else 4) * co + co * ci * k * k for b, ci, co, k in by_hand)
    assert floats == 36378 and W.stream_length(blocks, net_info) == floats
    params = W.synth_params(blocks, net_info, seed=1)
    assert len(params) == 14 and sum(p["weight"].size for p in params) == sum(co * ci * k * k for _, ci, co, k in by_hand)


def test_shapes_and_plan_of_the_cfg():
    blocks, net_info = _blocks(CFG)
    shapes = infer_shapes(blocks, net_info, 64, 64)
    assert shapes[1] == (64, 16, 16) and shapes[2] == (64, 1, 1) and shapes[4] == (64, 1, 1) and shapes[5] == (64, 16, 16)
    assert shapes[8] == (20, 1, 1) and shapes[11] == (20, 16, 16) and shapes[15] == (24, 16, 16) and shapes[19] == (16, 16, 16)
    assert infer_shapes(blocks, net_info, 96, 64)[2] == (64, 1, 1)
    for es in (2, 4):
        for reuse in (True, False):
            d = build_plan(blocks, net_info, 2, 64, 64, es, reuse=reuse)
            ops = {o["block"]: o for o in d["ops"]}
            for i, kind in ATTENTION_BLOCKS.items():
                assert ops[i]["kind"] == kind and ops[i]["inp"] is d["tensor_of"][i - 1], i
                assert ("res" in ops[i]) == (kind != "avgpool"), i
                if kind != "avgpool":
                    assert ops[i]["res"] is d["tensor_of"][i + blocks[i]["from"]], i
            # the shortcut behind the scale_channels is an add op of its own; nothing was copied
            assert ops[6]["kind"] == "add" and ops[6]["inp"] is ops[5]["out"] and ops[6]["res"] is ops[1]["out"]
            assert not [o for o in d["ops"] if o["kind"] == "copy"]
            # scale_channels 15 writes its slice of route 17's buffer; sam 19 reads block 16 inside that buffer
            out15, out16 = ops[15]["out"], ops[16]["out"]
            assert (out15.buf, out15.off, out15.c, out15.ld) == ("cat17", 16, 24, 40) and (out16.buf, out16.off, out16.c) == ("cat17", 0, 16)
            assert ops[19]["res"] is out16 and ops[19]["res"].ld == 40 and ops[18]["inp"] is d["tensor_of"][17]
            # the avgpool with two readers: conv 9 and (through route 13) conv 14
            assert ops[9]["inp"] is ops[8]["out"] and ops[14]["inp"] is ops[8]["out"] and 13 not in ops
            # no conv in front of an attention reader is fused with what follows it
            for i in (1, 4, 7, 10, 12, 14, 16, 18, 20, 21):
                assert not ops[i]["fuse_next"] and ops[i]["res"] is None, i
            # both inputs stay alive until the op has run
            first, last = d["live"]
            for n, o in enumerate(d["ops"]):
                for key in ("inp", "res"):
                    t = o.get(key)
                    if t is not None and t.buf != "input":
                        assert first[t.buf] < n <= last[t.buf], (n, key)


@pytest.mark.parametrize("es", [2, 4])
@pytest.mark.parametrize("reuse", [True, False], ids=["arena", "keep_all"])
def test_plan_executed_literally_equals_the_forward_by_block_index(es, reuse):
    """the plan of attention.cfg on a NaN-filled byte arena through the planner's offsets, slices and lifetimes: every block
    bit-equal to the restatement walked by block index -- a slot freed before an attention op has read it, or an output that shares
    bytes with an operand, shows here without a GPU"""
    case = PI.synth_case(CFG, 64, 64, batch=2)
    plan = build_plan(case["blocks"], case["net_info"], 2, 64, 64, es, reuse=reuse, fuse=False)
    assert AI.check_plan(case, plan, es) == 25
    if reuse:
        keep = build_plan(case["blocks"], case["net_info"], 2, 64, 64, es, reuse=False, fuse=False)
        assert plan["arena_bytes"] < keep["arena_bytes"]


def test_the_interpreter_sees_a_slot_freed_too_early():
    """the same plan with block 1's buffer released before scale_channels 5 and shortcut 6 have read it"""
    case = PI.synth_case(CFG, 64, 64, batch=2)
    plan = build_plan(case["blocks"], case["net_info"], 2, 64, 64, 2, reuse=True, fuse=False)
    ops = {o["block"]: o for o in plan["ops"]}
    plan["offsets"][ops[1]["out"].buf] = plan["offsets"][ops[4]["out"].buf]        # t1 where conv 4 writes the gates
    with pytest.raises(PI.PlanError):
        AI.check_plan(case, plan, 2)


@no_gpu
@pytest.mark.parametrize("dtype", ["float32", "bf16", "fp16"])
def test_plan_of_the_cfg_names_the_kernels(dtype):
    net = yolov3.Darknet(CFG, dtype=dtype)
    lib = _hip.lib()
    tag = AU.TAG[net.dtype]
    es = 4 if dtype == "float32" else 2
    desc = build_plan(net.blocks, net.net_info, 2, 64, 64, es)
    fake = kc._Fake(net._convs, es)
    ops, needs, _ = fill_ops(desc, net.net_info, net._convs, net.dtype, 2, "u8", "reference", None, fake)
    assert needs & _hip.CAP_ATTENTION and needs & _hip.CAP_LOGISTIC and needs & _hip.CAP_MISH
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, len(ops), fake(4096), None, ctypes.byref(handle)))
    try:
        for i, op in enumerate(ops):
            kind = ATTENTION_BLOCKS.get(int(op.block_idx))
            name = lib.y3_plan_op_kernel(handle, i).decode()
            if kind is None or op.kind == _hip.OP_CONV:
                assert not any(name.startswith(k) for k in AR.KINDS), (i, name)
                continue
            assert name == "%s_%s" % (kind, tag) and op.kind == AU.KIND_CODE[kind] and op.flags == 0, (i, name)
            grid, block, lds = _hip.plan_op_dims(handle, i)
            vec = 16 // es if op.in_c % (16 // es) == 0 else 1
            if kind == "avgpool":
                assert (op.out_h, op.out_w, op.in_h, op.in_w) == (1, 1, 16, 16)
                assert (grid, block, lds) == (2 * -(-(op.in_c // vec) // 8), 256, 0), (i, grid)
                assert lib.y3_plan_op_bytes(handle, i) == (2 * 256 + 2) * op.in_c * es
            else:
                assert op.d_res and op.res_ld >= op.out_c and (op.out_h, op.out_w) == (16, 16)
                assert (grid, block, lds) == (-(-2 * 256 * (op.out_c // vec) // 256), 256, 0), (i, grid)
                px = 2 * 256
                want = 3 * px * op.out_c * es if kind == "sam" else (2 * px + 2) * op.out_c * es
                assert lib.y3_plan_op_bytes(handle, i) == want and lib.y3_plan_op_flops(handle, i) == 0.0
    finally:
        lib.y3_plan_destroy(handle)


def test_a_stale_library_is_refused_for_this_cfg(monkeypatch):
    net = yolov3.Darknet(CFG, dtype="bf16")
    desc = build_plan(net.blocks, net.net_info, 1, 64, 64, 2)
    fake = kc._Fake(net._convs, 2)
    _, needs, _ = fill_ops(desc, net.net_info, net._convs, net.dtype, 1, "u8", "reference", None, fake)
    monkeypatch.setattr(_hip, "capabilities", lambda: 0xFFFFFFFF & ~_hip.CAP_ATTENTION)
    with pytest.raises(_hip.HipLibraryError, match="attention blocks"):
        _hip.require_capabilities(needs, CFG)


# ---------------------------------------------------------------------------------------------- the library's device code

def test_attention_library_code_objects():
    """18 instances in workgroups of 256; the avgpool tree's static LDS (32 x 8 x VEC floats), none in the products; no scratch,
    no spills, register and LDS budgets and wave64 are tests/test_code_object.py's, for every library, as is that the main
    library holds none of these kernels"""
    kernels = census.kernels("attn")          # (asserts: built, device code for gfx950 only)
    names = sorted(k[".name"] for k in kernels)
    assert len(names) == 18 and sum("avgpool_kernel" in n for n in names) == 6 and sum("attn_mul_kernel" in n for n in names) == 12
    for k in kernels:
        name = k[".name"]
        assert k[".max_flat_workgroup_size"] == 256, name
        if "avgpool_kernel" in name:
            assert k[".group_segment_fixed_size"] in (32 * 8 * 4 * v for v in (1, 4, 8)), name
        else:
            assert k[".group_segment_fixed_size"] == 0, name


def test_attention_library_census():
    """one key per compiled instance, each recording the one symbol of its kind, form and type (tests/golden/kernel_instances_attn.json,
    recorded on an MI355X by tools/make_kernel_instances.py --library attn; that every compiled kernel is launched by a recorded
    case of tests/test_gpu_attention.py and no recorded symbol is missing from the library are tests/test_code_object.py's rules)"""
    fixture = census.load("attn")
    assert set(fixture) == {"footprint"} and sorted(fixture["footprint"]) == sorted(AU.CENSUS_KEYS)
    for key, syms in fixture["footprint"].items():
        kind, form, dtype = AU.census_case(key)[:3]
        assert len(syms) == 1 and AU.symbol_matches(syms[0], kind, form, dtype), (key, syms)
    assert len({v[0] for v in fixture["footprint"].values()}) == 18
