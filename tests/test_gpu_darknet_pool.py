"""Darknet max-pool semantics on the GPU (-m gpu): Y3_F_POOL_DARKNET ops through the C ABI against the CPU witness
(tests/darknet_pool_restate.py), bit for bit in float32, bf16 and fp16; the centred SPP pyramid against the witness, against
three single pools, and around its slices of the route buffer; ``Darknet(..., pool="darknet")`` for every shipped network
that pools, against the restatement with the witness's pool, at the gates the existing tests of the same model use."""
import ctypes
import os

import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

import darknet_pool_restate as DP
import test_gpu_yolov4 as T4
import yolov4_restate as R
from golden_util import MODEL_DIR, SAMPLE_IMAGES, load_jpeg_bgr
from test_gpu_parity import BOX_ATOL, SCORE_ATOL

pytestmark = pytest.mark.gpu

DTYPES = {"float32": (_hip.Y3_F32, torch.float32, "f32"), "bf16": (_hip.Y3_BF16, torch.bfloat16, "bf16"),
          "fp16": (_hip.Y3_F16, torch.float16, "f16")}
FUSED = "(fused into the previous op)"


def _signed(shape, seed, tdtype):
    """signed values exactly representable in the storage type, as float32 (B, C, H, W)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 3.0).to(tdtype).float()


def _negative(shape, seed, tdtype):
    """the same, every value below -1 (rounded to the storage type after the shift)"""
    return (-_signed(shape, seed, tdtype).abs() - 1.0).to(tdtype).float()


def _nhwc(x, tdtype, ld):
    b, c, h, w = x.shape
    t = torch.zeros((b, h, w, ld), dtype=tdtype)
    t[..., :c] = x.permute(0, 2, 3, 1).to(tdtype)
    return t.cuda()


def _pool_op(dtype, x_dev, c, k, s, p, out_view, out_ld, out_hw, darknet=True, block=0):
    op = _hip.Y3Op()
    op.kind, op.dtype, op.block_idx = _hip.OP_MAXPOOL, DTYPES[dtype][0], block
    op.batch, op.in_h, op.in_w, op.in_c, op.in_ld = x_dev.shape[0], x_dev.shape[1], x_dev.shape[2], c, x_dev.shape[3]
    op.out_h, op.out_w, op.out_c, op.out_ld = out_hw[0], out_hw[1], c, out_ld
    op.ksize, op.stride = k, s
    if darknet:
        op.flags |= _hip.F_POOL_DARKNET
        op.pad = p
    op.d_in, op.d_out = x_dev.data_ptr(), out_view.data_ptr()
    return op


def _run(ops, **options):
    """(kernel names) of a plan of ``ops`` after one run of it"""
    lib = _hip.lib()
    zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    arr = (_hip.Y3Op * len(ops))(*ops)
    handle = ctypes.c_void_p()
    opts = _hip.options(**options)
    _hip.check(lib.y3_plan_create_ex(arr, len(ops), zero.data_ptr(), ctypes.byref(opts), ctypes.byref(handle)))
    try:
        names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
        _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    return names


def _one_pool(dtype, x, k, s, p=None, darknet=True, ld_extra=0):
    """one max-pool op on x (B, C, H, W float32 holding storage-type values) -> (kernel name, (B, C, Ho, Wo) float32)"""
    p = k - 1 if p is None else p
    tdtype = DTYPES[dtype][1]
    b, c, h, w = x.shape
    if darknet:
        oh, ow = DP.out_size(h, k, s, p), DP.out_size(w, k, s, p)
    else:
        oh, ow = (h, w) if s == 1 else ((h - k) // s + 1, (w - k) // s + 1)
    x_dev = _nhwc(x, tdtype, c + ld_extra)
    out = torch.zeros((b, oh, ow, c + ld_extra), dtype=tdtype, device="cuda")
    names = _run([_pool_op(dtype, x_dev, c, k, s, p, out, c + ld_extra, (oh, ow), darknet)])
    return names[0], out[..., :c].permute(0, 3, 1, 2).float().cpu().contiguous()


MAPS = [(13, 13), (16, 16), (19, 19), (20, 20), (38, 38), (17, 22)]       # 13, 19 and 17: odd maps at stride 2 as well
CHANNELS = [16, 13]                                                        # 16-byte vectors in every dtype / scalar in every dtype


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k,s", [(2, 1), (2, 2), (3, 2), (5, 1), (9, 1), (13, 1)])
def test_single_pool_is_the_witness_bit_for_bit(k, s, dtype):
    tag = DTYPES[dtype][2]
    for hw in MAPS:
        for c in CHANNELS:
            x = _signed((2, c) + hw, 1000 * k + 100 * s + hw[0] + c, DTYPES[dtype][1])
            name, got = _one_pool(dtype, x, k, s)
            what = "%s k=%d s=%d map %s c=%d" % (dtype, k, s, hw, c)
            assert name == "maxpool_dk_" + tag, what
            want = DP.pool(x, k, s)
            assert got.shape == want.shape, what
            assert torch.equal(got, want), what


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_explicit_padding_and_wider_pixel_strides(dtype):
    for k, s, p in [(2, 2, 0), (3, 2, 1), (3, 1, 0), (5, 1, 2), (2, 1, 2)]:
        x = _signed((1, 24, 15, 18), 7 * k + s + p, DTYPES[dtype][1])
        name, got = _one_pool(dtype, x, k, s, p, ld_extra=8)
        assert name.startswith("maxpool_dk_") and torch.equal(got, DP.pool(x, k, s, p)), (dtype, k, s, p)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("k", [2, 5, 9, 13])
def test_all_negative_map_tells_the_modes_apart(k, dtype):
    """The reference's pool counts out-of-range taps as 0.0, Darknet's leaves them out: on an all-negative map the last row and
    column must differ.  A library that ignored the flag would fail here."""
    tag = DTYPES[dtype][2]
    x = _negative((2, 16, 19, 19), k, DTYPES[dtype][1])
    name_dk, dk = _one_pool(dtype, x, k, 1)
    name_ref, ref = _one_pool(dtype, x, k, 1, darknet=False)
    assert (name_dk, name_ref) == ("maxpool_dk_" + tag, "maxpool_" + tag)
    assert torch.equal(dk, DP.pool(x, k, 1)) and torch.equal(ref, orc.maxpool(x, k, 1))
    assert (ref[:, :, -1, :] == 0).all() and (ref[:, :, :, -1] == 0).all()
    assert (dk < 0).all()
    assert not torch.equal(dk[:, :, -1, :], ref[:, :, -1, :]) and not torch.equal(dk[:, :, :, -1], ref[:, :, :, -1])


def test_library_refuses_what_the_rule_does_not_define():
    x = _signed((1, 16, 13, 13), 1, torch.float32)
    x_dev = _nhwc(x, torch.float32, 16)
    out = torch.zeros((1, 14, 14, 16), device="cuda")
    wrong_size = _pool_op("float32", x_dev, 16, 2, 2, 1, out, 16, (6, 6), block=7)       # Darknet: (13 + 1 - 2) / 2 + 1 = 7
    with pytest.raises(RuntimeError, match="maxpool block 7"):
        _run([wrong_size])
    empty_window = _pool_op("float32", x_dev, 16, 2, 1, 6, out, 16, (18, 18), block=8)   # padding / 2 = 3 > size - 1
    with pytest.raises(RuntimeError, match="maxpool block 8"):
        _run([empty_window])
    up = _pool_op("float32", x_dev, 16, 1, 1, 0, out, 16, (13, 13), block=9)
    up.kind = _hip.OP_UPSAMPLE
    with pytest.raises(RuntimeError, match="block 9.*Y3_F_POOL_DARKNET"):
        _run([up])


# ---- SPP pyramid -----------------------------------------------------------------------------------------------------------

SENTINEL = 0x5A


def _spp(dtype, x, order, modes=(True, True, True), **options):
    """pools `order` of x into channel slices 0, 1, 2 of a route buffer of 4 slices + 8 channels -> (names, {k: (B,C,H,W)}, rest)"""
    tdtype = DTYPES[dtype][1]
    b, c, h, w = x.shape
    ld = 4 * c + 8
    x_dev = _nhwc(x, tdtype, c)
    buf = torch.full((b * h * w * ld * tdtype.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda").view(tdtype).view(b, h, w, ld)
    ops = [_pool_op(dtype, x_dev, c, k, 1, k - 1, buf[0, 0, 0, n * c:], ld, (h, w), darknet=modes[n], block=10 + n)
           for n, k in enumerate(order)]
    names = _run(ops, **options)
    outs = {k: buf[..., n * c:(n + 1) * c].permute(0, 3, 1, 2).float().cpu().contiguous() for n, k in enumerate(order)}
    rest = buf[..., 3 * c:].contiguous().view(torch.uint8).cpu()
    return names, outs, rest


@pytest.mark.parametrize("order", [(5, 9, 13), (13, 5, 9)])
@pytest.mark.parametrize("hw", [(19, 19), (16, 16), (13, 13), (20, 20), (16, 20)])
@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_spp_pyramid_centred(dtype, hw, order):
    tag = DTYPES[dtype][2]
    x = _signed((3, 32) + hw, hw[0] * hw[1] + order[0], DTYPES[dtype][1])
    names, one, rest = _spp(dtype, x, order)
    assert names == ["maxpool_spp_pyramid_dk_" + tag, FUSED, FUSED]
    names3, three, rest3 = _spp(dtype, x, order, fuse_spp=0)
    assert names3 == ["maxpool_dk_" + tag] * 3
    for k in order:
        want = DP.pool(x, k, 1)
        assert torch.equal(want, torch.nn.functional.max_pool2d(x, k, 1, k // 2))
        assert torch.equal(one[k], want), (dtype, hw, k, "pyramid")
        assert torch.equal(three[k], want), (dtype, hw, k, "three pools")
        # the same on the bits (the storage values widened to float32 keep theirs): -0.0 == +0.0 as floats
        assert torch.equal(one[k].view(torch.int32), want.view(torch.int32)), (dtype, hw, k, "pyramid, bits")
        assert torch.equal(one[k].view(torch.int32), three[k].view(torch.int32)), (dtype, hw, k, "pyramid against three pools, bits")
    assert (rest == SENTINEL).all() and (rest3 == SENTINEL).all()          # nothing outside the three slices is written


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_spp_on_an_all_negative_map_differs_from_the_reference_pyramid(dtype):
    tag = DTYPES[dtype][2]
    x = _negative((2, 32, 19, 19), 5, DTYPES[dtype][1])
    names_dk, dk, _ = _spp(dtype, x, (5, 9, 13))
    names_ref, ref, _ = _spp(dtype, x, (5, 9, 13), modes=(False, False, False))
    assert names_dk[0] == "maxpool_spp_pyramid_dk_" + tag and names_ref[0] == "maxpool_spp_pyramid_" + tag
    for k in (5, 9, 13):
        assert torch.equal(dk[k], DP.pool(x, k, 1)) and torch.equal(ref[k], orc.maxpool(x, k, 1))
        assert (dk[k] < 0).all() and (ref[k][:, :, -1, :] == 0).all()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_spp_of_mixed_modes_does_not_fuse(dtype):
    tag = DTYPES[dtype][2]
    x = _signed((2, 32, 19, 19), 9, DTYPES[dtype][1])
    names, outs, rest = _spp(dtype, x, (5, 9, 13), modes=(False, True, True))
    assert names == ["maxpool_" + tag, "maxpool_dk_" + tag, "maxpool_dk_" + tag]
    assert torch.equal(outs[5], orc.maxpool(x, 5, 1))
    assert torch.equal(outs[9], DP.pool(x, 9, 1)) and torch.equal(outs[13], DP.pool(x, 13, 1))
    assert (rest == SENTINEL).all()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_spp_too_large_for_lds_falls_back(dtype):
    tag = DTYPES[dtype][2]
    x = _signed((1, 32, 38, 38), 38, DTYPES[dtype][1])           # (38 + 12)^2 positions x 64 bytes > 64 KiB
    names, outs, rest = _spp(dtype, x, (5, 9, 13))
    assert names == ["maxpool_dk_" + tag] * 3
    for k in (5, 9, 13):
        assert torch.equal(outs[k], DP.pool(x, k, 1))
    assert (rest == SENTINEL).all()


# ---- whole networks --------------------------------------------------------------------------------------------------------

DIMS = {"yolov3-spp": 608, "yolov3-tiny": 416, "yolov4": 608, "yolov4-tiny": 416, "yolov4-csp": 512}
OBJ_BIAS = -5.0
_PARAMS = {}


def _cfg(model):
    return os.path.join(MODEL_DIR, model + ".cfg")


def _params(model):
    if model not in _PARAMS:
        blocks, net_info = parse_config(_cfg(model))
        _PARAMS[model] = W.synth_params(blocks, net_info, seed=0, obj_bias=OBJ_BIAS, calib=W.load_calibration(model))
    return _PARAMS[model]


def _net(model, dtype, **kw):
    return yolov3.Darknet(_cfg(model), device="cuda", dtype=dtype, **kw).set_params(_params(model)).eval()


def _kernels(net):
    return [r["kernel"] for r in net.plan_report()]


def _bits(out):
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("model", ["yolov3-spp", "yolov3-tiny", "yolov4"])
def test_default_is_the_reference_pool(model):
    """no ``pool=`` and ``pool="reference"``: the same bits, and no Darknet-rule kernel in the plan"""
    frames = synth_frames(31, 2, DIMS[model], DIMS[model])
    plain = _net(model, "bf16")
    a = _bits(plain.forward_frames(frames))
    named = _net(model, "bf16", pool="reference")
    b = named.forward_frames(frames)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    for net in (plain, named):
        assert not any("_dk" in k for k in _kernels(net))
        assert any(k.startswith("maxpool_") for k in _kernels(net))


@pytest.mark.parametrize("model", ["yolov3-spp", "yolov3-tiny", "yolov4", "yolov4-tiny", "yolov4-csp"])
def test_float32_network_matches_restatement_with_darknet_pools(model):
    _float32_network_matches_restatement(model, DIMS[model])


@pytest.mark.parametrize("model", ["yolov3-spp", "yolov3-tiny"])
def test_float32_network_matches_restatement_with_darknet_pools_at_32_pixels(model):
    """1 x 1, 2 x 2 and 4 x 4 maps: the centred 13-window has one tap inside a 1 x 1 map (yolov3-spp), and yolov3-tiny's last
    stride-2 pool goes from 2 x 2 to 1 x 1 and its size-2 stride-1 pool runs on that one pixel"""
    _float32_network_matches_restatement(model, 32)


def _float32_network_matches_restatement(model, dim):
    net = _net(model, "float32", pool="darknet")
    cls = DP.NewCoordsRestatement if model == "yolov4-csp" else DP.Restatement
    ref = cls(_cfg(model), _params(model))
    frames = synth_frames(13, 2, dim, dim)
    x = R.frames_to_input(frames)
    got = net.forward(x)
    names = _kernels(net)
    pools = [k for k in names if k.startswith("maxpool_")]
    assert pools and all("_dk_" in k for k in pools), pools
    if model in ("yolov3-spp", "yolov4", "yolov4-csp"):
        assert pools == ["maxpool_spp_pyramid_dk_f32"]
    want = ref.forward(x)
    assert got["bbox_xywh"].shape == want["bbox_xywh"].shape
    np.testing.assert_allclose(got["bbox_xywh"].cpu().numpy(), want["bbox_xywh"].numpy(), rtol=1e-4, atol=BOX_ATOL)
    np.testing.assert_allclose(got["class_prob"].cpu().numpy(), want["class_prob"].numpy(), atol=SCORE_ATOL)
    dflt = _net(model, "float32").forward(x)
    if model == "yolov4-tiny":
        # its pools are all size 2 / stride 2 on even maps at the cfg's size: the two rules coincide
        for k in got:
            assert torch.equal(got[k], dflt[k]), k
    else:
        assert not torch.equal(got["class_prob"], dflt["class_prob"])
        assert not torch.equal(got["bbox_xywh"], dflt["bbox_xywh"])


class _OracleWithDarknetPools(object):
    """oracle.darknet_oracle with the witness's pool in place of its own, for the teacher-forced gate of test_gpu_yolov4.py"""

    def __getattr__(self, name):
        return getattr(orc, name)

    @staticmethod
    def maxpool(x, k, s):
        return DP.pool(x, k, s)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("model", ["yolov4", "yolov3-spp"])
def test_16bit_every_block_teacher_forced_batch16_darknet_pools(monkeypatch, model, mode):
    """test_gpu_yolov4.py's gate (every block fed with the product's own input, one storage ulp; pools, routes and upsamples
    bit for bit) on a ``pool="darknet"`` network, its pool blocks compared with the witness."""
    monkeypatch.setitem(T4.DIMS, "yolov3-spp", 608)
    monkeypatch.setattr(T4, "_net", lambda m, dtype, **kw: _net(m, dtype, pool="darknet", **kw))
    monkeypatch.setattr(T4, "orc", _OracleWithDarknetPools())
    checked, kernel_of = T4._teacher_forced(model, mode, 16, (0, 15))
    names = sorted({k[0] for k in kernel_of.values()})
    print(mode, model, "blocks checked", checked, names)
    assert checked >= (130 if model == "yolov4" else 75)
    assert any(k.startswith("maxpool_spp_pyramid_dk_") for k in names)
    assert not any(k.startswith("maxpool_") and "_dk_" not in k for k in names)


def test_csp_letterboxed_inference_is_batching_independent():
    """``inference`` one frame at a time and ``detect_in_frames`` at batch 16 return the same detections on a
    ``pool="darknet"`` yolov4-csp network with letterboxing: the combination yolov4-csp was trained with."""
    net = _net("yolov4-csp", "bf16", pool="darknet")
    images = [load_jpeg_bgr(n) for n in SAMPLE_IMAGES[:3]] * 6             # 18 frames: a full batch and a partial one
    streamed = list(yolov3.detect_in_frames(net, images, batch_size=16, letterbox=True))
    assert len(streamed) == len(images)
    assert any("_dk_" in k for k in _kernels(net))
    batch = yolov3.inference(net, images[:16], device="cuda", letterbox=True)
    kept = 0
    for f in (0, 1, 2, 15, 17):
        one = yolov3.inference(net, images[f], device="cuda", letterbox=True)[0]
        kept += len(one[1])
        for a, b in zip(streamed[f], one):
            assert np.array_equal(np.asarray(a), np.asarray(b)), "frame %d" % f
        if f < 16:
            for a, b in zip(batch[f], one):
                assert np.array_equal(np.asarray(a), np.asarray(b)), "frame %d of a batch of 16" % f
    assert kept > 0
