"""The memory-bound layer kernels on every storage pattern (-m gpu): max-pool in every form, upsample, add and copy, one op per
plan through the C ABI, on the maps of tests/layer_patterns.py -- every bf16 / fp16 pattern, planted and random float32 ones,
zeros of both signs, NaN taps -- against the references stated there.  Outputs are compared as integers, never as floats: -0
is not +0 here, and a subnormal is not zero.  The one allowance is the rule's own: where it says "some NaN" (add results, and
16-bit NaN through upsample and copy) every NaN counts as the same pattern.

Every output goes into a channel slice of a wider buffer filled with a sentinel byte; the rest of the buffer must be unchanged.
Each case asserts the kernel that ran.  The pyramid runs a second time as three single pools (fuse_spp = 0) on the same data,
and the two must agree with each other bit for bit as well as with the reference."""
import numpy as np
import pytest
import torch

from yolov3 import _hip

import layer_patterns as L
from test_gpu_darknet_pool import FUSED, _pool_op, _run

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
_INT = {16: torch.int16, 32: torch.int32}


def _dev(p, dtype):
    """patterns (B, H, W, ld) -> a device tensor of the storage type holding them"""
    return L.to_torch(p, dtype).cuda()


def _ints(t):
    """a device tensor of a storage type -> the integer view of it that comparisons are made on"""
    return t.contiguous().view(_INT[t.element_size() * 8])


def _want(p, dtype, nan_ok=False):
    p = L.canon_nan(p, dtype) if nan_ok else np.ascontiguousarray(p)
    return torch.from_numpy(p.view(L.itype(dtype)).copy()).cuda()


def _got(view, dtype, nan_ok=False):
    g = _ints(view)
    if not nan_ok:
        return g
    mag = g.to(torch.int64) & (L.sign_bit(dtype) - 1)
    quiet = L.inf_bits(dtype) | (1 << (L.man_bits(dtype) - 1))
    return torch.where(mag > L.inf_bits(dtype), torch.full_like(g, quiet), g)


def _slice_geometry(dtype, c, slices=1):
    """(channel offset of the first slice, pixel stride) of the output buffer: multiples of the 16-byte vector for a channel
    count that runs the wide form, odd ones otherwise"""
    vec = 16 // (L.bits(dtype) // 8)
    if c % vec == 0:
        return vec, slices * c + 3 * vec
    return 3, slices * c + 8


class _Out(object):
    """a sentinel-filled (B, Ho, Wo, ld) buffer with ``slices`` output slices of c channels from channel ``off`` on"""

    def __init__(self, dtype, b, oh, ow, c, slices=1):
        td = L.torch_dtype(dtype)
        self.c, self.slices = c, slices
        self.off, self.ld = _slice_geometry(dtype, c, slices)
        self.buf = torch.full((b * oh * ow * self.ld * td.itemsize,), SENTINEL, dtype=torch.uint8, device="cuda").view(td).view(b, oh, ow, self.ld)

    def view(self, n=0):
        return self.buf[0, 0, 0, self.off + n * self.c:]

    def slice(self, n=0):
        return self.buf[..., self.off + n * self.c:self.off + (n + 1) * self.c]

    def rest_untouched(self):
        rest = torch.cat([self.buf[..., :self.off], self.buf[..., self.off + self.slices * self.c:]], dim=-1)
        return bool((rest.contiguous().view(torch.uint8) == SENTINEL).all())


def _layer_op(kind, dtype, x_dev, c, out, oh, ow, k=1, s=1, darknet=False, n=0, block=0):
    op = _pool_op(dtype, x_dev, c, k, s, k - 1, out.view(n), out.ld, (oh, ow), darknet=darknet, block=block)
    op.kind = kind
    return op


def _report(what, got, want):
    """the first few disagreeing elements, as patterns: what a failure prints"""
    bad = (got != want).nonzero()
    lines = ["%s: %d of %d elements differ" % (what, bad.shape[0], got.numel())]
    for idx in bad[:6].tolist():
        mask = (1 << (got.element_size() * 8)) - 1
        lines.append("  at %s got 0x%X want 0x%X" % (tuple(idx), int(got[tuple(idx)]) & mask, int(want[tuple(idx)]) & mask))
    return "\n".join(lines)


def _check(failures, what, got, want):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not torch.equal(got, want):
        failures.append(_report(what, got, want))


def _finish(failures):
    if failures:
        print("\n".join(failures))
    assert not failures, "%d cases differ from the reference; the first: %s" % (len(failures), failures[0])


# ---- max pools -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("form", ["maxpool", "maxpool_dk"])
def test_single_pool_returns_the_maximum_bits(form, dtype):
    darknet = form == "maxpool_dk"
    failures = []
    for label, m in L.pool_inputs(form, dtype):
        b, h, w, c = m.shape
        x_dev = _dev(m, dtype)
        for k, s in L.pool_ks(form):
            oh, ow = L.pool_geometry(h, w, k, s, darknet)[:2]
            out = _Out(dtype, b, oh, ow, c)
            names = _run([_layer_op(_hip.OP_MAXPOOL, dtype, x_dev, c, out, oh, ow, k, s, darknet)])
            what = "%s %s %s k=%d s=%d" % (form, dtype, label, k, s)
            assert names == [form + "_" + L.tag(dtype)], what
            assert out.rest_untouched(), what
            _check(failures, what, _got(out.slice(), dtype), _want(L.pool_expected(form, dtype, label, k, s), dtype))
    _finish(failures)


@pytest.mark.parametrize("dtype", L.DTYPES)
@pytest.mark.parametrize("form", ["spp", "spp_dk"])
def test_pyramid_returns_the_maximum_bits_and_equals_three_pools(form, dtype):
    darknet = form == "spp_dk"
    single = ("maxpool_dk_" if darknet else "maxpool_") + L.tag(dtype)
    pyramid = ("maxpool_spp_pyramid_dk_" if darknet else "maxpool_spp_pyramid_") + L.tag(dtype)
    failures = []
    for label, m in L.pool_inputs(form, dtype):
        b, h, w, c = m.shape
        x_dev = _dev(m, dtype)
        got = {}
        for fuse, expect in ((1, [pyramid, FUSED, FUSED]), (0, [single] * 3)):
            out = _Out(dtype, b, h, w, c, slices=3)
            ops = [_layer_op(_hip.OP_MAXPOOL, dtype, x_dev, c, out, h, w, k, 1, darknet, n=n, block=10 + n)
                   for n, k in enumerate(L.SPP_KS)]
            names = _run(ops, fuse_spp=fuse)
            what = "%s %s %s fuse_spp=%d" % (form, dtype, label, fuse)
            assert names == expect, what
            assert out.rest_untouched(), what
            got[fuse] = [_got(out.slice(n), dtype).clone() for n in range(3)]
        for n, k in enumerate(L.SPP_KS):
            what = "%s %s %s k=%d" % (form, dtype, label, k)
            want = _want(L.pool_expected(form, dtype, label, k, 1), dtype)
            _check(failures, what + " pyramid", got[1][n], want)
            _check(failures, what + " three pools", got[0][n], want)
            _check(failures, what + " pyramid against three pools", got[1][n], got[0][n])
    _finish(failures)


# ---- upsample, copy, add ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", L.DTYPES)
def test_upsample_returns_every_pattern(dtype):
    """float32: every pattern identical, NaN payloads included; 16-bit: every non-NaN pattern identical, a NaN some NaN"""
    nan_ok = L.bits(dtype) == 16
    failures = []
    for label, shape in (("wide", L.WIDE_UP), ("elem", L.ELEM_UP)):
        m = L.input_map("all", dtype, shape)
        b, h, w, c = m.shape
        x_dev = _dev(m, dtype)
        for s in L.UPSAMPLE_STRIDES:
            out = _Out(dtype, b, h * s, w * s, c)
            names = _run([_layer_op(_hip.OP_UPSAMPLE, dtype, x_dev, c, out, h * s, w * s, 1, s)])
            what = "upsample %s %s stride %d" % (dtype, label, s)
            assert names == ["upsample_" + L.tag(dtype)], what
            assert out.rest_untouched(), what
            _check(failures, what, _got(out.slice(), dtype, nan_ok), _want(L.upsample_gather(m, s), dtype, nan_ok))
    _finish(failures)


@pytest.mark.parametrize("dtype", L.DTYPES)
def test_copy_returns_every_pattern(dtype):
    nan_ok = L.bits(dtype) == 16
    failures = []
    for label, shape in (("wide", L.WIDE), ("elem", L.ELEM)):
        m = L.input_map("all", dtype, shape)
        b, h, w, c = m.shape
        x_dev = _dev(m, dtype)
        out = _Out(dtype, b, h, w, c)
        names = _run([_layer_op(_hip.OP_COPY, dtype, x_dev, c, out, h, w)])
        what = "copy %s %s" % (dtype, label)
        assert names == ["copy_" + L.tag(dtype)], what
        assert out.rest_untouched(), what
        _check(failures, what, _got(out.slice(), dtype, nan_ok), _want(m, dtype, nan_ok))
    _finish(failures)


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("dtype", L.DTYPES)
def test_add_rounds_the_float_sum_once(dtype, inplace):
    """every ordered 16-bit pattern against each second operand of layer_patterns.SECOND (float32: the planted list against
    itself); in place the first operand is the output slice itself (d_out == d_in)"""
    failures = []
    for label, shape in (("wide", L.WIDE), ("elem", L.ELEM)):
        b, h, w, c = shape
        for name, a, second in L.add_cases(dtype, shape):
            out = _Out(dtype, b, h, w, c)
            res = _dev(second, dtype)
            if inplace:
                out.slice().copy_(_dev(a, dtype))
                op = _layer_op(_hip.OP_ADD, dtype, out.buf, c, out, h, w)
                op.d_in = out.view().data_ptr()
            else:
                a_dev = _dev(a, dtype)
                op = _layer_op(_hip.OP_ADD, dtype, a_dev, c, out, h, w)
            op.d_res, op.res_ld = res.data_ptr(), c
            names = _run([op])
            what = "add %s %s second operand %s%s" % (dtype, label, name, " in place" if inplace else "")
            assert names == ["add_" + L.tag(dtype)], what
            assert out.rest_untouched(), what
            _check(failures, what, _got(out.slice(), dtype, True), _want(L.add_torch(a, second, dtype), dtype, True))
            if not inplace:
                assert torch.equal(_ints(a_dev), _want(a, dtype)), what          # the operands are read only
            assert torch.equal(_ints(res), _want(second, dtype)), what
    _finish(failures)
