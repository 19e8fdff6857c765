"""The grouped and depthwise conv kernels on operands whose byte offsets pass 2^32 (-m gpu): tests/test_gpu_big_operands.py step
for step, on the rows of tests/grouped_suites.py (one per compiled instance, float32 and bf16; the host half, with the refusals at
the pixel and the launch limit, is in tests/test_grouped_host.py).

One device allocation per case, ``[pad of 4 GiB][input][output][residual] ...``, every operand ``[guard | body | guard]`` and every
activation operand a channel slice of a wider stride of its own: an address that wraps at 2^32 or a sign-extended 32-bit offset
lands in the pad or in a neighbouring operand -- recorded, never a fault.  Frame b of the input and of the shortcut operand is
base frame b % 3, NaN round them; the output slice is prefilled with NaN, the byte pattern round it.  After the run:

  (a) frames 0-2 and the last three hold, bit for bit, what the SAME instance gives on the three base frames alone, run dense
      between zero guards -- and that small run is, bit for bit, the ordered float32 restatement (tests/grouped_ordered.py);
  (b) every frame b of the output equals its frame b % 3 bit for bit, and no element is NaN;
  (c) the pad, every guard, every margin and every read-only operand is byte for byte what it was.

No tolerance.  A case takes 20 to 30 GiB for its allocation and as much again for the copy (c) compares with; it is skipped only
where the device has less free."""
import ctypes

import pytest
import torch

import footprint_util as fu
import grouped_cases as GC
import grouped_ordered as GO
import grouped_suites as GS

pytestmark = pytest.mark.gpu

SLACK = 3 << 30                                              # temporaries of the fills and checks, the small run


def _nhwc(t, tdt):
    return t.permute(0, 2, 3, 1).contiguous().to(tdt)


def _feed(case, dtype, data, lay, path, frames=None):
    """{operand name: [tensor per slice]} for fu.fill; ``frames``: a device index tensor, frame b of the result is base frame
    ``frames[b]`` of the three-frame data"""
    tdt = GC.TORCH_DT[dtype]
    host, cp, _ = GC.device_weights(case, path, data["p"]["weight"])
    sc, bi = torch.zeros(cp), torch.zeros(cp)
    sc[:case["cout"]], bi[:case["cout"]] = torch.from_numpy(data["scale"]), torch.from_numpy(data["bias"])
    feed = {"weight": [torch.from_numpy(host).to(tdt).reshape(1, -1)], "scale": [sc.reshape(1, -1)], "bias": [bi.reshape(1, -1)],
            "zero page": [torch.zeros(lay["zero page"].slices[0][1], dtype=tdt)]}
    for name, t, c in (("input", data["x"], case["cin"]), ("residual", data["res"], case["cout"])):
        base = _nhwc(t, tdt)
        if frames is not None:
            base = base.to(frames.device).reshape(3, -1)[frames]
        feed[name] = [base.reshape(-1, c)]
    return feed


def _run(ops, lay, alloc, base):
    from yolov3 import _hip as H
    lib = H.lib()
    handle = ctypes.c_void_p()
    H.check(lib.y3_plan_create_ex(ops, 1, lay["zero page"].ptr(base), None, ctypes.byref(handle)))
    try:
        name = lib.y3_plan_op_kernel(handle, 0).decode()
        before = alloc.clone()
        H.check(lib.y3_plan_run(handle, None, None))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    return name, before


def _alloc(total, dev):
    raw = torch.empty(total + fu.ALIGN, dtype=torch.uint8, device=dev)
    shift = -raw.data_ptr() % fu.ALIGN
    return raw, raw[shift:shift + total]


@pytest.mark.parametrize("dtype", GS.BIG_DTYPES)
@pytest.mark.parametrize("instance", sorted(GS.BIG_ROWS))
def test_grouped_kernel_addresses_operands_past_4_gib(instance, dtype):
    from yolov3 import _hip as H
    H.require_gpu()
    dev = torch.device("cuda:0")
    case = GS.BIG_ROWS[instance]
    want = GS.kernel_name(instance, dtype)
    path = GC.PATH_DWISE if GC.is_dwise(case) else GC.PATH_GROUPED
    tdt = GC.TORCH_DT[dtype]
    B = GS.big_batch(case, dtype)
    _, lay0 = GS.build(case, dtype, B, "strided", lead=[fu.pad_operand()])
    need = 2 * lay0.total + SLACK
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("%s %s needs %.1f GiB of device memory, %.1f GiB are free" % (instance, dtype, need / 2.0 ** 30, free / 2.0 ** 30))
    data = GC.make(case, dtype)
    assert data["x"].shape[0] == 3

    # ---- the three base frames alone, dense between zero guards: the ordered restatement's bits, and what (a) compares with
    _, lay3 = GS.build(case, dtype, 3, "dense")
    raw3, alloc3 = _alloc(lay3.total, dev)
    ops3, lay3 = GS.build(case, dtype, 3, "dense", alloc3.data_ptr())
    fu.fill(alloc3, lay3, _feed(case, dtype, data, lay3, path), poisoned=False)
    torch.cuda.synchronize()
    name, before3 = _run(ops3, lay3, alloc3, alloc3.data_ptr())
    assert name == want, (name, want)
    msg = fu.footprint_violations(before3, alloc3, lay3)
    assert msg is None, "small dense run: " + msg
    dense = fu.read_slice(alloc3, lay3["output"], 0, torch.uint8)
    ho, wo = GC.out_hw(case)
    got3 = dense.view(tdt).reshape(3, ho, wo, case["cout"]).float().permute(0, 3, 1, 2).contiguous().cpu()
    assert torch.equal(got3, torch.from_numpy(GO.of_case(case, dtype, data))), "%s: the dense three-frame run is not the ordered restatement" % want
    del before3, alloc3, raw3

    # ---- the big run
    raw, alloc = _alloc(lay0.total, dev)
    base = alloc.data_ptr()
    ops, lay = GS.build(case, dtype, B, "strided", base, lead=[fu.pad_operand()])
    assert lay.total == lay0.total and lay.operands[0].name == "pad" and lay.operands[0].body_bytes >= (1 << 32)
    assert all(o.body_bytes > fu.SPAN + o.body_bytes // B for o in GS.span_operands(lay))
    idx = torch.arange(B, device=dev) % 3
    fu.fill(alloc, lay, _feed(case, dtype, data, lay, path, idx), poisoned=True, u8_guard=0xFF)
    torch.cuda.synchronize()
    name, before = _run(ops, lay, alloc, base)
    assert name == want, (name, want)
    try:
        # (c) nothing but the output slice changed
        msg = fu.region_violations(before, alloc, lay)
        assert msg is None, msg
        del before
        o = lay["output"]
        t = fu.read_slice(alloc, o, 0, torch.uint8)
        f = t.reshape(B, -1)
        three = dense.reshape(3, -1)
        assert three.shape[1] == f.shape[1], (tuple(three.shape), tuple(f.shape))
        # (a) the first and the last three frames against the small run of the same instance
        for b in (0, 1, 2, B - 3, B - 2, B - 1):
            differ = int((f[b] != three[b % 3]).sum())
            assert differ == 0, "frame %d of %d differs from the three-frame run's frame %d in %d of %d bytes" % (b, B, b % 3, differ, f.shape[1])
        # (b) no NaN, and every frame is frame b % 3
        msg = fu.nan_violations(t, B, o.fmt) or fu.frame_violations(t, B)
        assert msg is None, msg
        del t, f, three
    finally:
        before = alloc = raw = None
        torch.cuda.empty_cache()
