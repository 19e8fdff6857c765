"""The plans of a partitioned GPU, run: every kernel whose launch, tile shape or selection reads the CU count, at the counts a
DPX / QPX / CPX partition of an MI355X has (128, 64, 32) and at two stress values (20 and 1), on the ordinary 256-CU device
(tests/cu_count_util.py has the seam, the counts and the list of what runs; tests/test_cu_count_host.py proves without a GPU that
the list crosses every chooser rule that reads the count).  A grid of 32 workgroups computes the same values on 256 CUs as on 32: no
kernel here synchronises between workgroups.  What this cannot show is how a partition PERFORMS, or anything about its share of L2.

a. One-op rows, with the machinery of tests/test_gpu_footprint.py as it is (``_run``, the oracle gate, ``_no_nan``, the byte
   footprint of the dense and of the strided, poisoned run).  At 256 CUs the persistent kernels get one tile per workgroup on every
   row of the footprint table; the ``*_strided_tiles`` rows are sized so that on 20 CUs the workgroups own two different numbers of
   tiles, both at least 2 -- asserted from the grid the plan recorded -- and on 1 CU one workgroup owns them all: the code that
   carries state from tile to tile runs under the oracle, the poison and the footprint for the first time.  Where the kernel is the
   one the row gets on the whole chip, the output is that run's byte for byte (another grid, the same sums); where the chooser moved
   the row, the oracle gate decides and the pair is printed.
b. Whole networks block by block, ``_teacher_forced`` of tests/test_gpu_bf16.py and the walker of tests/test_gpu_yolov4.py as they
   are, tolerances included.
c. A plan keeps the count it was created with: created under one count and run under another, both ways.
d. Arena on, ``forward_frames`` as users run it, against the keep-all run of the same count.

Need an MI355X: -m gpu.  No test here changes or asks for the device's partition mode."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cu_count_util as cu
import footprint_util as fu
import kernel_census as census
import test_gpu_footprint as TF
from yolov3 import _hip

pytestmark = pytest.mark.gpu


def _device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------------------------------------ a. one-op rows

_OWN = {}        # (row, dtype) -> (outputs, kernel names) of the dense run at the device's own count, oracle-gated: made once, left unchanged
_COVERED = []


def _row(n):
    cid, opt, over = cu.ONE_OP_ROWS[n]
    return cu.one_op_case(cid, over), opt, cu.one_op_name(cid, opt, over)


def _own(n, dtype):
    if (n, dtype) not in _OWN:
        case, opt, name = _row(n)
        dense, msg, names, ref, lay = TF._run(case, dtype, "dense", opt_name=opt)
        assert msg is None, "%s at the device's own count: %s" % (name, msg)
        TF._no_nan(dense, lay)
        TF._check_dense_against_oracle(case, dtype, dense, ref, lay)
        _OWN[n, dtype] = (dense, names)
    return _OWN[n, dtype]


def _covered():
    if not _COVERED:
        _COVERED.append(census.union(census.load()["footprint"]))
    return _COVERED[0]


def _assert_in_census(what):
    """every symbol launched since the last clear is one that a footprint case at the device's own count launches too: no other
    count reaches a compiled instance that the one-op suite leaves out"""
    assert census.LAUNCHED, what
    got = set().union(*census.LAUNCHED)
    names = census.demangle(got)
    unreachable = set(census.LIBRARIES["main"].unreachable)
    assert not got & unreachable, "%s launched what kernel_census.UNREACHABLE excludes: %s" % (what, [names[s] for s in got & unreachable])
    assert got <= _covered(), "%s launched instances no footprint case covers:\n  %s" % (
        what, "\n  ".join(names[s] for s in sorted(got - _covered())))
    del census.LAUNCHED[:]


@pytest.mark.parametrize("count", cu.GPU_COUNTS)
@pytest.mark.parametrize("n,dtype", cu.one_op_ids(), ids=["%s-%s" % (cu.one_op_name(*cu.ONE_OP_ROWS[n]), d) for n, d in cu.one_op_ids()])
def test_one_op_row_under_another_cu_count(n, dtype, count):
    _hip.require_gpu()
    assert count <= _device_cus()
    case, opt, name = _row(n)
    own, own_names = _own(n, dtype)
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
    with _hip.device_cus(count):
        # the launch the plan records under this count, from a plan that only decides (fake addresses, every fragment-order copy given)
        step = cu.case_steps(case, dtype, opt, mode="dense")[0]
        dense, msg, names, ref, lay = TF._run(case, dtype, "dense", opt_name=opt)
        assert msg is None, "dense run: " + msg
        assert names[0] == step["kernel"], (names, step["kernel"])
        TF._no_nan(dense, lay)
        u8 = any(o.fmt == "u8" and o.side == "in" for o in lay.operands)
        for guard in ((0x00, 0xFF) if u8 else (0,)):
            strided, msg, snames, _, slay = TF._run(case, dtype, "strided", u8_guard=guard, opt_name=opt)
            assert snames == names, (snames, names)
            assert msg is None, "strided run (uint8 guards 0x%02X): %s" % (guard, msg)
            TF._no_nan(strided, slay)
            assert strided.keys() == dense.keys()
            for key in dense:
                assert torch.equal(strided[key], dense[key]), "%s: %d bytes of the strided, poisoned run differ from the dense run" % (
                    key, int((strided[key] != dense[key]).sum()))
    grid = step["dims"][0]
    if cu.ONE_OP_ROWS[n][0] in cu.PERSISTENT_ROWS:
        tiles = fu.persistent_grid(case, step["op"], case["B"], 1 << 30)
        assert names[0] == fu.family_name(case, dtype), names
        if count == 20:
            why = cu.uneven(case, step["op"], grid, tiles)
            assert why is None, why
        if count == 1:
            assert grid == (step["op"].out_c // int(case["family"].rsplit("x", 1)[1]) if name.startswith("wres") else 1), grid
    if names == own_names:
        # the same kernel on the same data with another grid (or tile shape): no legitimate difference
        for key in own:
            assert torch.equal(dense[key], own[key]), "%s at %d CUs (%s, grid %d): %d bytes of %s differ from the run at the device's own count" % (
                name, count, names[0], grid, int((dense[key] != own[key]).sum()), key)
    else:
        print("%s %s: %s at the device's own count, %s (grid %d) at %d CUs" % (name, dtype, ", ".join(own_names), ", ".join(names), grid, count))
        TF._check_dense_against_oracle(case, dtype, dense, ref, lay)
    _assert_in_census("%s %s at %d CUs" % (name, dtype, count))


# ------------------------------------------------------------------------------------------------ c. decided at creation
# The launchers of the persistent kernels ask their geometry function again at launch (csrc/conv_1x1.hip launch_conv1x1_wres,
# csrc/conv_halo.hip launch_conv_patch, csrc/conv_fused.hip launch_stem_s2 / launch_resblock), which reads the count again: they may
# take only what does not depend on it, and launch the grid the step recorded.

@pytest.mark.parametrize("created,run", [(20, 0), (0, 20), (1, 128), (32, 1)], ids=["20-own", "own-20", "1-128", "32-1"])
@pytest.mark.parametrize("cid", cu.PERSISTENT_ROWS)
def test_one_op_plan_keeps_the_count_it_was_created_with(cid, created, run):
    _hip.require_gpu()
    lib = _hip.lib()
    n = next(k for k, r in enumerate(cu.ONE_OP_ROWS) if r == (cid, None, {}))
    case, opt, name = _row(n)
    dtype = case["dtypes"][-1]
    own, own_names = _own(n, dtype)
    seen = []

    def logged_under_the_other_count(call):
        # (_run has created the plan by now, under ``created``; only the run sees ``run``)
        _hip.check(lib.y3_set_tuning(b"device_cus", run))
        seen.append(run)
        try:
            return census.logged(call)
        finally:
            _hip.check(lib.y3_set_tuning(b"device_cus", created))

    del census.LAUNCHED[:]
    with _hip.device_cus(created):
        dense, msg, names, _, lay = TF._run(case, dtype, "strided", logged=logged_under_the_other_count)
    assert seen == [run] and names == own_names
    assert msg is None, msg
    TF._no_nan(dense, lay)
    for key in own:
        assert torch.equal(dense[key], own[key]), "%s created under %d, run under %d: %d bytes of %s differ" % (
            name, created, run, int((dense[key] != own[key]).sum()), key)


def _net(dtype, options=None, **kw):
    import test_gpu_bf16 as G
    return G._net("yolov3", dtype, options=options, **kw)


def _small_frames(seed=7):
    from yolov3.synthdata import synth_frames
    _, h, w, batch, _ = cu.NETS[0]
    return synth_frames(seed, batch, h, w)


def _outputs(net, frames):
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    return {k: out[k].cpu() for k in ("bbox_xywh", "class_prob", "class_idx")}


@pytest.mark.parametrize("oname", ["default", "wres_always"])
def test_network_plan_keeps_the_count_it_was_created_with(oname):
    """compiled under 32 CUs and run after the context has ended; compiled at the device's own count and run under 32"""
    _hip.require_gpu()
    frames = _small_frames()
    a, b = _net("bf16", cu.NET_OPTIONS[oname]), _net("bf16", cu.NET_OPTIONS[oname])
    with _hip.device_cus(32):
        inside = _outputs(a, frames)
        kernels32 = [r["kernel"] for r in a.plan_report()]
    for frag in cu.NET_EXPECT[oname]:
        assert any(frag in k for k in kernels32), (frag, sorted(set(kernels32)))
    outside = _outputs(a, frames)
    assert [r["kernel"] for r in a.plan_report()] == kernels32 and len(a._plans) == 1
    own = _outputs(b, frames)
    kernels_own = [r["kernel"] for r in b.plan_report()]
    assert kernels_own != kernels32
    with _hip.device_cus(32):
        own_inside = _outputs(b, frames)
    assert [r["kernel"] for r in b.plan_report()] == kernels_own and len(b._plans) == 1
    for k in inside:
        assert torch.equal(outside[k], inside[k]), "%s: the plan made under 32 CUs gave other values once the override had ended" % k
        assert torch.equal(own_inside[k], own[k]), "%s: the plan made at the device's own count gave other values under the override" % k


# ------------------------------------------------------------------------------------------------ b. whole networks

_NET_CASES = [(m, h, w, b, o, d) for m, h, w, b, o in cu.NETS for d in cu.net_dtypes(o)]


@pytest.mark.parametrize("count", cu.NET_COUNTS)
@pytest.mark.parametrize("model,h,w,batch,oname,mode", _NET_CASES, ids=["%s-%s-%s" % (c[0], c[4], c[5]) for c in _NET_CASES])
def test_every_block_teacher_forced_under_another_cu_count(model, h, w, batch, oname, mode, count):
    import test_gpu_bf16 as G
    from yolov3.synthdata import synth_frames
    _hip.require_gpu()
    frames = synth_frames(1000 + h + w + batch, batch, h, w)
    expect = cu.NET_EXPECT[oname] if (model == "yolov3" and count == 32 and mode != "float32") else ()
    with _hip.device_cus(count):
        checked, frac, names = G._teacher_forced(model, frames, expect, options=cu.NET_OPTIONS[oname] or None, mode=mode)
    print("%s %s %dx%d b%d %s at %d CUs: %d blocks checked, worst mismatch share %.4f; %s" % (
        mode, model, h, w, batch, oname, count, checked, frac, sorted(set(names))))
    assert checked >= (20 if model == "yolov3-tiny" else 75)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_yolov4_tiny_every_block_under_32_cus(mode):
    import test_gpu_yolov4 as G4
    _hip.require_gpu()
    with _hip.device_cus(32):
        checked, kernel_of = G4._teacher_forced("yolov4-tiny", mode, 2, (0, 1))
    print(mode, "yolov4-tiny at 32 CUs: blocks checked", checked, sorted({k[0] for k in kernel_of.values()}))
    assert checked >= 30


# ------------------------------------------------------------------------------------------------ d. as users run it

@pytest.mark.parametrize("count", [32, 128])
def test_arena_run_equals_the_keep_all_run_of_the_same_count(count):
    """tests/test_gpu_plan_graph.py test_arena_reuse_same_kernels_same_outputs_twice, under the count"""
    _hip.require_gpu()
    frames = _small_frames(11)
    with _hip.device_cus(count):
        keep = _net("bf16", keep_all=True, fuse=True)
        want = _outputs(keep, frames)
        names = [(r["block"], r["kernel"]) for r in keep.plan_report()]
        net = _net("bf16")
        first = _outputs(net, frames)
        assert [(r["block"], r["kernel"]) for r in net.plan_report()] == names
        plan = net._last_plan
        second = _outputs(net, frames)
        assert net._last_plan is plan and len(net._plans) == 1
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(first[k], want[k]), "%d CUs: %s differs from the keep-all run" % (count, k)
        assert torch.equal(second[k], first[k]), "%d CUs: %s differs on the second forward" % (count, k)
    assert bool(torch.isfinite(first["class_prob"]).all())
