"""Network plans that hold the direct-weights fused block kernel (csrc/conv_block_dw.hip; y3_options.fuse_block = 3 / 4): arena
reuse, a real route slice as the output of a pair, the rule that z must not overlap x -- and the configuration the benchmark
times, which ``Pipeline`` selects by default for more than one batch in flight.

  small network   yolov3 at 160 x 224 x 3 frames (tests/block_dw_cases.py NET), bf16 and fp16, fuse_block = 4: every block
                  teacher-forced at the gates of tests/test_gpu_cu_count.py test_every_block_teacher_forced_under_another_cu_count
                  (tests/test_gpu_bf16.py ``_teacher_forced``); outputs bit-equal to fuse_block = 0; the arena run bit-equal to
                  the keep-all run; no fused pair writes over its own input.
  shipped shape   yolov3 608 bf16 at batch 16 under the options a Pipeline builds, three runs: bit-identical to fuse_block = 0.
  the default     a Pipeline with two batches in flight and no options.
Need an MI355X: -m gpu."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import block_dw_cases as BDC  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("bbox_xywh", "class_prob", "class_idx")
TAG = {"bf16": "bf16", "fp16": "f16"}


def _outputs(net, frames):
    out = net.forward_frames(frames)
    torch.cuda.synchronize()
    return {k: out[k].cpu() for k in KEYS}


def _dw_blocks(net, dtype):
    return [r["block"] for r in net.plan_report() if r["kernel"] == "conv_block_dw_%s_x128" % TAG[dtype]]


def _assert_no_pair_in_place(cp, blocks):
    """the address check of tests/test_gpu_block_fused.py test_whole_network_with_the_fused_block_equals_the_two_launches"""
    seen = 0
    for n in range(cp.n_ops - 1):
        if int(cp.ops[n].block_idx) in blocks:
            a, b = cp.ops[n], cp.ops[n + 1]
            x0, xb = a.d_in, a.batch * a.in_h * a.in_w * a.in_ld * 2
            z0, zb = b.d_out, b.batch * b.out_h * b.out_w * b.out_ld * 2
            assert not (x0 < z0 + zb and z0 < x0 + xb), "fused pair at block %d runs in place" % a.block_idx
            seen += 1
    assert seen == len(blocks)


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_small_network_with_the_kernel_teacher_forced_and_equal_to_the_two_launches(mode):
    import test_gpu_bf16 as G
    from yolov3 import _hip
    from yolov3.synthdata import synth_frames
    _hip.require_gpu()
    model, h, w, batch = BDC.NET
    frames = synth_frames(2000 + h + w + batch, batch, h, w)
    name = "conv_block_dw_%s_x128" % TAG[mode]
    checked, frac, names = G._teacher_forced(model, frames, (name,), options={"fuse_block": 4}, mode=mode)
    print("%s %s %dx%d b%d fuse_block 4: %d blocks checked, worst mismatch share %.4f" % (mode, model, h, w, batch, checked, frac))
    # that test's bound, 75 blocks, counts both convs of these pairs; a fused pair is one check, of its second conv against the
    # oracle's two convs from the pair's input (81 checks at most in yolov3, less one per fused pair: 68 here)
    assert checked >= 75 - len(BDC.NET_BLOCKS)
    # (the keep-all plan of the teacher-forced walk never hands z the bytes of x: it fuses at least the arena plan's pairs)
    assert names.count(name) >= len(BDC.NET_BLOCKS), names.count(name)

    fused = G._net(model, mode, options={"fuse_block": 4})
    got = _outputs(fused, frames)
    assert _dw_blocks(fused, mode) == list(BDC.NET_BLOCKS), _dw_blocks(fused, mode)
    cp = fused._last_plan
    _assert_no_pair_in_place(cp, BDC.NET_BLOCKS)
    blk, c, ld = BDC.NET_ROUTE_SLICE
    z = next(cp.ops[n + 1] for n in range(cp.n_ops - 1) if int(cp.ops[n].block_idx) == blk)
    assert (z.out_c, z.out_ld) == (c, ld) and z.flags & _hip.F_RESIDUAL          # a pair that writes a slice of a route buffer
    again = _outputs(fused, frames)
    keep = G._net(model, mode, options={"fuse_block": 4}, keep_all=True, fuse=True)
    kept = _outputs(keep, frames)
    assert set(BDC.NET_BLOCKS) <= set(_dw_blocks(keep, mode))
    plain = G._net(model, mode, options={"fuse_block": 0})
    want = _outputs(plain, frames)
    assert not any("conv_block" in r["kernel"] for r in plain.plan_report())
    for k in KEYS:
        assert torch.equal(got[k], want[k]), "%s differs from the network under fuse_block = 0" % k
        assert torch.equal(again[k], got[k]), "%s differs on the second forward" % k
        assert torch.equal(kept[k], got[k]), "%s: the arena run differs from the keep-all run" % k
    assert bool(torch.isfinite(got["class_prob"]).all())


def _net_608(options):
    import yolov3
    from golden_util import MODELS
    from yolov3 import weights as W
    net = yolov3.Darknet(MODELS["yolov3"], device="cuda", dtype="bf16", options=options).eval()
    return net.set_params(W.synth_params(net.blocks, net.net_info, seed=0, obj_bias=-8.5, calib=W.load_calibration("yolov3")))


def test_the_shipped_shape_equals_the_two_launches():
    """yolov3 608 bf16 at batch 16 under what a Pipeline passes (fuse_block = 3, the 256-pixel strip tiles): 256 rectangles per
    pair, one round on 256 CUs; three runs, each bit-identical to the network under fuse_block = 0 with the same mask"""
    from yolov3 import _hip
    from yolov3.synthdata import synth_frames
    _hip.require_gpu()
    mask = int(_hip.options().auto_mask) | _hip.AM_HALO_TILE256
    frames = torch.from_numpy(synth_frames(4321, 16, 608, 608)).cuda()
    outs = {}
    for mode in (0, 3):
        net = _net_608({"fuse_block": mode, "auto_mask": mask})
        runs = [_outputs(net, frames) for _ in range(3)]
        for k in KEYS:
            assert torch.equal(runs[0][k], runs[1][k]) and torch.equal(runs[0][k], runs[2][k]), (mode, k)
        outs[mode] = runs[0]
        blocks = _dw_blocks(net, "bf16")
        assert (len(blocks) >= 8) == (mode == 3), (mode, blocks)
        if mode == 3:
            _assert_no_pair_in_place(net._last_plan, blocks)
        del net
    for k in KEYS:
        assert torch.equal(outs[0][k], outs[3][k]), k
    assert bool(torch.isfinite(outs[3]["class_prob"]).all())


def test_a_pipeline_with_batches_in_flight_selects_the_kernel_by_default():
    """in_flight > 1 and no options: fuse_block = 3, and every plan names the kernel on the 76 x 76 pairs; explicit options, or
    a network whose own options hold fuse_block, keep what they were given"""
    import warnings

    from yolov3 import _hip
    from yolov3.pipeline import Pipeline
    _hip.require_gpu()
    lib = _hip.lib()

    def pairs(pipe):
        out = []
        for cp in pipe.plans:
            ix = [i for i in range(cp.n_ops) if lib.y3_plan_op_kernel(cp.handle, i).decode() == "conv_block_dw_bf16_x128"]
            assert all((cp.ops[i].in_h, cp.ops[i].in_w) == (76, 76) for i in ix)
            out.append(len(ix))
        return out

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # (the hardware-queue advice, where the runtime has few)
        net = _net_608(None)
        pipe = Pipeline(net, 16, in_flight=2)
        assert pipe.options["fuse_block"] == 3 and pipe.options["auto_mask"] & _hip.AM_HALO_TILE256
        assert len(pipe.plans) == 2 and all(n >= 8 for n in pairs(pipe)), pairs(pipe)
        off = Pipeline(net, 16, in_flight=2, options={"fuse_block": 0})
        assert off.options == {"fuse_block": 0} and pairs(off) == [0, 0]
        del pipe, off
        own = _net_608({"fuse_block": 0})
        kept = Pipeline(own, 16, in_flight=2)
        assert kept.options["fuse_block"] == 0 and pairs(kept) == [0, 0]
        one = Pipeline(own, 16, in_flight=1)
        assert one.options is None
