"""The planner's graph decisions through ``Darknet`` on the GPU (-m gpu): tests/golden/cfg/graph_*.cfg, batch 2, 32 x 48.

tests/test_plan_graph_host.py pins which decision each cfg reaches and runs the plans on a CPU arena; here the same plans run as
``y3_op``s, through ``Darknet._compile``'s addresses and strides and the executor's fused groups.

Every block, ``keep_all=True, fuse=True``:

* float32: every block against the float64-accumulating forward by block index (tests/plan_interp.py ``reference_blocks``) at
  the tolerances of tests/test_gpu_odd_cfg.py, boxes and scores likewise.
* bf16 / fp16: every conv teacher-forced at one storage ulp (tests/test_gpu_bf16.py ``_close_bf16``), heads through the decode.
* routes, copies, pools, upsamples and reorgs: bit for bit the same operation on the HIP run's own inputs, in every dtype.
* every ``add``: bit for bit the single rounding of a + b, both taken from the HIP run.  A shortcut fused into its conv has no
  ``a`` in memory: there ``a`` is the conv teacher-forced on the HIP run's input, ``b`` the HIP run's, at the conv's tolerance.
* the kernels of the fusion near-misses of graph_pools.cfg, by name.

Arena on, ``keep_all=False`` (what users run): the same kernels by name, outputs ``torch.equal`` to the keep-all run's, and a
second forward on the same plan equal to the first.

graph_heads.cfg runs in float32 only; in bf16 / fp16 ``forward`` must raise before anything is launched.
"""
import numpy as np
import pytest
import torch

import yolov3
from oracle import darknet_oracle as orc

import plan_interp as PI
import yolov2_restate as R2
import yolov4_restate as R4
from test_gpu_bf16 import MODES, _close_bf16, _flip_slack

pytestmark = pytest.mark.gpu

DTYPES = ("float32", "bf16", "fp16")
CASES = [(name, dtype) for name in PI.GRAPH_CFGS for dtype in DTYPES if dtype == "float32" or name not in PI.F32_ONLY]
_runs = {}
_refs = {}


def _net(name, dtype, keep_all):
    case = PI.graph_case(name)
    kw = dict(keep_all=True, fuse=True) if keep_all else {}
    return yolov3.Darknet(case["path"], device="cuda", dtype=dtype, **kw).set_params(case["params"]).eval()


def _names(net):
    return [(r["block"], r["kernel"]) for r in net.plan_report()]


def _keep_all_run(name, dtype):
    """(net, outputs on the CPU, [(block, kernel)]) of the keep-all run; made once per case and left unchanged"""
    if (name, dtype) not in _runs:
        net = _net(name, dtype, True)
        out = net.forward_frames(PI.graph_case(name)["frames"])
        torch.cuda.synchronize()
        _runs[name, dtype] = (net, {k: v.cpu() for k, v in out.items()}, _names(net))
    return _runs[name, dtype]


def _reference_f32(name):
    if name not in _refs:
        case = PI.graph_case(name)
        _refs[name] = PI.reference_blocks(case["path"], case["params"], case["x"], accumulate="f64")
    return _refs[name]


def _check_pool_kernels(kernel_of, dtype):
    """graph_pools.cfg: which groups the fused kernels take"""
    def single(blocks):
        return all(len(kernel_of[b]) == 1 and "spp" not in kernel_of[b][0] and not kernel_of[b][0].startswith("(fused")
                   for b in blocks)

    assert kernel_of[2][0].startswith("maxpool_spp_pyramid_"), kernel_of[2]          # 13 / 9 / 5
    assert kernel_of[4][0].startswith("(fused") and kernel_of[6][0].startswith("(fused"), (kernel_of[4], kernel_of[6])
    assert single((9, 11, 13)), [kernel_of[b] for b in (9, 11, 13)]                  # 5 / 9 / 9
    assert single((16, 17, 18)), [kernel_of[b] for b in (16, 17, 18)]                # cascade
    if dtype == "float32":           # 24 channels are 96 bytes: three 32-byte channel groups
        assert kernel_of[21][0].startswith("maxpool_spp_pyramid_"), kernel_of[21]
    else:                            # 48 bytes: in_c % (2 * vec) fails
        assert single((21, 23, 25)), [kernel_of[b] for b in (21, 23, 25)]
    for b in (33, 34, 41, 42):       # shortcut not from the pair's input; a second reader of the 1x1
        assert "resblock" not in kernel_of[b][0] and not kernel_of[b][0].startswith("(fused"), (b, kernel_of[b])
    if dtype != "float32":           # the pair as Darknet-53 has it
        assert kernel_of[37][0].startswith("conv_resblock_fused_") and kernel_of[38][0].startswith("(fused"), (
            kernel_of[37], kernel_of[38])


@pytest.mark.parametrize("name,dtype", CASES)
def test_every_block(name, dtype):
    case = PI.graph_case(name)
    net, out, names = _keep_all_run(name, dtype)
    kernel_of = {}
    for b, k in names:
        kernel_of.setdefault(b, []).append(k)
    print("%s %s: %s" % (name, dtype, {b: ",".join(k) for b, k in sorted(kernel_of.items())}))
    if name == "graph_pools":
        _check_pool_kernels(kernel_of, dtype)
    blocks, params = case["blocks"], case["params"]
    restate = R4.Restatement(case["path"], params)
    slot = restate.slot
    f32 = dtype == "float32"
    mode = None if f32 else dtype
    rnd = (lambda t: t) if f32 else MODES[mode]["rnd"]
    emulate = None if f32 else MODES[mode]["emulate"]
    tensor_of = net._last_plan.desc["tensor_of"]
    want = _reference_f32(name) if f32 else None
    x_net = rnd(case["x"])
    cache = {}

    def hip(i):
        if i < 0:
            return x_net
        if i not in cache:
            cache[i] = net.block_output(i).cpu()
        return cache[i]

    def conv(i, x):
        blk = blocks[i]
        k = blk["size"]
        return orc.conv_block(x, params[slot[i]], blk["stride"], (k - 1) // 2 if "pad" in blk else 0, blk["activation"] == "leaky",
                              round_weights=emulate)

    def fused_away(i):
        return kernel_of.get(i, [""])[0].startswith("(fused")

    def close(got, ref, what, slack=None):
        if f32:
            np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=1e-4, atol=2e-5, err_msg=what)
        else:
            _close_bf16(got, rnd(ref), what, slack, mode)

    checked, heads = 0, []
    for i, blk in enumerate(blocks):
        kind = blk["type"]
        what = "%s %s block %d (%s, %s)" % (name, dtype, i, kind, ",".join(kernel_of.get(i, ["-"])))
        if kind == "convolutional":
            if i > 0 and name not in PI.F32_ONLY and hip(i - 1).shape[1] % 8 == 0:
                assert not kernel_of[i][0].startswith("conv_direct"), what       # on the grain: an MFMA kernel
            nxt = blocks[i + 1]["type"] if i + 1 < len(blocks) else None
            if nxt == "convolutional" and fused_away(i + 1):
                assert not f32, what
                continue                                   # first half of a fused pair: checked with its second half
            slack = None
            if fused_away(i) and blocks[i - 1]["type"] == "convolutional":
                mid = conv(i - 1, hip(i - 2))              # the pair's intermediate tensor stays on chip, rounded to storage
                p2 = params[slot[i]]
                alpha2 = torch.from_numpy(p2["bn_gamma"] / np.sqrt(p2["bn_var"] + orc.BN_EPS))
                slack = _flip_slack(mid, rnd(torch.from_numpy(p2["weight"])), alpha2, blk["stride"],
                                    (blk["size"] - 1) // 2 if "pad" in blk else 0, mode)
                y = conv(i, rnd(mid))
            elif not f32:
                y = conv(i, hip(i - 1))
            if nxt == "yolo":
                heads.append((i + 1, want[i] if f32 else y))    # 16-bit: float32 logits, checked through the decode below
                if f32:
                    close(hip(i), want[i], what)
                checked += 1
                continue
            if tensor_of[i] is None:                       # conv + shortcut in one epilogue, one rounding of the sum
                sc = i + 1
                assert blocks[sc]["type"] == "shortcut", what
                if f32:
                    close(hip(sc), want[sc], what + " + shortcut")
                else:
                    close(hip(sc), y + hip(sc + blocks[sc]["from"]), what + " + shortcut", slack)
            else:
                close(hip(i), want[i] if f32 else y, what, slack)
        elif kind == "shortcut":
            if tensor_of[i - 1] is None:
                continue                                   # checked with its conv
            assert kernel_of[i] and "add" in kernel_of[i][0], what
            assert torch.equal(hip(i), rnd(hip(i - 1) + hip(i + blk["from"]))), what
        elif kind == "maxpool":
            assert torch.equal(hip(i), orc.maxpool(hip(i - 1), blk["size"], blk["stride"])), what
        elif kind == "upsample":
            assert torch.equal(hip(i), orc.upsample(hip(i - 1), blk["stride"])), what
        elif kind == "route":
            assert torch.equal(hip(i), R4.route([hip(j) if j in blk["layers"] else None for j in range(i)], blk)), what
        elif kind == "reorg3d":
            assert torch.equal(hip(i), R2.reorg_block(hip(i - 1), blk)), what
        else:
            assert kind == "yolo", what
            if blocks[i - 1]["type"] != "convolutional":   # float32 only: the logits are another block's output
                assert f32, what
                heads.append((i, want[i]))
            continue
        if f32 and kind != "convolutional":
            close(hip(i), want[i], what)                   # and against the reference in free run
        checked += 1

    heads.sort(key=lambda h: h[0])
    row = 0
    for yi, logits in heads:
        box, prob, idx = restate.decode(yi, logits)
        n = prob.shape[1]
        what = "%s %s head at block %d (%s)" % (name, dtype, yi, ",".join(kernel_of.get(yi - 1, ["-"]) + kernel_of.get(yi, ["-"])))
        box_tol, prob_tol = (dict(rtol=1e-4, atol=1e-5), dict(rtol=1e-4, atol=1e-6)) if f32 else (
            dict(rtol=2e-4, atol=2e-5), dict(rtol=5e-4, atol=2e-5))
        torch.testing.assert_close(out["bbox_xywh"][:, row:row + n], box, msg=lambda m: what + " boxes: " + m, **box_tol)
        torch.testing.assert_close(out["class_prob"][:, row:row + n], prob, msg=lambda m: what + " scores: " + m, **prob_tol)
        assert torch.equal(out["class_idx"][:, row:row + n], idx), what        # one class
        row += n
        checked += 1
    assert row == out["class_prob"].shape[1] and len(heads) == sum(1 for b in blocks if b["type"] == "yolo")
    fused_shortcuts = sum(1 for t in tensor_of if t is None)
    fused_pairs = sum(1 for i, b in enumerate(blocks) if b["type"] == "convolutional" and fused_away(i))
    assert checked == len(blocks) - fused_shortcuts - fused_pairs, (checked, len(blocks), fused_shortcuts, fused_pairs)


@pytest.mark.parametrize("name,dtype", CASES)
def test_arena_reuse_same_kernels_same_outputs_twice(name, dtype):
    _, want, names = _keep_all_run(name, dtype)
    frames = PI.graph_case(name)["frames"]
    net = _net(name, dtype, False)
    first = {k: v.cpu() for k, v in net.forward_frames(frames).items()}
    assert _names(net) == names
    plan = net._last_plan
    second = {k: v.cpu() for k, v in net.forward_frames(frames).items()}
    assert net._last_plan is plan and len(net._plans) == 1
    for k in ("bbox_xywh", "class_prob", "class_idx"):
        assert torch.equal(first[k], want[k]), "%s %s: %s differs from the keep-all run" % (name, dtype, k)
        assert torch.equal(second[k], first[k]), "%s %s: %s differs on the second forward" % (name, dtype, k)
    assert bool(torch.isfinite(first["class_prob"]).all())


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16bit_head_readers_raise_before_any_launch(dtype):
    net = _net("graph_heads", dtype, False)
    with pytest.raises(ValueError, match=r"conv block 2: block 4 \(route\) reads the logits of the head conv of yolo block 3"):
        net.forward_frames(PI.graph_case("graph_heads")["frames"])
    assert net._plans == {} and not hasattr(net, "_last_plan")
