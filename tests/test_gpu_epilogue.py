"""Every conv epilogue on planted pre-activations, bit for bit (-m gpu).

Zero conv weights make the accumulator +0 in every kernel, so channel c's pre-activation is its folded bias, bit for bit, at
every pixel; tests/epilogue_cases.py holds the planted values and what each must become.  Linear and leaky are demanded
exactly; mish and logistic must land on a storage value that a float32 result within the project's bound (4 float32 ulp or
1e-6 of the float64 function) can round to.

A conv that reads a non-finite activation has a NaN accumulator (0 * inf), so every conv block of the family network is
checked in a forward of its own: the complete list in that block, finite-only lists in the blocks before it.  The plan is
built once per test; between forwards only the device copies of scale and bias change (Darknet.update_bn).

The family network has no channel count off the 16-byte chunk, so it never reaches the direct fallback: ``conv_direct_*`` gets
the whole list in a one-op plan of its own (test_direct_conv_epilogue), with a shortcut operand and with float32 output too.
"""
import ctypes

import numpy as np
import pytest
import torch

import yolov3
from yolov3 import _hip
from yolov3.synthdata import synth_frames

import epilogue_cases as E
import yolov4_restate as R
from test_gpu_yolov4_families import FAMILY_CFG, FAMILY_DIM, FAMILY_RUNS, HEAD, _conv, _net, _params, _run, _write

pytestmark = pytest.mark.gpu

RUN_NAMES = [r[0] for r in FAMILY_RUNS]
# kernels that keep their first conv's output on chip: that epilogue is checked through the second conv in the fused-kernel
# tests below, not in the family network
ON_CHIP = ("conv_stem_s2_fused", "conv_resblock_fused", "conv_block_fused")
FUSED_DTYPES = ("bf16", "fp16")       # the storage types the fused-kernel tests below run
TAG = {"bf16": "bf16", "fp16": "f16"}
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _cfg_text(act):
    return FAMILY_CFG.replace("activation=mish", "activation=" + act)


def _planted_params(base, convs, act, dtype, run, checked):
    """parameter dicts with zero weights and the planted BN shift: the complete list (or the searched shortcut cases) in conv
    block ``checked``, finite-only values in every other.  Returns (params, t of the checked block, tags, r or None)."""
    out, info = [], None
    for slot, (blk, ch) in enumerate(convs):
        p = dict(base[slot])
        if blk == HEAD:
            out.append(p)
            continue
        r = None
        if blk == checked and blk in E.RESIDUAL_FROM and act in ("linear", "leaky"):
            t, tags, r = E.residual_layer(act, dtype, run, blk, ch)
        else:
            t, idx = E.layer_values(act, run, blk, ch)
            tags = [E.cases(act)[i].tag for i in idx]
            if blk != checked:
                # (a residual block before the checked one: its sum with the operand must stay finite as well)
                t = np.full(ch, E.FILLER, dtype=np.float32) if blk in E.RESIDUAL_FROM else E.finite_only(act, dtype, t)
        neg = np.asarray([g == E.NEG_SCALE_TAG for g in tags]) & (E.bits(t) == 0x80000000)
        p["weight"] = np.zeros_like(p["weight"])
        p["bn_beta"] = t.astype(np.float32)
        p["bn_mean"] = np.where(neg, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        p["bn_gamma"] = np.where(neg, -np.abs(p["bn_gamma"]), np.abs(p["bn_gamma"])).astype(np.float32)
        if blk == checked:
            info = (t.astype(np.float32), tags, r)
        out.append(p)
    return (out,) + info


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.view(1, -1, 1, 1)


def _gate(got, lo, hi, nan, what, tags, t):
    """got: (B, C, H, W) float32 on the device; lo / hi / nan per channel (epilogue_cases.expect)"""
    gb = got.contiguous().view(torch.int32)
    lo_t, hi_t = _dev(lo), _dev(hi)
    lob, hib = _dev(E.bits(lo).view(np.int32)), _dev(E.bits(hi).view(np.int32))
    nan_t, exact = _dev(nan), lob == hib
    ok = torch.where(nan_t, torch.isnan(got), torch.where(exact, gb == lob, (got >= lo_t) & (got <= hi_t)))
    n_bad = int((~ok).sum())
    if n_bad:
        where = (~ok).nonzero()[:8].cpu().numpy()
        lines = ["%s: %d of %d values miss" % (what, n_bad, ok.numel())]
        for b, c, y, x in where:
            lines.append("  frame %d pixel (%d, %d) channel %d [%s] t = %r (%08x): got %08x (%r), want %08x .. %08x%s" % (
                b, y, x, c, tags[c], float(t[c]), int(E.bits(t[c])), int(gb[b, c, y, x]) & 0xffffffff, float(got[b, c, y, x]),
                int(E.bits(lo[c])), int(E.bits(hi[c])), " (NaN)" if nan[c] else ""))
        print("\n".join(lines))
        pytest.fail("\n".join(lines))


def _uniform_channels(x, what):
    """(C,) float32: the value every pixel of every frame of x holds in its channel, bit for bit"""
    first = x[0, :, 0, 0]
    assert bool((x.view(torch.int32) == first.view(torch.int32).view(1, -1, 1, 1)).all()), what + ": not one value per channel"
    return first.cpu().numpy()


def _kernels(net):
    kernel_of = {}
    for r in net.plan_report():
        kernel_of.setdefault(r["block"], []).append(r["kernel"])
    return kernel_of


@pytest.mark.filterwarnings("ignore:dtype='fp16'. non-finite outputs")      # planted on purpose: the head reads inf and NaN
@pytest.mark.parametrize("run", RUN_NAMES)
@pytest.mark.parametrize("act", E.ACTS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_epilogue_on_every_conv_family(tmp_path, dtype, act, run):
    run_idx = RUN_NAMES.index(run)
    _, options, batch = FAMILY_RUNS[run_idx]
    cfg = _write(tmp_path, _cfg_text(act), "family.cfg")
    base = _params(cfg)
    ref = R.Restatement(cfg, base)
    blocks = ref.blocks
    rounds = ref.rounding_points()            # False: the conv's only reader is the shortcut after it, ONE rounding of a + r
    convs = [(i, int(b["filters"])) for i, b in enumerate(blocks) if b["type"] == "convolutional"]
    frames = synth_frames(700 + batch, batch, FAMILY_DIM, FAMILY_DIM)
    sel = sorted(set([0, batch - 1]))
    f32_input = dtype == "float32"
    lib = _hip.lib()
    x_in = R.frames_to_input(frames).cuda() if f32_input else None
    net, kernel_of, checked, on_chip = None, None, [], []
    for blk, ch in convs:
        if blk == HEAD:
            continue
        params, t, tags, r = _planted_params(base, convs, act, dtype, run_idx, blk)
        if net is None:
            net = _net(cfg, dtype, params, options)
        else:
            net.update_bn(params)
            torch.cuda.synchronize()
        _run(net, frames, f32_input)
        if kernel_of is None:
            kernel_of = _kernels(net)
            print("%s %s %s: %s" % (dtype, act, run, {b: k[0] for b, k in sorted(kernel_of.items())}))
        cp = net._last_plan
        op = [cp.ops[n] for n in range(cp.n_ops) if cp.ops[n].kind == _hip.OP_CONV and cp.ops[n].block_idx == blk][0]
        what = "%s %s %s block %d (%s)" % (dtype, act, run, blk, kernel_of[blk][0])
        # the fold gives the planted value as bias, bit for bit
        _, bias = net._fold_bn(net_slot(convs, blk))
        assert (E.bits(bias) == E.bits(t)).all(), what
        if f32_input:
            # the premise on the GPU: the conv once more as a linear, shortcut-free op gives its bias at every pixel
            lin = _hip.Y3Op()
            ctypes.memmove(ctypes.byref(lin), ctypes.byref(op), ctypes.sizeof(lin))
            lin.flags &= ~(_hip.F_LEAKY | _hip.F_MISH | _hip.F_LOGISTIC | _hip.F_RESIDUAL | _hip.F_FUSE_NEXT)
            lin.d_res = None
            buf = torch.zeros(batch * op.out_h * op.out_w * op.out_ld, dtype=torch.float32, device="cuda")
            lin.d_out = buf.data_ptr()
            _hip.check(lib.y3_op_run(ctypes.byref(lin), x_in.data_ptr(), net._zero.data_ptr(), _hip.stream_ptr()))
            torch.cuda.synchronize()
            pre = buf.view(batch, op.out_h, op.out_w, op.out_ld)[..., :op.out_c].permute(0, 3, 1, 2)[sel]
            _gate(pre, t, t, np.isnan(t), what + " pre-activation", tags, t)
        # the restatement says where the sum is rounded once; a plan that runs such a shortcut as a kernel of its own (and says
        # so: no F_RESIDUAL on the conv) is held to rnd(rnd(a) + r) below, and no plan may fuse a shortcut anywhere else
        fused = bool(op.flags & _hip.F_RESIDUAL)
        assert (blk in E.RESIDUAL_FROM) == (not rounds[blk]) and (not fused or not rounds[blk]), what
        if fused != (not rounds[blk]):
            print(what + ": shortcut runs as its own kernel, " + kernel_of[blk + 1][0])
        if kernel_of[blk][0].startswith(ON_CHIP):
            assert dtype in FUSED_DTYPES, what + ": no test shows this on-chip epilogue"
            on_chip.append(blk)               # the first conv of a fused pair: its output never reaches memory
            continue
        assert cp.desc["tensor_of"][blk + 1 if fused else blk] is not None, what + ": output not in memory"
        if blk in E.RESIDUAL_FROM:
            src = net.block_output(E.RESIDUAL_FROM[blk])[sel]
            got_r = _uniform_channels(src, what + " shortcut operand")
            if r is None:
                r = got_r                     # mish / logistic: the operand as the product stored it (gated in its own forward)
            assert (E.bits(r) == E.bits(got_r)).all() and np.isfinite(r).all(), what + " shortcut operand"
            if fused:
                _gate(net.block_output(blk + 1)[sel], *E.expect(act, dtype, t, r, fused=True), what + " + shortcut", tags, t)
            else:
                _gate(net.block_output(blk)[sel], *E.expect(act, dtype, t), what, tags, t)
                _gate(net.block_output(blk + 1)[sel], *E.expect(act, dtype, t, r, fused=False),
                      what + " + shortcut (%s)" % kernel_of[blk + 1][0], tags, t)
        else:
            assert not fused
            _gate(net.block_output(blk)[sel], *E.expect(act, dtype, t), what, tags, t)
        checked.append(blk)
    # every conv block was checked under the kernel that ran it, or runs inside a kernel the fused-kernel tests cover
    assert sorted(checked + on_chip) == [b for b, _ in convs if b != HEAD], (checked, on_chip)
    names = [k for b, ks in sorted(kernel_of.items()) for k in ks]
    del net
    if act in ("mish", "logistic"):
        # the plan is the one this run has on natural weights in test_mish_on_every_conv_family: weights do not choose kernels
        assert not on_chip
        mish_cfg = _write(tmp_path, FAMILY_CFG, "family_mish.cfg")
        nat = _net(mish_cfg, dtype, _params(mish_cfg), options)
        _run(nat, frames, f32_input)
        want = [k for b, ks in sorted(_kernels(nat).items()) for k in ks]
        assert names == want, (names, want)


def net_slot(convs, blk):
    return [b for b, _ in convs].index(blk)


# ---- the fused kernels with epilogues of their own ------------------------------------------------------------------------
# Hand-built two-op plans of tests/test_gpu_parity.py and tools/block_bench.py in both 16-bit storage
# types, leaky and linear (the kernels decline mish and logistic).  First the first conv's epilogue, whose result stays on
# chip: zero weights and a planted bias there, and a second conv whose output channel c reads intermediate channel c mod C_mid
# with weight 1.0 at the centre tap, scale 1, bias 0 -- its sum is that one product and zeros, so it shows the first
# epilogue's rounded value: act2(rnd(act1(t1))) (+ r).  Only finite intermediates can be shown this way (0 * inf).  Then the
# second conv's epilogue: everything zero but its bias.
PAIR_CFG = ("[net]\nwidth=96\nheight=96\nchannels=3\n\n" + _conv(32, 3, 1, "leaky", bn=False) + _conv(64, 3, 2, "leaky", bn=False) +
            _conv(32, 1, 1, "leaky", bn=False) + _conv(64, 3, 1, "leaky", bn=False) + "[shortcut]\nfrom=-3\nactivation=linear\n\n" +
            _conv(18, 1, act="linear", bn=False) + "[yolo]\nmask=0,1,2\nanchors=10,14, 23,27, 37,58\nclasses=1\nnum=3\n")
PAIR_SHAPES = ((32, 3, 3), (64, 32, 3), (32, 64, 1), (64, 32, 3), (18, 64, 1))      # (cout, cin, k) of its convs


def _identity(cout, cin, k):
    w = np.zeros((cout, cin, k, k), dtype=np.float32)
    w[np.arange(cout), np.arange(cout) % cin, k // 2, k // 2] = 1.0
    return w


def _pair_net(tmp_path, planted, dtype):
    """PAIR_CFG with zero weights and biases but for ``planted``: {conv slot: (weight or None, bias or None)}"""
    net = yolov3.Darknet(_write(tmp_path, PAIR_CFG, "pair.cfg"), device="cuda", dtype=dtype)
    params = []
    for slot, (co, ci, k) in enumerate(PAIR_SHAPES):
        w, b = planted.get(slot, (None, None))
        params.append({"weight": np.zeros((co, ci, k, k), dtype=np.float32) if w is None else w,
                       "bias": np.zeros(co, dtype=np.float32) if b is None else np.asarray(b, dtype=np.float32)})
    return net.set_params(params)


def _plus0(t):
    """the pre-activation a bias gives under a positive scale: +0 * scale + bias (a bias of -0 gives +0)"""
    with np.errstate(invalid="ignore"):
        return (E.f32(t) + np.float32(0)).astype(np.float32)


def _through(dtype, act1, act2, t1, n_out, r=None):
    """what the second conv stores when it reads the first epilogue's on-chip value through an identity centre tap"""
    mid = E.RND[dtype](E.act_exact(act1, _plus0(t1)))
    assert np.isfinite(mid).all()
    return E.expect(act2, dtype, _plus0(mid[np.arange(n_out) % mid.size]), r)


def _chunks(act, width):
    t, idx = E.padded(act)
    tags = [E.cases(act)[i].tag for i in idx]
    return [(t[k:k + width], tags[k:k + width]) for k in range(0, E.LIST_LEN, width)]


def _nchw(out):
    return (out if isinstance(out, torch.Tensor) else torch.from_numpy(out)).cuda().float().permute(0, 3, 1, 2)


# (leaky, leaky) only: the stem-pair and residual-block choosers take no other activation (both ops must carry F_LEAKY:
# y3_choose_conv_fused_stem_s2 / y3_choose_conv_fused_resblock in csrc/conv_fused.hip); the bottleneck kernel takes linear too
@pytest.mark.parametrize("fuse_stem", [1, 2])
@pytest.mark.parametrize("dim", [96, 80])
@pytest.mark.parametrize("dtype", FUSED_DTYPES)
def test_fused_stem_pair_epilogues(tmp_path, dtype, dim, fuse_stem):
    from test_gpu_parity import _first_two_convs_plan
    lib = _hip.lib()
    frames = synth_frames(9 + dim, 1, dim, dim)
    try:
        _hip.check(lib.y3_set_tuning(b"fuse_stem", fuse_stem))
        for n, (t, tags) in enumerate(_chunks("leaky", 32)):          # the stem conv's epilogue, through the stride-2 conv
            t1 = E.finite_only("leaky", dtype, t)
            net = _pair_net(tmp_path, {0: (None, t1), 1: (_identity(64, 32, 3), None)}, dtype)
            out, name = _first_two_convs_plan(net, frames, True, net._torch_device(), dtype)
            assert name == "conv_stem_s2_fused_u8_" + TAG[dtype]
            _gate(_nchw(out), *_through(dtype, "leaky", "leaky", t1, 64), "%s fuse_stem %d first epilogue, chunk %d" % (name, fuse_stem, n),
                  (tags * 2), np.tile(t1, 2))
        for n, (t, tags) in enumerate(_chunks("leaky", 64)):          # the stride-2 conv's own epilogue
            net = _pair_net(tmp_path, {1: (None, t)}, dtype)
            out, name = _first_two_convs_plan(net, frames, True, net._torch_device(), dtype)
            assert name == "conv_stem_s2_fused_u8_" + TAG[dtype]
            _gate(_nchw(out), *E.expect("leaky", dtype, _plus0(t)), "%s fuse_stem %d second epilogue, chunk %d" % (name, fuse_stem, n),
                  tags, t)
    finally:
        lib.y3_set_tuning(b"fuse_stem", 1)


def _operand(n, seed, dtype):
    """n finite shortcut operands of mixed size and sign, values of the storage type"""
    rng = np.random.RandomState(seed)
    return E.RND[dtype]((rng.standard_normal(n) * 10.0 ** rng.randint(-2, 3, n)).astype(np.float32))


@pytest.mark.parametrize("dim,batch", [(48, 2), (40, 1)])
@pytest.mark.parametrize("dtype", FUSED_DTYPES)
def test_fused_residual_block_epilogues(tmp_path, dtype, dim, batch):
    from test_gpu_parity import _resblock_plan
    r = _operand(64, dim, dtype)
    x = torch.from_numpy(r).to(TORCH_DTYPE[dtype]).cuda().view(1, 1, 1, 64).expand(batch, dim, dim, 64).contiguous()
    want_name = "conv_resblock_fused_%s_64_32_64" % TAG[dtype]
    for n, (t, tags) in enumerate(_chunks("leaky", 32)):              # the 1x1's epilogue, through the 3x3 and the shortcut add
        t1 = E.finite_only("leaky", dtype, t)
        net = _pair_net(tmp_path, {2: (None, t1), 3: (_identity(64, 32, 3), None)}, dtype)
        out, name = _resblock_plan(net, x, True, net._torch_device(), dtype)
        assert name == want_name
        _gate(_nchw(out), *_through(dtype, "leaky", "leaky", t1, 64, r), "%s first epilogue, chunk %d" % (name, n), tags * 2, np.tile(t1, 2))
    second = _chunks("leaky", 64)
    ts, stags = E.shortcut_cases("leaky", dtype, r, dim)
    for n, (t, tags) in enumerate(second + [(ts, stags)]):            # the 3x3's epilogue with its fused shortcut
        net = _pair_net(tmp_path, {3: (None, t)}, dtype)
        out, name = _resblock_plan(net, x, True, net._torch_device(), dtype)
        assert name == want_name
        _gate(_nchw(out), *E.expect("leaky", dtype, _plus0(t), r), "%s second epilogue, chunk %d" % (name, n), tags, t)
    assert set(stags) >= {"shortcut: witness", "shortcut: tie", "shortcut: inexact", "shortcut: cancel", "shortcut: inf", "shortcut: nan"}


def _block_pair(h, batch, acts, r, dtype):
    """tests/block_dw_util.py's 1x1 (256 -> 128) + 3x3 (128 -> 256) + shortcut pair (the pair of tools/block_bench.py with the
    fragment-order copies of both weights, which the direct-weights form of the kernel reads) with activations ``acts``, every
    weight and bias zero, both scales 1, and the input (= shortcut operand) r per channel"""
    import block_dw_util as bb
    _hip.require_gpu()
    x = torch.from_numpy(r).view(1, 1, 1, -1).expand(batch, h, h, 256)
    convs = [dict(w=torch.zeros((co, ci, k, k)), scale=torch.ones(co), bias=torch.zeros(co)) for ci, co, k in ((256, 128, 1), (128, 256, 3))]
    t, ops = bb.make_pair(torch.device("cuda:0"), dtype, x, convs, True)
    for n, act in enumerate(acts):
        ops[n].flags = (ops[n].flags & ~_hip.F_LEAKY) | (_hip.F_LEAKY if act == "leaky" else 0)
    assert torch.equal(t["x"].float().cpu()[0, 0, 0], torch.from_numpy(r)) and not bool(t["wf0"].any()) and not bool(t["wf1"].any())
    return bb, t, ops


def _refragment(t, ops):
    """the fragment-order copies of both weights, remade from the weights as they are now: a plan reads the caller's copy, so
    weights rewritten between runs (``t["w1"].copy_``) reach a kernel that reads fragments only through this"""
    import ctypes
    for n in (0, 1):
        _hip.check(_hip.lib().y3_conv_make_fragment_weights(ctypes.byref(ops[n]), ctypes.c_void_p(t["wf%d" % n].data_ptr()), None))
    torch.cuda.synchronize()


def _block_run(bb, t, ops, mode, batch, h, census_key=None):
    """``census_key``: the run is taken with the launch log and held to that entry of the block library's census"""
    import contextlib
    lib = _hip.lib()
    out = torch.full((batch, h, h, 256), 7.0, dtype=t["x"].dtype, device="cuda:0")
    plan = bb.make_plan(ops, t["zero"], out, fuse_block=mode)
    try:
        with (_hip.launch_log() if census_key else contextlib.nullcontext()) as log:
            _hip.check(lib.y3_plan_run(plan, None, _hip.stream_ptr()))
        torch.cuda.synchronize()
        name = lib.y3_plan_op_kernel(plan, 0).decode()
    finally:
        lib.y3_plan_destroy(plan)
    if census_key:
        import kernel_census as census
        assert len(log.symbols) == 1 and "conv_block_dw_kernel" in log.symbols[0], log.symbols
        census.assert_census(census_key, library="block", launched=[log.symbols])
    return out, name


# mode -> the name of the pair's first op: fuse_block = 2 the fused kernel, 4 its direct-weights form (csrc/conv_block_dw.hip,
# which inlines y3_bn_act8 / y3_add8 / y3_pack8 on its own), 0 the two launches
BLOCK_MODES = (2, 0, 4)


def _block_name_ok(name, mode, dtype):
    want = {2: "conv_block_fused_%s_x128", 4: "conv_block_dw_%s_x128"}.get(mode)
    if want is None:
        return not name.startswith("conv_block")
    return name == want % TAG[dtype]


@pytest.mark.parametrize("acts", [("leaky", "leaky"), ("linear", "leaky"), ("leaky", "linear")])
@pytest.mark.parametrize("h,batch", [(20, 2), (9, 3)])
@pytest.mark.parametrize("dtype", FUSED_DTYPES)
def test_fused_bottleneck_block_epilogues(dtype, h, batch, acts):
    import block_dw_cases as BDC
    r = _operand(256, h, dtype)
    bb, t, ops = _block_pair(h, batch, acts, r, dtype)
    key = BDC.epilogue_key(dtype)
    # the 1x1's epilogue: the whole list in its 128 channels, shown by an identity centre tap
    t1, idx = E.padded(acts[0])
    tags = [E.cases(acts[0])[i].tag for i in idx]
    t1 = E.finite_only(acts[0], dtype, t1)
    t["bi0"][:128].copy_(torch.from_numpy(t1))
    w = torch.zeros_like(t["w1"])
    w[torch.arange(256), 4 * 128 + torch.arange(256) % 128] = 1.0
    t["w1"].copy_(w)
    _refragment(t, ops)
    lo, hi, nan = _through(dtype, acts[0], acts[1], t1, 256, r)
    # where the identity tap puts a non-zero value on top of the shortcut operand: a stale copy (zero weights) would store r alone
    shown = ~nan & (lo != r) & (hi != r)
    assert shown.sum() > 100
    r_dev = torch.from_numpy(r).cuda()
    for mode in BLOCK_MODES:
        out, name = _block_run(bb, t, ops, mode, batch, h, key if mode == 4 else None)
        assert _block_name_ok(name, mode, dtype), (mode, name)
        _gate(_nchw(out), lo, hi, nan, "%s %s first epilogue" % (name, acts), tags * 2, np.tile(t1, 2))
        # ... which says that the fragment-order copy was remade after the weights were rewritten; read it all the same: the zero
        # weights the copy held before would leave the shortcut operand alone
        assert bool((out.float() - r_dev)[..., torch.from_numpy(shown).cuda()].ne(0).all()), "%s: a stale fragment-order copy (zero weights)" % name
    # the 3x3's epilogue with the fused shortcut: the whole list, then the searched shortcut cases
    t2, idx = E.padded(acts[1])
    ts, stags = E.shortcut_cases(acts[1], dtype, r[128:], h)
    t2, tags = np.concatenate([t2, ts]), [E.cases(acts[1])[i].tag for i in idx] + stags
    t["bi0"].zero_()
    t["w1"].zero_()
    _refragment(t, ops)
    assert not bool(t["wf1"].any())
    t["bi1"][:256].copy_(torch.from_numpy(t2))
    for mode in BLOCK_MODES:
        out, name = _block_run(bb, t, ops, mode, batch, h, key if mode == 4 else None)
        assert _block_name_ok(name, mode, dtype), (mode, name)
        _gate(_nchw(out), *E.expect(acts[1], dtype, _plus0(t2), r), "%s %s second epilogue" % (name, acts), tags, t2)


@pytest.mark.parametrize("act", ["linear", "leaky"])
@pytest.mark.parametrize("dtype", FUSED_DTYPES)
def test_shortcut_operand_non_finite(dtype, act):
    """inf + -inf, finite + NaN, NaN + inf: a conv that reads its shortcut operand from a tensor of its own (the two launches of
    the bottleneck pair; the fused kernels and the networks take the operand from an input of the chain, which must be finite)"""
    h, batch = 9, 2
    bb, t, ops = _block_pair(h, batch, (act, act), np.full(256, 0.5, dtype=np.float32), dtype)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    pairs = [(inf, -inf), (-inf, inf), (np.float32(1.5), nan), (nan, inf), (inf, inf), (-inf, np.float32(2.0)), (nan, nan),
             (np.float32(-3.0), -inf)]
    t2 = np.asarray([pairs[c % len(pairs)][0] for c in range(256)], dtype=np.float32)
    r2 = np.asarray([pairs[c % len(pairs)][1] for c in range(256)], dtype=np.float32)
    tags = ["shortcut: %r + %r" % (float(a), float(b)) for a, b in zip(t2, r2)]
    res = torch.from_numpy(r2).to(TORCH_DTYPE[dtype]).cuda().view(1, 1, 1, -1).expand(batch, h, h, 256).contiguous()
    ops[1].d_res, ops[1].res_ld = res.data_ptr(), 256
    t["bi1"][:256].copy_(torch.from_numpy(t2))
    out, name = _block_run(bb, t, ops, 0, batch, h)
    lo, hi, isnan = E.expect(act, dtype, t2, r2)
    assert isnan[0] and isnan[2] and np.isinf(lo[4])
    _gate(_nchw(out), lo, hi, isnan, "%s %s non-finite shortcut operand" % (name, act), tags, t2)


# ---- the direct fallback --------------------------------------------------------------------------------------------------
# conv_direct_kernel (csrc/conv_small.hip) narrows through y3_from_float<T> on a path of its own, and the family network never
# reaches it (no odd channel count): a one-op plan through the C ABI, 1x1 conv 13 -> 128 channels on a 2 x 5 x 7 map, zero
# weights and a finite input, so the pre-activation of channel c is +0 * scale[c] + bias[c] = the planted t[c]; the -0 entry
# gets scale -1 (+0 * -1 = -0, and -0 + -0 = -0), every other entry scale +1.
DIRECT_DTYPES = {"float32": (_hip.Y3_F32, torch.float32, "f32"), "bf16": (_hip.Y3_BF16, torch.bfloat16, "bf16"),
                 "fp16": (_hip.Y3_F16, torch.float16, "f16")}
ACT_FLAG = {"linear": 0, "leaky": _hip.F_LEAKY, "mish": _hip.F_MISH, "logistic": _hip.F_LOGISTIC}
DIRECT_SHAPE = (2, 5, 7, 13, 128)          # B, h, w, cin, cout


def _direct_conv(dtype, act, t, tags, r=None, out_f32=False):
    """(stored output as (B, C, H, W) float32 on the device, kernel name) of the one-op plan with pre-activations ``t`` (one
    per channel), shortcut operand ``r`` per channel or None, and float32 output from 16-bit storage with ``out_f32``"""
    _hip.require_gpu()
    lib = _hip.lib()
    B, h, w, cin, cout = DIRECT_SHAPE
    code, tdt, _ = DIRECT_DTYPES[dtype]
    es = 4 if dtype == "float32" else 2
    k_ld = -(-cin // (128 // es)) * (128 // es)
    dev = torch.device("cuda:0")
    x = (torch.rand((B, h, w, cin), generator=torch.Generator().manual_seed(13)) - 0.5).to(tdt).to(dev)
    wgt = torch.zeros((cout, k_ld), dtype=tdt, device=dev)
    neg = np.asarray([g == E.NEG_SCALE_TAG for g in tags]) & (E.bits(t) == 0x80000000)
    scale = torch.from_numpy(np.where(neg, -1.0, 1.0).astype(np.float32)).to(dev)
    bias = torch.from_numpy(E.f32(t).copy()).to(dev)
    out = torch.full((B, h, w, cout), 7.0, dtype=torch.float32 if out_f32 else tdt, device=dev)
    zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
    op = _hip.Y3Op()
    op.kind, op.dtype, op.batch, op.block_idx = _hip.OP_CONV, code, B, 1
    op.flags = ACT_FLAG[act] | (_hip.F_OUT_F32 if out_f32 else 0) | (_hip.F_RESIDUAL if r is not None else 0)
    op.in_h, op.in_w, op.in_c, op.in_ld = h, w, cin, cin
    op.out_h, op.out_w, op.out_c, op.out_ld = h, w, cout, cout
    op.ksize, op.stride, op.pad = 1, 1, 0
    op.cout_pad, op.k_ld = cout, k_ld
    op.d_in, op.d_out = x.data_ptr(), out.data_ptr()
    op.d_weight, op.d_scale, op.d_bias = wgt.data_ptr(), scale.data_ptr(), bias.data_ptr()
    if r is not None:
        res = torch.from_numpy(E.f32(r).copy()).to(tdt).to(dev).view(1, 1, 1, -1).expand(B, h, w, cout).contiguous()
        op.d_res, op.res_ld = res.data_ptr(), cout
    ops = (_hip.Y3Op * 1)(op)
    handle = ctypes.c_void_p()
    _hip.check(lib.y3_plan_create_ex(ops, 1, zero.data_ptr(), None, ctypes.byref(handle)))
    try:
        name = lib.y3_plan_op_kernel(handle, 0).decode()
        _hip.check(lib.y3_plan_run(handle, x.data_ptr(), _hip.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    return out.float().permute(0, 3, 1, 2).contiguous(), name


@pytest.mark.parametrize("act", E.ACTS)
@pytest.mark.parametrize("dtype", E.DTYPES)
def test_direct_conv_epilogue(dtype, act):
    want_name = "conv_direct_" + DIRECT_DTYPES[dtype][2]
    t, idx = E.padded(act)
    tags = [E.cases(act)[i].tag for i in idx]
    assert E.NEG_SCALE_TAG in tags and len(t) == DIRECT_SHAPE[4]
    got, name = _direct_conv(dtype, act, t, tags)
    assert name == want_name, name
    _gate(got, *E.expect(act, dtype, t), "%s %s %s" % (name, dtype, act), tags, t)
    if dtype != "float32":
        # Y3_F_OUT_F32: the value stored is the float32 result, not narrowed
        got, name = _direct_conv(dtype, act, t, tags, out_f32=True)
        assert name == want_name, name
        _gate(got, *E.expect(act, "float32", t), "%s %s %s, float32 out" % (name, dtype, act), tags, t)
    if act in ("linear", "leaky"):
        # the shortcut operand is added in float32 before the one store (`v += res`): one rounding of the sum
        r = _operand(DIRECT_SHAPE[4], 13, dtype)
        ts, stags = E.shortcut_cases(act, dtype, r, 13)
        got, name = _direct_conv(dtype, act, ts, stags, r=r)
        assert name == want_name, name
        _gate(got, *E.expect(act, dtype, ts, r, fused=True), "%s %s %s + shortcut" % (name, dtype, act), stags, ts)
        # (float32 storage has no tie and no witness of a second rounding: E.shortcut_cases plants those as "plain")
        kinds = {"shortcut: inexact", "shortcut: cancel", "shortcut: inf", "shortcut: nan"}
        assert set(stags) >= kinds | (set() if dtype == "float32" else {"shortcut: witness", "shortcut: tie"}), sorted(set(stags))
