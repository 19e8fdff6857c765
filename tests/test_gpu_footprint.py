"""Every kernel family touches exactly the memory its y3_op describes (tests/footprint_util.py has the layout, the fills and
the case table).  Per case, through the C ABI and under one option set, with the family name asserted each time:

  dense run     private dense operands between zero guards: the form the rest of the suite validates.  Its output is held to
                the gate of tests/test_gpu_bf16.py (``_close_bf16`` against the oracle's conv_block in that dtype's emulation,
                max-pool / upsample / add / copy exact); float32 to the tolerances of test_mini_every_block_fp32.
  strided run   every operand a channel slice of a wider pixel stride, NaN around every input-side operand, a byte pattern
                around the output, NaN in the output slice: the slice equals the dense run's bit for bit and holds no NaN,
                and not one byte outside the output slice changed -- margins, guards, and every input-side operand.
  aliasing      the in-place add (d_out == d_in) and the fused blocks whose shortcut operand is the group's input run in that
                strided layout too.

The table holds every kernel the shipped cfgs' plans reach (tests/golden/kernel_choice.json) and the conv code only a user's own
cfg reaches: the direct fallback ``conv_direct_*`` in each of its input forms (activations, float NCHW, uint8 frames; odd
channel counts, 7x7, one input channel, float32 store from 16-bit storage), and on all three implicit-GEMM versions the
per-chunk (KMODE 1) and several-taps (KMODE 2) K-tilings, 5x5 and even kernels and a 3x3 without padding.
``test_implicit_gemm_versions_sum_in_one_k_order`` holds the versions to one another bit for bit on those K-tilings.

Below the family name the library is compiled by instance: every run here is taken with the library's launch log, and the set
of code-object symbols it launched must equal the record of tests/golden/kernel_instances.json for that case
(tests/kernel_census.py, which keeps the launch log and ``assert_census``; tools/make_kernel_instances.py writes the record,
tests/test_code_object.py proves that it leaves no compiled kernel out).

Guards lie inside the allocation: a stray access is recorded, never a fault.  The reference has no counterpart of these
layouts (the reference's yolov3/darknet.py:366-399 allocates a tensor per block).  Need an MI355X: -m gpu."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import footprint_util as fu
import kernel_census as census

pytestmark = pytest.mark.gpu

EMULATE = {"bf16": "bf16", "fp16": "f16"}
# tests/test_gpu_parity.py::test_mini_every_block_fp32: np.testing.assert_allclose(got, want, rtol=1e-4, atol=2e-5)
FP32_RTOL, FP32_ATOL = 1e-4, 2e-5


# ------------------------------------------------------------------------------------------------ data

def _conv_specs(case):
    """[(operand prefix, cin, cout, rows of the weight matrix that hold filters, k, stride, leaky)] of the case's convs"""
    g = case["group"]
    if g == "conv":
        return [("", case["cin"], case["cout"], case["k"], case["s"], case.get("leaky", True))]
    if g == "stem_pair":
        return [("op0 ", 3, 32, 3, 1, True), ("op1 ", 32, 64, 3, 2, True)]
    if g == "resblock":
        return [("op0 ", 64, 32, 1, 1, True), ("op1 ", 32, 64, 3, 1, True)]
    if g == "block":
        return [("op0 ", case["cin"], 128, 1, 1, True), ("op1 ", 128, case["cout"], 3, 1, True)]
    if g == "head":
        return [("op0 ", case["cin"], 255, 1, 1, False)]
    return []


def _make_data(case, dtype, lay, paths, plant=None):
    """{operand name: [storage tensor per slice]} for the input-side operands of ``lay`` and, for the oracle, the float32
    values: {"x": NCHW input, "res": NCHW, "convs": [params dict per conv]}.  Seeded per case: every run holds the same.

    ``plant`` (tests/exact_sums.py ``plant``; conv groups only): its values instead of the seeded random ones -- input,
    shortcut, and per conv the weights and the folded scale and bias as they are.  Every value must survive the storage
    type unchanged.  The oracle parameters of such a run hold scale and bias, no batch norm."""
    from yolov3 import _hip as H

    def planted(a, dt):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(torch.float32)
        assert torch.equal(t.to(dt).float(), t), "a planted value is no %s" % dt
        return t.to(dt)
    gen = torch.Generator().manual_seed(sum(map(ord, case["id"])) * 7 + 1)
    tdt = fu.TORCH_DT[dtype]
    B, h, w = case["B"], case["h"], case["w"]
    data, ref = {}, {"convs": []}
    for o in lay.operands:
        if o.side not in ("in", "inout"):
            continue
        if o.name in ("input", "input/output", "residual"):
            c = o.slices[0][1]
            if o.fmt == "u8" and plant is not None:
                import exact_sums as XS
                t = torch.from_numpy(XS.frames_of(plant))
                ref["frames"] = t.numpy()
                data[o.name] = [t.reshape(1, -1)]
            elif plant is not None:
                key = "res" if o.name == "residual" else "x"
                if key == "x" and case["group"] == "conv" and case["inp"] == "nchw":
                    t = planted(plant["x"].transpose(0, 3, 1, 2), tdt).float()
                    ref["x"] = t
                    data[o.name] = [t.reshape(1, -1)]
                else:
                    t = planted(plant[key].reshape(o.pixels, c), tdt if o.fmt != "float32" else torch.float32)
                    ref[key] = t.float().reshape(B, -1, c)
                    data[o.name] = [t]
            elif o.fmt == "u8":
                t = torch.randint(0, 256, (B, h, w, case.get("cin", 3)), generator=gen, dtype=torch.uint8)
                ref["frames"] = t.numpy()
                data[o.name] = [t.reshape(1, -1)]
            elif case["group"] == "conv" and case["inp"] == "nchw":
                t = torch.rand((B, case["cin"], h, w), generator=gen).to(tdt).float()      # (storage-exact values, held as float32)
                ref["x"] = t
                data[o.name] = [t.reshape(1, -1)]
            else:
                scale = 4.0 if case["group"] in ("yolo",) else 1.0
                t = ((torch.rand((o.pixels, c), generator=gen) - 0.5) * scale).to(tdt if o.fmt != "float32" else torch.float32)
                key = "res" if o.name == "residual" else "x"
                ref[key] = t.float().reshape(B, -1, c)
                data[o.name] = [t]
        elif o.name == "zero page" or o.name.endswith("fragment weights"):
            data[o.name] = [torch.zeros(o.slices[0][1], dtype=tdt)]
    for n, ((prefix, cin, cout, k, s, leaky), path) in enumerate(zip(_conv_specs(case), paths)):
        kk = k * k * cin
        if plant is not None:
            wt = planted(plant["convs"][n]["w"], tdt).float()
            assert tuple(wt.shape) == (cout, cin, k, k)
        else:
            wt = ((torch.rand((cout, cin, k, k), generator=gen) - 0.5) * (6.0 / kk) ** 0.5).to(tdt).float()
        ow = lay[prefix + "weight"]
        if path == H.PATH_STEM_MFMA:
            host = torch.zeros((32, 32))
            host[:cout, :27] = wt.flip(1).permute(0, 2, 3, 1).reshape(cout, 27)
            wdev = host.to(tdt)
            cp = 32
        elif path == H.PATH_STEM:
            cp = fu.round_up(cout, 8)
            host = torch.zeros((kk, cp))
            host[:, :cout] = wt.permute(2, 3, 1, 0).reshape(kk, cout)
            wdev = host
        else:
            cp = lay[prefix + "scale"].slices[0][1]
            k_ld = ow.slices[0][1] // cp
            host = torch.zeros((cp, k_ld))
            host[:cout, :kk] = wt.permute(0, 2, 3, 1).reshape(cout, kk)
            wdev = host.to(tdt)
        data[prefix + "weight"] = [wdev.reshape(1, -1)]
        gamma = torch.rand(cout, generator=gen) + 0.5
        beta = torch.rand(cout, generator=gen) - 0.5
        sc, bi = torch.zeros(cp), torch.zeros(cp)
        if plant is not None:
            sc[:cout], bi[:cout] = torch.from_numpy(plant["convs"][n]["scale"]), torch.from_numpy(plant["convs"][n]["bias"])
            p = {"weight": wt.numpy(), "scale": plant["convs"][n]["scale"], "bias": plant["convs"][n]["bias"]}
        elif case["group"] == "head" or not leaky and case.get("out_f32"):
            sc[:cout], bi[:cout] = 1.0, beta                      # a head conv: bias, no batch norm
            p = {"weight": wt.numpy(), "bias": beta.numpy()}
        else:
            from oracle import darknet_oracle as orc
            var = np.ones(cout, dtype=np.float32)
            sc[:cout] = torch.from_numpy((gamma.numpy() / np.sqrt(var + orc.BN_EPS)).astype(np.float32))   # Darknet._fold_bn
            bi[:cout] = beta
            p = {"weight": wt.numpy(), "bn_gamma": gamma.numpy(), "bn_beta": beta.numpy(),
                 "bn_mean": np.zeros(cout, dtype=np.float32), "bn_var": var}
        data[prefix + "scale"], data[prefix + "bias"] = [sc.reshape(1, -1)], [bi.reshape(1, -1)]
        ref["convs"].append(dict(p=p, k=k, s=s, leaky=leaky, pad=case.get("pad", fu.conv_pad(k))))
    ref["path"] = paths[0]
    return data, ref


# ------------------------------------------------------------------------------------------------ one run

def _run(case, dtype, mode, u8_guard=0, opt_name=None, plant=None, logged=census.logged):
    """(output tensors, footprint message or None, kernel names, float32 reference values, layout).  ``plant``: planted operands
    for ``_make_data``; such a run also returns the scratch operands as it finds them (the float32 logits of an unfused head).
    ``logged``: what runs the plan, once it is created, in place of ``census.logged``"""
    from yolov3 import _hip as H
    lib = H.lib()
    dev = torch.device("cuda:0")
    opt = H.options(**fu._opts()[opt_name or case["opt"]])
    _, lay0, _, _ = fu.build(case, dtype, mode, opt)
    raw = torch.empty(lay0.total + fu.ALIGN, dtype=torch.uint8, device=dev)
    shift = -raw.data_ptr() % fu.ALIGN
    alloc = raw[shift:shift + lay0.total]                    # (bodies start on 4 KiB boundaries)
    base = alloc.data_ptr()
    assert base % fu.ALIGN == 0
    ops, lay, frag, path = fu.build(case, dtype, mode, opt, base)
    assert lay.total == lay0.total
    paths = [path, H.PATH_IGEMM]
    data, ref = _make_data(case, dtype, lay, paths, plant)
    fu.fill(alloc, lay, data, poisoned=mode != "dense", u8_guard=u8_guard)
    torch.cuda.synchronize()
    # fragment-order weight copies: made by the library into their operand, which is all that call may write
    for i, name in frag.items():
        before = alloc.clone()
        with H.launch_log() as flog:
            H.check(lib.y3_conv_make_fragment_weights(ctypes.byref(ops[i]), ctypes.c_void_p(ops[i].d_weight_frag), None))
        torch.cuda.synchronize()
        census.FRAGMENT_LAUNCHED.append(flog.symbols)
        lay[name].side = "scratch"
        msg = fu.footprint_violations(before, alloc, lay)
        lay[name].side = "in"
        assert msg is None, "y3_conv_make_fragment_weights: " + msg
    handle = ctypes.c_void_p()
    H.check(lib.y3_plan_create_ex(ops, len(ops), lay["zero page"].ptr(base), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        names = [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))]
        before = alloc.clone()
        d_input = lay["input"].ptr(base) if lay.has("input") else None
        logged(lambda: H.check(lib.y3_plan_run(handle, d_input, None)))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    msg = fu.footprint_violations(before, alloc, lay)
    outs = {}
    for o in lay.operands:
        if o.side in ("out", "inout") or (plant is not None and o.side == "scratch"):
            for k in range(len(o.slices)):
                outs["%s/%d" % (o.name, k)] = fu.read_slice(alloc, o, k, torch.uint8).cpu()
    return outs, msg, names, ref, lay


def _typed(outs, key, fmt):
    dt = {"float32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16, "i64": torch.int64}[fmt]
    t = outs[key]
    return t.contiguous().view(dt).reshape(t.shape[0], -1)


# ------------------------------------------------------------------------------------------------ the existing gates

def _gate(got, want_unrounded, dtype, what, slack=None):
    """``got`` against the oracle's float32 result: the 16-bit modes under tests/test_gpu_bf16.py's own comparison, float32
    under test_mini_every_block_fp32's tolerances"""
    if dtype == "float32":
        np.testing.assert_allclose(got.float().numpy(), want_unrounded.numpy(), rtol=FP32_RTOL, atol=FP32_ATOL, err_msg=what)
        return
    import test_gpu_bf16 as G
    G._close_bf16(got.float(), G.MODES[dtype]["rnd"](want_unrounded), what, slack, dtype)


def _nchw(t, B, h, w):
    return t.float().reshape(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


def _check_dense_against_oracle(case, dtype, outs, ref, lay):
    from oracle import darknet_oracle as orc
    from yolov3 import _hip as H
    g = case["group"]
    B, h, w = case["B"], case["h"], case["w"]
    emulate = EMULATE.get(dtype)
    acc = "f64" if dtype == "float32" else "f32"

    def conv(x, cv):
        return orc.conv_block(x, cv["p"], cv["s"], cv["pad"], cv["leaky"], round_weights=emulate, accumulate=acc)

    def x_of():
        if "frames" in ref:
            x = torch.from_numpy(orc.frames_to_input(list(ref["frames"])))
            # the MFMA stem stores byte / 255 in the storage type before it multiplies; the VALU stem and conv_direct read the
            # bytes themselves and multiply byte / 255 in float32 by the (storage-type) weights: no rounding of the input
            return orc.storage_round(emulate)(x) if emulate and ref["path"] == H.PATH_STEM_MFMA else x
        return ref["x"] if ref["x"].dim() == 4 else _nchw(ref["x"], B, h, w)

    if g in ("conv", "stem_pair", "resblock", "block"):
        o = lay["output"]
        cvs = ref["convs"]
        x = x_of()
        slack = None
        if len(cvs) == 2:
            import test_gpu_bf16 as G
            mid = conv(x, cvs[0])
            p2 = cvs[1]["p"]
            alpha2 = torch.from_numpy(p2["bn_gamma"] / np.sqrt(p2["bn_var"] + orc.BN_EPS))
            rnd = G.MODES[dtype]["rnd"]
            slack = G._flip_slack(mid, rnd(torch.from_numpy(p2["weight"])), alpha2, cvs[1]["s"], 1, dtype)
            y = conv(rnd(mid), cvs[1])
            res = x if (g == "resblock" or case.get("res")) else None
        else:
            y = conv(x, cvs[0])
            res = _nchw(ref["res"], B, y.shape[2], y.shape[3]) if case["res"] else None
        if res is not None:
            y = y + res                                        # one rounding of the sum (conv + shortcut in one epilogue)
        got = _nchw(_typed(outs, "output/0", o.fmt), B, y.shape[2], y.shape[3])
        if o.fmt == "float32" and dtype != "float32":
            # float32 logits of a 16-bit head conv: exact products, float32 accumulation -- the float32 gate
            np.testing.assert_allclose(got.numpy(), y.numpy(), rtol=FP32_RTOL, atol=FP32_ATOL, err_msg=case["id"])
        else:
            _gate(got, y, dtype, "%s %s" % (case["id"], dtype), slack)
        return
    if g == "layer":
        kind = case["kind"]
        x = _nchw(ref["x"], B, h, w)
        if kind == "maxpool":
            if case["dk"]:
                import darknet_pool_restate as DP
                want = DP.pool(x, case["k"], case["s"])
            else:
                want = orc.maxpool(x, case["k"], case["s"])
        elif kind == "upsample":
            want = orc.upsample(x, case["s"])
        elif kind == "add":
            want = (x + _nchw(ref["res"], B, h, w)).to(fu.TORCH_DT[dtype]).float()
        else:
            want = x
        key = "input/output/0" if case["alias"] else "output/0"
        got = _nchw(_typed(outs, key, dtype), B, want.shape[2], want.shape[3])
        assert torch.equal(got, want), "%s: %d values differ from the oracle" % (case["id"], int((got != want).sum()))
        return
    if g == "reorg":
        import yolov2_restate as R2
        x = _nchw(ref["x"], B, h, w)
        want = torch.from_numpy(R2.reorg(x.numpy(), case["s"], case["form3d"]))
        got = _nchw(_typed(outs, "output/0", dtype), B, want.shape[2], want.shape[3])
        assert torch.equal(got, want), "%s: %d values differ from Darknet's loop" % (case["id"], int((got != want).sum()))
        return
    if g == "spp":
        x = _nchw(ref["x"], B, h, w)
        for i, k in enumerate((5, 9, 13)):
            if case["dk"]:
                import darknet_pool_restate as DP
                want = DP.pool(x, k, 1)
            else:
                want = orc.maxpool(x, k, 1)
            got = _nchw(_typed(outs, "concat/%d" % i, dtype), B, h, w)
            assert torch.equal(got, want), "%s pool %d" % (case["id"], k)
        return
    if g == "head":
        # the gate the suite holds the fused head kernels to (tests/test_gpu_parity.py): the two separate kernels, bit for bit
        held = list(census.LAUNCHED)
        plain, msg, names, _, _ = _run(case, dtype, "dense", opt_name="head_unfused")
        census.LAUNCHED[:] = held                                    # (the two separate kernels are not this case's launch set)
        assert msg is None, msg
        assert names[0].startswith("conv_igemm_") and names[1] == "yolo_decode_f32", names
        for key in ("bbox/0", "prob/0", "cls/0"):
            assert torch.equal(outs[key], plain[key]), "%s: fused head differs from conv + decode in %s" % (case["id"], key)
        return
    if g == "yolo":
        x = _nchw(ref["x"], B, h, w)
        box, prob, idx = orc.yolo_decode(x, [(30.0 + 40 * a, 60.0 + 25 * a) for a in range(case["n_anchor"])])
        box = box.clone()
        box[..., 2] /= 416.0                                  # Darknet.forward divides w, h by the network size (the op's net_w, net_h)
        box[..., 3] /= 352.0
        # the comparison of tests/test_gpu_parity.py::test_yolo_decode_op_any_class_count, tolerances included
        np.testing.assert_allclose(_typed(outs, "bbox/0", "float32").reshape(B, -1, 4).numpy(), box.numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(_typed(outs, "prob/0", "float32").reshape(B, -1).numpy(), prob.numpy(), rtol=1e-5, atol=1e-8)
        got, want = _typed(outs, "cls/0", "i64").reshape(B, -1).numpy(), idx.numpy()
        differ = got != want
        if differ.any():                                      # only where the top two class logits are within float rounding
            na, ncls = case["n_anchor"], case["ncls"]
            t = x.numpy().reshape(B, na, ncls + 5, h, w)[:, :, 5:].transpose(0, 1, 3, 4, 2).reshape(B, -1, ncls)
            top2 = np.sort(t[differ], axis=-1)[:, -2:]
            assert np.all(top2[:, 1] - top2[:, 0] < 1e-5), "arg-max differs beyond a rounding tie"
        return
    raise AssertionError(g)


# ------------------------------------------------------------------------------------------------ the test

def _no_nan(outs, lay):
    for o in lay.operands:
        if o.side in ("out", "inout") and o.fmt in fu.NAN_BYTES:
            for k in range(len(o.slices)):
                t = _typed(outs, "%s/%d" % (o.name, k), o.fmt)
                assert not bool(torch.isnan(t.float()).any()), "%s slice %d holds NaN: %d elements never written or poisoned" % (
                    o.name, k, int(torch.isnan(t.float()).sum()))


@pytest.mark.parametrize("cid", ["%s-%s" % p for p in fu.case_ids()])
def test_kernel_touches_exactly_its_operands(cid):
    from yolov3 import _hip
    _hip.require_gpu()
    cname, dtype = cid.rsplit("-", 1)
    case = fu.case_by_id(cname)
    want = fu.family_name(case, dtype)
    del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
    dense, msg, names, ref, lay = _run(case, dtype, "dense")
    assert names[0] == want, (names, want)
    assert msg is None, "dense run: " + msg
    _no_nan(dense, lay)
    _check_dense_against_oracle(case, dtype, dense, ref, lay)

    u8 = any(o.fmt == "u8" and o.side == "in" for o in lay.operands)
    for guard in ((0x00, 0xFF) if u8 else (0,)):
        strided, msg, names, _, slay = _run(case, dtype, "strided", u8_guard=guard)
        assert names[0] == want, (names, want)
        assert msg is None, "strided run (uint8 guards 0x%02X): %s" % (guard, msg)
        _no_nan(strided, slay)
        assert strided.keys() == dense.keys()
        for key in dense:
            assert torch.equal(strided[key], dense[key]), "%s: %d bytes of the strided, poisoned run differ from the dense run" % (
                key, int((strided[key] != dense[key]).sum()))
    # the dense run and every strided run launched exactly the compiled instance(s) recorded for this case
    assert len(census.LAUNCHED) == (3 if u8 else 2)
    census.assert_census(cid)
    if census.FRAGMENT_LAUNCHED:
        census.LAUNCHED[:] = census.FRAGMENT_LAUNCHED
        census.assert_census(census.FRAGMENT_KEY)


# ------------------------------------------------------------------------------------------------ one K order
# csrc/api.hip choose_conv: "Which kernel runs changes speed only: every MFMA conv kernel sums in the same K order".
# tests/test_gpu_parity.py::test_kernel_choice_does_not_change_a_bit holds that on the shipped shapes, all of them one tap per
# K-tile; here the per-chunk (KMODE 1) and several-taps (KMODE 2) K-tilings of the three implicit-GEMM versions, each shape run
# dense under several option sets on the SAME data (the case of the table that gives the shape seeds it).

K_ORDER_FAMILY = {"igemm1": "conv_igemm_%s_128x{bn}", "igemm2_noshrink": "conv_igemm2_%s_128x{bn}", "igemm3": "conv_igemm3_%s_128x128",
                  "igemm2_96": "conv_igemm2_%s_96x64", "igemm3_64": "conv_igemm3_%s_64x128"}
# (case of the table that gives shape and data, option sets; igemm3_64 has 16-bit tiles only)
K_ORDER_SHAPES = [("igemm1_k3s2_c40", ("igemm1", "igemm2_noshrink", "igemm3", "igemm2_96", "igemm3_64")),
                  ("igemm1_1x1_c72", ("igemm1", "igemm2_noshrink", "igemm3", "igemm2_96", "igemm3_64")),
                  ("igemm3_128_k5_c16_res", ("igemm3", "igemm2_96", "igemm3_64")),
                  ("igemm1_k3_c24_res", ("igemm1", "igemm2_noshrink"))]


@pytest.mark.parametrize("dtype", fu.ALL)
@pytest.mark.parametrize("cid,opts", K_ORDER_SHAPES, ids=["k3s2_c40", "1x1_c72", "k5_c16_res", "k3_c24_res"])
def test_implicit_gemm_versions_sum_in_one_k_order(cid, opts, dtype):
    from yolov3 import _hip
    _hip.require_gpu()
    base = fu.case_by_id(cid)
    first = None
    del census.LAUNCHED[:]
    for opt in opts:
        if opt == "igemm3_64" and dtype == "float32":
            continue
        family = K_ORDER_FAMILY[opt].format(bn=128 if base["cout"] > 64 else 64)
        outs, msg, names, _, _ = _run(dict(base, opt=opt, family=family), dtype, "dense")
        assert names[0] == family % fu.TAG[dtype], (opt, names)
        assert msg is None, "%s: %s" % (opt, msg)
        if first is None:
            first = (opt, names[0], outs)
            continue
        differ = int((outs["output/0"] != first[2]["output/0"]).sum())
        assert differ == 0, "%s %s: %d bytes of %s (%s) differ from %s (%s)" % (
            cid, dtype, differ, names[0], opt, first[1], first[0])


# ------------------------------------------------------------------------------------------------ the other entry points
# Every buffer of a call is a flat ``[guard | exact-size body | guard]`` of one allocation, sized exactly as include/yolov3_hip.h
# says (workspaces: exactly the ``*_workspace_bytes`` query).  The call runs three times: unguarded, on separate exact-size
# tensors (workspace 0xFF); between zero guards (workspace zero); and with NaN / 0xFF round its inputs, the byte pattern round
# its outputs and its workspace, and 0xFF IN the workspace.  Nothing outside the output bodies and the workspace may change, and
# the outputs of all three must be equal byte for byte -- so no entry point relies on what a workspace holds when it gets it.

def _guarded(bufs, call, poisoned):
    """``bufs``: [(name, side, fmt, elements, host tensor or None)]; ``call(ptr)`` gets {name: device address}"""
    dev = torch.device("cuda:0")
    ops = [fu.flat(name, side, fmt, n) for name, side, fmt, n, _ in bufs]
    lay = fu.Layout(ops)
    raw = torch.empty(lay.total + fu.ALIGN, dtype=torch.uint8, device=dev)
    shift = -raw.data_ptr() % fu.ALIGN
    alloc = raw[shift:shift + lay.total]
    base = alloc.data_ptr()
    data = {name: [t.reshape(1, -1)] for name, side, _, _, t in bufs if side == "in"}
    fu.fill(alloc, lay, data, poisoned=poisoned, u8_guard=0xFF if poisoned else 0)
    torch.cuda.synchronize()
    before = alloc.clone()
    census.logged(lambda: call({o.name: o.ptr(base) for o in ops}))
    torch.cuda.synchronize()
    msg = fu.footprint_violations(before, alloc, lay)
    assert msg is None, ("poisoned guards: " if poisoned else "zero guards: ") + msg
    return {o.name: fu.read_slice(alloc, o, 0, torch.uint8).cpu() for o in ops if o.side == "out"}


def _unguarded(bufs, call):
    """the same call on separate exact-size tensors, outputs pre-filled as ``fu.fill`` pre-fills them"""
    dev = torch.device("cuda:0")
    t = {}
    for name, side, fmt, n, host in bufs:
        es = fu.flat(name, side, fmt, n).es
        if side == "in":
            t[name] = host.contiguous().reshape(-1).view(torch.uint8).to(dev)
        elif side == "out" and fmt in fu.NAN_BYTES:
            t[name] = torch.tensor(fu.NAN_BYTES[fmt], dtype=torch.uint8).repeat(n).to(dev)
        else:
            t[name] = torch.full((n * es,), 0x7F if side == "out" else 0xFF, dtype=torch.uint8, device=dev)
        assert t[name].numel() == n * es and t[name].data_ptr() % 16 == 0, name
    torch.cuda.synchronize()
    census.logged(lambda: call({name: v.data_ptr() for name, v in t.items()}))
    torch.cuda.synchronize()
    return {name: t[name].reshape(1, -1).cpu() for name, side, _, _, _ in bufs if side == "out"}


def _both(bufs, call, key):
    """outputs of the unguarded call, after the two guarded calls have been held to it byte for byte and all three to the
    launch set recorded as ``key``"""
    del census.LAUNCHED[:]
    free = _unguarded(bufs, call)
    for what, poisoned in (("zero guards", False), ("poisoned guards", True)):
        got = _guarded(bufs, call, poisoned)
        for k in free:
            assert torch.equal(free[k], got[k]), "%s: %d bytes differ between the unguarded call and the call between %s" % (
                k, int((free[k] != got[k]).sum()), what)
    assert len(census.LAUNCHED) == 3
    census.assert_census(key)
    return free


def _detect_inputs():
    """4 frames x 5000 rows: frame 0 has no candidate, frame 1 a handful, frames 2 and 3 ~4500 each (more than the 4096 the
    kernel sorts in LDS: the global-memory sort)"""
    import darknet_nms_restate as R
    box, prob, cls = R.detector_inputs(batch=4, rows=5000, seed=77)
    prob[0] = 0.0
    prob[1, 12:] *= 0.05
    hw = np.asarray([(1080, 1920), (427, 640), (333, 1000), (608, 608)], np.int32)
    return box, prob, cls, hw


def _detect_bufs(ws_bytes, box, prob, cls, hw):
    b, rows = prob.shape
    T = torch.from_numpy
    return [("bbox", "in", "float32", b * rows * 4, T(box)), ("prob", "in", "float32", b * rows, T(prob)),
            ("cls", "in", "i64", b * rows, T(cls)), ("orig_hw", "in", "i32", b * 2, T(hw)),
            ("workspace", "scratch", "u8", ws_bytes, None),
            ("det_count", "out", "i32", b, None), ("det_tlbr", "out", "i64", b * rows * 4, None),
            ("det_prob", "out", "float32", b * rows, None), ("det_cls", "out", "i64", b * rows, None),
            ("det_row", "out", "i32", b * rows, None)]


DETECTORS = ["detect", "letterbox", "darknet_iou", "darknet_greedynms", "darknet_diounms"]


def _detect_call(which, b, rows, ws_bytes, thresh=0.1):
    from yolov3 import _hip as H
    lib = H.lib()

    def call(p):
        args = (p["bbox"], p["prob"], p["cls"], b, rows, p["orig_hw"], ctypes.c_float(thresh), 0.3, p["workspace"], ws_bytes,
                p["det_count"], p["det_tlbr"], p["det_prob"], p["det_cls"], p["det_row"])
        if which == "detect":
            H.check(lib.y3_detect(*args, None))
        elif which == "letterbox":
            H.check(lib.y3_detect_letterbox(*args, 608, 608, None))
        else:
            kind = H.NMS_KINDS[which.split("_")[1]]
            H.check(lib.y3_detect_darknet(*args, 608, 608, kind, ctypes.c_float(0.6), None))
    return call


@pytest.mark.parametrize("which", DETECTORS)
def test_detectors_stay_inside_exact_size_workspace_and_outputs(which):
    from yolov3 import _hip as H
    H.require_gpu()
    lib = H.lib()
    box, prob, cls, hw = _detect_inputs()
    b, rows = prob.shape
    ws = int((lib.y3_detect_darknet_workspace_bytes if which.startswith("darknet") else lib.y3_detect_workspace_bytes)(b, rows))
    outs = _both(_detect_bufs(ws, box, prob, cls, hw), _detect_call(which, b, rows, ws), "detect-" + which)
    count = outs["det_count"].view(torch.int32).flatten().tolist()
    assert count[0] == 0 and 0 < count[1] <= 12 and count[2] > 0 and count[3] > 0, count
    assert int((prob[2] >= np.float32(0.1)).sum()) > 4096


NMS = ["int64", "float32", "float64", "darknet_iou", "darknet_greedynms", "darknet_diounms"]


NMS_SIZES = [1, 300, 5000]


@pytest.mark.parametrize("n", NMS_SIZES)
@pytest.mark.parametrize("which", NMS)
def test_nms_entry_points_stay_inside_exact_size_workspace_and_outputs(which, n):
    import darknet_nms_restate as R
    from yolov3 import _hip as H
    H.require_gpu()
    lib = H.lib()
    # (inputs of the committed restatement cases: tests/darknet_nms_restate.py CASES / BIG_CASES)
    xywh, prob, cls = R.clusters(*{1: (5, 1, 1), 300: (0, 300, 1), 5000: (101, 5000, 3)}[n])
    T = torch.from_numpy
    tl = xywh[:, :2] - xywh[:, 2:] / 2
    tlbr = np.concatenate([tl, tl + xywh[:, 2:]], 1) * 608.0
    if which.startswith("darknet"):
        ws = int(lib.y3_nms_darknet_workspace_bytes(n))
        boxes = ("xywh", "in", "float32", n * 4, T(xywh))
        pr = ("prob", "in", "float32", n, T(prob))
    elif which == "int64":
        ws = int(lib.y3_nms_workspace_bytes(n))
        boxes = ("tlbr", "in", "i64", n * 4, T(tlbr.astype(np.int64)))
        pr = ("prob", "in", "float32", n, T(prob))
    else:
        ws = int(lib.y3_nms_float_workspace_bytes(n))
        f64 = which == "float64"
        boxes = ("tlbr", "in", "f64" if f64 else "float32", n * 4, T(tlbr.astype(np.float64 if f64 else np.float32)))
        pr = ("prob", "in", "f64", n, T(prob.astype(np.float64)))
    bufs = [boxes, pr, ("cls", "in", "i64", n, T(cls)), ("workspace", "scratch", "u8", ws, None),
            ("keep", "out", "i64", n, None), ("keep_count", "out", "i32", 1, None)]

    def call(p):
        if which.startswith("darknet"):
            H.check(lib.y3_nms_darknet(p["xywh"], p["prob"], p["cls"], n, ctypes.c_float(0.45), H.NMS_KINDS[which.split("_")[1]],
                                       ctypes.c_float(0.6), p["workspace"], ws, p["keep"], p["keep_count"], None))
        elif which == "int64":
            H.check(lib.y3_nms(p["tlbr"], p["prob"], p["cls"], n, 0.3, p["workspace"], ws, p["keep"], p["keep_count"], None))
        else:
            H.check(lib.y3_nms_float(p["tlbr"], H.Y3_F64 if which == "float64" else H.Y3_F32, p["prob"], p["cls"], n, 0.3,
                                     p["workspace"], ws, p["keep"], p["keep_count"], None))
    outs = _both(bufs, call, "nms-%s-%d" % (which, n))
    kept = int(outs["keep_count"].view(torch.int32)[0])
    assert 1 <= kept <= n
    if which.startswith("darknet"):         # the values: Darknet's rule as tests/darknet_nms_restate.py states it
        want = R.keep_fast(xywh, prob, cls, R.THRESH, which.split("_")[1], R.BETA)
        assert outs["keep"].view(torch.int64).flatten()[:kept].tolist() == [int(i) for i in want]
    else:                                   # the reference's rule (inference.py:161-266) as the oracle states it
        from oracle import darknet_oracle as orc
        boxes = tlbr.astype({"int64": np.int64, "float32": np.float32, "float64": np.float64}[which])
        want = orc.non_max_suppression(boxes, prob, class_idx=cls, iou_thresh=0.3)
        assert sorted(outs["keep"].view(torch.int64).flatten()[:kept].tolist()) == sorted(int(i) for i in want)


def test_pack_records_stays_inside_exact_size_buffers():
    """records of kmax = 7 per frame: frame 0 has no detection, frames 2 and 3 far more than kmax"""
    from yolov3 import _hip as H
    H.require_gpu()
    lib = H.lib()
    box, prob, cls, hw = _detect_inputs()
    b, rows = prob.shape
    ws = int(lib.y3_detect_workspace_bytes(b, rows))
    det = _both(_detect_bufs(ws, box, prob, cls, hw), _detect_call("detect", b, rows, ws), "detect-detect")
    kmax = 7
    V = lambda k, dt: det[k].contiguous().view(dt).flatten()
    bufs = [("det_count", "in", "i32", b, V("det_count", torch.int32)), ("det_tlbr", "in", "i64", b * rows * 4, V("det_tlbr", torch.int64)),
            ("det_prob", "in", "float32", b * rows, V("det_prob", torch.float32)), ("det_cls", "in", "i64", b * rows, V("det_cls", torch.int64)),
            ("det_row", "in", "i32", b * rows, V("det_row", torch.int32)),
            ("records", "out", "i32", b * kmax * 8, None), ("rec_count", "out", "i32", b, None)]

    def call(p):
        H.check(lib.y3_pack_records(p["det_count"], p["det_tlbr"], p["det_prob"], p["det_cls"], p["det_row"], b, rows, kmax,
                                    p["records"], p["rec_count"], None))
    outs = _both(bufs, call, "y3_pack_records")
    rc = outs["rec_count"].view(torch.int32).flatten().tolist()
    assert rc == V("det_count", torch.int32).tolist() and rc[0] == 0 and rc[2] > kmax


RESIZES = [((37, 53), (29, 41)), ((21, 35), (45, 77)), ((3, 5), (7, 11))]


@pytest.mark.parametrize("src,dst", RESIZES)
def test_resize_stays_inside_exact_size_frames(src, dst):
    """odd sizes: 5883 -> 3567, 2205 -> 10395 and 45 -> 231 bytes, none a multiple of 16"""
    from yolov3 import _hip as H
    from yolov3 import preprocess as P
    H.require_gpu()
    lib = H.lib()
    (sh, sw), (dh, dw) = src, dst
    assert (sh * sw * 3) % 16 and (dh * dw * 3) % 16
    frame = np.random.default_rng(sh).integers(0, 256, (sh, sw, 3), dtype=np.uint8)
    T = torch.from_numpy
    bufs = [("src", "in", "u8", sh * sw * 3, T(frame)), ("ytab", "in", "i32", dh * 4, T(P.axis_table(sh, dh, False))),
            ("xtab", "in", "i32", dw * 4, T(P.axis_table(sw, dw, True))), ("dst", "out", "u8", dh * dw * 3, None)]

    def call(p):
        H.check(lib.y3_resize_bilinear_u8(p["src"], sh, sw, p["dst"], dh, dw, p["ytab"], p["xtab"], None))
    outs = _both(bufs, call, "y3_resize_bilinear_u8-%dx%d-%dx%d" % (sh, sw, dh, dw))
    want = P.resize_bilinear_u8(frame, dh, dw)
    assert np.array_equal(outs["dst"].numpy().reshape(dh, dw, 3), want)


def test_letterbox_stays_inside_exact_size_frames():
    """two frames of different odd sizes into a 45 x 51 network: 2 x 6885 bytes out"""
    from yolov3 import _hip as H
    from yolov3 import preprocess as P
    H.require_gpu()
    lib = H.lib()
    net_h, net_w = 45, 51
    shapes = [(37, 53), (61, 23)]
    rng = np.random.default_rng(9)
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    T = torch.from_numpy
    bufs = [("dst", "out", "u8", len(frames) * net_h * net_w * 3, None)]
    geo = []
    for i, f in enumerate(frames):
        nh, nw, _, _ = P.letterbox_geometry(f.shape[0], f.shape[1], net_h, net_w)
        geo.append((nh, nw))
        bufs += [("src%d" % i, "in", "u8", f.size, T(f)), ("ytab%d" % i, "in", "i32", nh * 4, T(P.axis_table(f.shape[0], nh, False))),
                 ("xtab%d" % i, "in", "i32", nw * 4, T(P.axis_table(f.shape[1], nw, True)))]

    def call(p):
        descs = (H.Y3LetterboxFrame * len(frames))()
        for i, f in enumerate(frames):
            descs[i].d_src, descs[i].src_h, descs[i].src_w = p["src%d" % i], f.shape[0], f.shape[1]
            descs[i].d_ytab, descs[i].d_xtab = p["ytab%d" % i], p["xtab%d" % i]
        H.check(lib.y3_letterbox_u8(descs, len(frames), p["dst"], net_h, net_w, 128, None))
    outs = _both(bufs, call, "y3_letterbox_u8")
    got = outs["dst"].numpy().reshape(len(frames), net_h, net_w, 3)
    for i, f in enumerate(frames):
        assert np.array_equal(got[i], P.letterbox_u8(f, net_h, net_w, 128)), i


COPY_SIZES = [1, 15, 100003, 1 << 20]


@pytest.mark.parametrize("nbytes", COPY_SIZES)
def test_copy_bytes_stays_inside_exact_size_buffers(nbytes):
    from yolov3 import _hip as H
    H.require_gpu()
    lib = H.lib()
    src = torch.from_numpy(np.random.default_rng(nbytes).integers(0, 256, nbytes, dtype=np.uint8))
    bufs = [("src", "in", "u8", nbytes, src), ("dst", "out", "u8", nbytes, None)]

    def call(p):
        H.check(lib.y3_copy_bytes(p["src"], p["dst"], nbytes, 8, None))
    outs = _both(bufs, call, "y3_copy_bytes-%d" % nbytes)
    assert torch.equal(outs["dst"].flatten(), src)


CXYWH = ["int64", "float32", "float64"]


@pytest.mark.parametrize("which", CXYWH)
def test_cxywh_to_tlbr_stays_inside_exact_size_rows(which):
    """y3_cxywh_to_tlbr / y3_cxywh_to_tlbr_float (the reference's cxywh_to_tlbr, inference.py:269-283) on 1000 rows of 6 columns,
    more than one block and a partial last one: tl = c - floor(wh / 2), br = c + floor(wh / 2) in the rows' own type, exactly;
    the columns past the fourth are copied as they are"""
    from yolov3 import _hip as H
    H.require_gpu()
    lib = H.lib()
    n, cols = 1000, 6
    rng = np.random.default_rng(11)
    ndt = {"int64": np.int64, "float32": np.float32, "float64": np.float64}[which]
    fmt = {"int64": "i64", "float32": "float32", "float64": "f64"}[which]
    xywh = rng.uniform(-50.0, 700.0, (n, cols))
    xywh[:, 2:4] = rng.uniform(-20.0, 300.0, (n, 2))               # (negative sizes: floor, not truncation)
    xywh = (np.floor(xywh * 4) / 4 if which != "int64" else np.floor(xywh)).astype(ndt)      # (quarters: exact in float32)
    bufs = [("xywh", "in", fmt, n * cols, torch.from_numpy(xywh)), ("tlbr", "out", fmt, n * cols, None)]

    def call(p):
        if which == "int64":
            H.check(lib.y3_cxywh_to_tlbr(p["xywh"], p["tlbr"], n, cols, None))
        else:
            H.check(lib.y3_cxywh_to_tlbr_float(p["xywh"], p["tlbr"], n, cols, H.Y3_F64 if which == "float64" else H.Y3_F32, None))
    outs = _both(bufs, call, "y3_cxywh_to_tlbr-" + which)
    tdt = {"int64": torch.int64, "float32": torch.float32, "float64": torch.float64}[which]
    got = outs["tlbr"].contiguous().view(tdt).reshape(n, cols).numpy()
    half = xywh[:, 2:4] // 2 if which == "int64" else np.floor(xywh[:, 2:4] / ndt(2))
    assert np.array_equal(got[:, 0:2], xywh[:, 0:2] - half) and np.array_equal(got[:, 2:4], xywh[:, 0:2] + half)
    assert np.array_equal(got[:, 4:], xywh[:, 4:])                       # the columns past the fourth are copied
