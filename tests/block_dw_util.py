"""Shared by tests/test_gpu_block_dw.py, tests/test_block_dw_host.py and tools/make_kernel_instances.py: the cases of the
direct-weights fused block kernel (csrc/conv_block_dw.hip, libyolov3_hip_block.so; y3_options.fuse_block = 3 / 4) and a two-op
plan on given operands with the fragment-order copies the kernel reads.  The library's census is the "block" row of
tests/kernel_census.py (tests/golden/kernel_instances_block.json)."""
import ctypes

TAG = {"bf16": "bf16", "fp16": "f16"}
FRAMES = 3

# Maps (w x h), with the rectangles conv_block.hip's choose_tile cuts at three frames: 19 x 19 is one exact rectangle per frame;
# 21 x 13 one rectangle of 273 pixels per frame -- seven of the 24 pixel fragments hang over the rectangle's end, one straddles it,
# and rows of 21 + 2 patch pixels put every fragment across row ends; 38 x 38 four exact 19 x 19 rectangles.  choose_tile gives
# 21 x 13 no rectangle that crosses the FRAME's edges, so a fourth map does that: 25 x 43 is cut 2 x 2 into 13 x 22 rectangles
# that hang over the right and the bottom edge by one pixel each.
MAPS = {"19x19": (19, 19), "21x13": (13, 21), "38x38": (38, 38), "25x43": (43, 25)}          # name -> (h, w)
RECTANGLES = {"19x19": (19, 19, 1, 1), "21x13": (21, 13, 1, 1), "38x38": (19, 19, 2, 2), "25x43": (13, 22, 2, 2)}   # tw, th, tiles x, y
# Channels: Cin 256 with the shortcut and two output passes; Cin 384 (twelve sub-chunks) without; Cin 192 (six) and ONE pass
CHANNELS = {"c256_res": (256, 256, True), "c384": (384, 256, False), "c192_one_pass": (192, 128, False)}
# bf16 everywhere, fp16 on two
CASES = [(m, c, "bf16") for m in MAPS for c in CHANNELS] + [("21x13", "c256_res", "fp16"), ("38x38", "c384", "fp16")]


def case_key(m, c, dtype):
    return "block_dw_%s_%s-%s" % (m, c, dtype)


def make_pair(dev, dtype, x, convs, res):
    """A 1x1 (cin -> 128) + 3x3 (128 -> cout) pair on given operands, with fragment-order copies of both weights.
    x: (B, h, w, cin) float tensor of storage-type values; convs: two dicts of w (cout, cin, k, k), scale, bias (float tensors).
    Returns (tensors to keep alive, the two y3_op structs)."""
    import torch
    from yolov3 import _hip
    lib = _hip.lib()
    c_dtype, tdt = {"bf16": (_hip.Y3_BF16, torch.bfloat16), "fp16": (_hip.Y3_F16, torch.float16)}[dtype]
    B, h, w, cin = x.shape
    t = {"x": x.to(tdt).to(dev).contiguous(), "mid": torch.zeros((B, h, w, 128), dtype=tdt, device=dev),
         "zero": torch.zeros(4096, dtype=torch.uint8, device=dev)}
    ops = (_hip.Y3Op * 2)()
    for n, conv in enumerate(convs):
        co, ci, k, _ = conv["w"].shape
        kk = k * k * ci
        k_ld = (kk + 63) // 64 * 64
        cp = (co + 127) // 128 * 128
        wm = torch.zeros((cp, k_ld), dtype=torch.float32)
        wm[:co, :kk] = conv["w"].permute(0, 2, 3, 1).reshape(co, kk)           # K order (ky, kx, ci)
        sc, bi = torch.zeros(cp), torch.zeros(cp)
        sc[:co], bi[:co] = conv["scale"], conv["bias"]
        t["w%d" % n], t["sc%d" % n], t["bi%d" % n] = wm.to(tdt).to(dev), sc.to(dev), bi.to(dev)
        t["wf%d" % n] = torch.zeros(cp * k_ld, dtype=tdt, device=dev)
        op = ops[n]
        op.kind, op.dtype, op.batch = _hip.OP_CONV, c_dtype, B
        op.ksize, op.stride, op.pad = k, 1, (k - 1) // 2
        op.in_c, op.out_c, op.in_ld, op.out_ld = ci, co, ci, co
        op.in_h = op.out_h = h
        op.in_w = op.out_w = w
        op.cout_pad, op.k_ld = cp, k_ld
        op.d_weight, op.d_scale, op.d_bias = t["w%d" % n].data_ptr(), t["sc%d" % n].data_ptr(), t["bi%d" % n].data_ptr()
        op.flags = _hip.F_LEAKY
        op.block_idx = n
        _hip.check(lib.y3_conv_make_fragment_weights(ctypes.byref(op), ctypes.c_void_p(t["wf%d" % n].data_ptr()), None))
        op.d_weight_frag = t["wf%d" % n].data_ptr()
    torch.cuda.synchronize()
    ops[0].d_in, ops[0].d_out = t["x"].data_ptr(), t["mid"].data_ptr()
    ops[0].flags |= _hip.F_FUSE_NEXT
    ops[1].d_in = t["mid"].data_ptr()
    if res:
        ops[1].d_res, ops[1].res_ld = t["x"].data_ptr(), cin
        ops[1].flags |= _hip.F_RESIDUAL
    return t, ops


def random_pair(dev, dtype, B, h, w, cin, cout, res, seed):
    """make_pair on random operands: also returns them, as float tensors of storage-type values, for an oracle"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    tdt = {"bf16": torch.bfloat16, "fp16": torch.float16}[dtype]
    x = (torch.randn((B, h, w, cin), generator=gen) * 0.7).to(tdt).float()
    convs = []
    for ci, co, k in ((cin, 128, 1), (128, cout, 3)):
        kk = k * k * ci
        convs.append(dict(w=(torch.randn((co, ci, k, k), generator=gen) * (2.0 / kk) ** 0.5).to(tdt).float(),
                          scale=torch.rand(co, generator=gen) + 0.5, bias=torch.rand(co, generator=gen) - 0.5))
    t, ops = make_pair(dev, dtype, x, convs, res)
    return t, ops, x, convs


def make_plan(ops, zero, out, **options):
    from yolov3 import _hip
    ops[1].d_out = out.data_ptr()
    handle = ctypes.c_void_p()
    opt = _hip.options(**options)
    _hip.check(_hip.lib().y3_plan_create_ex(ops, 2, zero.data_ptr(), ctypes.byref(opt), ctypes.byref(handle)))
    return handle
