"""The grouped and depthwise conv kernels restated in their own sum order, float32 operation by operation (numpy only).

csrc/conv_grouped.hip and DESIGN.md section 1 state the arithmetic of ``conv_dwise_*`` and ``conv_grouped_*``; this module does
exactly that, one rounded float32 operation per line, for every output element:

    acc = +0
    for ky, for kx, for c of the group:
        acc = f32(acc + f32(x * w))        # taps outside the image are skipped
    t = f32(f32(acc * scale) + bias)
    v = t                         (linear)
    v = max(t, f32(0.1f * t))     (leaky)
    v = f32(v + r)                (with a shortcut operand)
    store = one rounding of v to the storage type (epilogue_cases.rne_bf16 / rne_f16; float32 stores v)

For linear and leaky ops these are the kernels' bits: tests/test_gpu_grouped.py demands ``torch.equal``.  Mish and logistic run
``__expf`` and ``v_rcp_f32`` on the device, which numpy does not restate bit for bit; here they are float32 numpy functions of
``t`` and the result is held to the toleranced gates only (tests/test_grouped_host.py).

``reverse=True`` visits the taps and the group's channels in the opposite order (ky, kx and c descending): NOT the kernels' order,
used by the host test to show that the equality can tell one order from another.
"""
import numpy as np

import epilogue_cases as E

F32 = np.float32
EXACT_ACTS = ("linear", "leaky")


def out_hw(h, w, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1


def accumulate(x, wt, stride, pad, groups, reverse=False):
    """x (B, cin, h, w), wt (cout, cin / groups, k, k), float32 -> the float32 sums (B, cout, ho, wo) in the stated order"""
    x, wt = np.ascontiguousarray(x, dtype=F32), np.ascontiguousarray(wt, dtype=F32)
    B, cin, h, w = x.shape
    cout, cg_in, k = wt.shape[0], wt.shape[1], wt.shape[2]
    assert cin % groups == 0 and cout % groups == 0 and cg_in == cin // groups and wt.shape[3] == k
    cg_out = cout // groups
    ho, wo = out_hw(h, w, k, stride, pad)
    first = (np.arange(cout) // cg_out) * cg_in                      # the first input channel of each output channel's group
    iy0, ix0 = np.arange(ho) * stride - pad, np.arange(wo) * stride - pad
    acc = np.zeros((B, cout, ho, wo), dtype=F32)
    taps = [(ky, kx, c) for ky in range(k) for kx in range(k) for c in range(cg_in)]
    for ky, kx, c in (reversed(taps) if reverse else taps):
        iy, ix = iy0 + ky, ix0 + kx
        ok = ((iy >= 0) & (iy < h))[:, None] & ((ix >= 0) & (ix < w))[None, :]
        if not ok.any():
            continue
        xs = x[:, first + c][:, :, np.clip(iy, 0, h - 1)][:, :, :, np.clip(ix, 0, w - 1)]
        prod = (xs * wt[:, c, ky, kx].reshape(1, cout, 1, 1)).astype(F32)          # one rounding
        acc = np.where(ok[None, None], (acc + prod).astype(F32), acc)              # one rounding; a tap outside adds nothing
    return acc


def epilogue(acc, scale, bias, act, res=None):
    """the float32 value in front of the store: scale, bias, activation, shortcut operand, each operation rounded"""
    sc, bi = (np.asarray(a, dtype=F32).reshape(1, -1, 1, 1) for a in (scale, bias))
    with np.errstate(all="ignore"):
        t = ((acc * sc).astype(F32) + bi).astype(F32)
        if act == "leaky":
            v = np.maximum(t, (E.SLOPE * t).astype(F32))
        elif act == "mish":
            sp = np.maximum(t, F32(0)) + np.log1p(np.exp(-np.abs(t)))
            v = (t * np.tanh(sp)).astype(F32)
        elif act == "logistic":
            v = (F32(1) / (F32(1) + np.exp(-t))).astype(F32)
        else:
            assert act == "linear", act
            v = t
        if res is not None:
            v = (v + np.asarray(res, dtype=F32)).astype(F32)
    return v.astype(F32)


def stored(x, wt, scale, bias, stride, pad, groups, act, dtype, res=None, reverse=False):
    """the values the op stores, as float32 (B, cout, ho, wo)"""
    return E.RND[dtype](epilogue(accumulate(x, wt, stride, pad, groups, reverse), scale, bias, act, res))


def of_case(case, dtype, data, reverse=False):
    """``stored`` for a case of tests/grouped_cases.py and the data ``grouped_cases.make`` gave for it"""
    res = None if data["res"] is None else np.asarray(data["res"])
    return stored(np.asarray(data["x"]), data["p"]["weight"], data["scale"], data["bias"], case["s"], case["pad"], case["groups"],
                  case.get("act", "leaky"), dtype, res, reverse)
