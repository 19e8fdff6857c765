"""Shared by tests/test_gpu_attention.py and tests/test_attention_host.py: one attention
op (Y3_OP_AVGPOOL / Y3_OP_SCALE_CHANNELS / Y3_OP_SAM, csrc/attention.hip, libyolov3_hip_attn.so) as a one-op plan on operands
laid out by tests/footprint_util.py -- every operand a channel slice of a wider, NaN-poisoned, guarded body inside one allocation,
compared as bytes before and after the run --, the expectations, and the cases of the library's census (the "attn" row of
tests/kernel_census.py, tests/golden/kernel_instances_attn.json)."""
import contextlib
import ctypes

import numpy as np

import attention_ordered as AO
import epilogue_cases as E
import footprint_util as FU

DTYPES = ("float32", "bf16", "fp16")
KINDS = ("avgpool", "scale_channels", "sam")
TAG = FU.TAG
# the identifier of each kind's kernel template inside a code-object symbol, and the BCAST argument that tells the two products apart
TEMPLATE = {"avgpool": "avgpool_kernel", "scale_channels": "attn_mul_kernel", "sam": "attn_mul_kernel"}
T_MANGLED = {"float32": "f", "bf16": "DF16b", "fp16": "DF16_"}


def vec_of(dtype):
    return 16 // FU.ES[dtype]


def census_key(kind, form, dtype):
    return "attn_%s_%s-%s" % (kind, form, dtype)


CENSUS_KEYS = [census_key(k, f, d) for k in KINDS for f in ("vec", "elem") for d in DTYPES]


def symbol_matches(symbol, kind, form, dtype):
    """whether a code-object symbol is the instance (kind, form, dtype): template identifier, element type, VEC and BCAST"""
    vec = vec_of(dtype) if form == "vec" else 1
    args = "I%sLi%dE" % (T_MANGLED[dtype], vec)
    if kind != "avgpool":
        args += "Lb%dE" % (kind == "scale_channels")
    return "%d%s%s" % (len(TEMPLATE[kind]), TEMPLATE[kind], args) in symbol


# ---- expectations (numpy, on float32 arrays of storage-type values) ---------------------------------------------------------

def to_storage(x32, dtype):
    """float32 array -> float32 array of the values after ONE rounding to the storage type"""
    return E.RND[dtype](np.ascontiguousarray(x32, dtype=np.float32))


def product_expected(src, prev, dtype):
    """the exact product rounded once: src (B, H, W, C), prev (B, 1, 1, C) or (B, H, W, C), float32 arrays of storage values"""
    with np.errstate(all="ignore"):
        return E.rnd64(dtype, src.astype(np.float64) * prev.astype(np.float64)).astype(np.float32)


def avgpool_ordered_expected(x, dtype):
    """the ordered float32 sum divided by float32(P), rounded once to storage: x (B, H, W, C) -> (B, 1, 1, C)"""
    b, _, _, c = x.shape
    return to_storage(AO.avgpool(x), dtype).reshape(b, 1, 1, c)


def avgpool_gate(x, dtype):
    """|got - float64 mean| <= this, per output: P * 2^-24 * mean|x| for the float32 sum (every one of the P - 1 additions rounds a
    partial sum of magnitude at most sum|x| by half an ulp, 2^-24 relative), one float32 ulp of the quotient for the division, and
    half a storage ulp of the quotient for the store (2^-8 / 2^-11 / 2^-24 of its magnitude in bf16 / fp16 / float32, or half the
    subnormal spacing).  Derived, not measured."""
    b, h, w, c = x.shape
    p = h * w
    a = np.abs(x.astype(np.float64)).reshape(b, p, c)
    mean_abs = a.mean(axis=1)
    q = np.abs(x.astype(np.float64).reshape(b, p, c).mean(axis=1))
    eps_store = {"float32": 2.0 ** -24, "bf16": 2.0 ** -8, "fp16": 2.0 ** -11}[dtype]
    tiny = {"float32": 2.0 ** -149, "bf16": 2.0 ** -133, "fp16": 2.0 ** -24}[dtype]          # the subnormal spacing
    bound = p * 2.0 ** -24 * mean_abs
    top = (q + bound) * (1.0 + 2.0 ** -23)          # no smaller than the magnitude of the float32 quotient
    return (bound + 2.0 ** -23 * top + eps_store * top + 0.5 * tiny).reshape(b, 1, 1, c)


def same_bits(got, want):
    """element-wise: the same float32 bits, or both NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


# ---- one op on the GPU ------------------------------------------------------------------------------------------------------

KIND_CODE = {"avgpool": 8, "scale_channels": 9, "sam": 10}


def _storage(x32, dtype):
    """float32 numpy (B, H, W, C) of storage values -> torch tensor of the storage type, (pixels, C)"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32))
    return t.to(FU.TORCH_DT[dtype]).reshape(-1, x32.shape[-1])


def run_op(kind, dtype, prev, src=None, form="vec", same_buffer=False, options=None, stream=None, runs=1):
    """One attention op on ``prev`` (and ``src``): float32 numpy arrays (B, H, W, C) holding storage-type values.  Every operand is a
    channel slice of a wider poisoned body between guards (footprint_util); ``form`` "vec" puts slices, strides and bases on the
    16-byte grain, "elem" on odd element offsets (the element form, whatever the channel count); ``same_buffer`` makes ``src``
    and the output two slices of ONE body; ``runs`` > 1 runs the plan again after the allocation was filled afresh (the launch log
    records the first run).  Returns dict(out=(B, Ho, Wo, C) float32, kernel=plan name, symbols=launch log,
    dims=(grid, block, lds)); asserts that nothing outside the output slice changed and that no NaN of the poison got in."""
    import torch
    from yolov3 import _hip
    lib = _hip.lib()
    b, hp, wp, c = prev.shape
    if kind == "avgpool":
        oh = ow = 1
    else:
        assert src is not None and src.shape[0] == b and src.shape[3] == c
        oh, ow = src.shape[1], src.shape[2]
    unit = vec_of(dtype) if form == "vec" else 1
    assert form == "elem" or c % unit == 0
    lds = set()

    def operand(name, side, pixels, v, nslices=1):
        c0, ld = FU.strided_ld(nslices * c + (nslices - 1) * unit, unit, v, avoid=lds)
        lds.add(ld)
        return FU.Operand(name, side, dtype, pixels, ld, [(c0 + k * (c + unit), c) for k in range(nslices)])

    operands = [operand("prev", "in", b * hp * wp, 0)]
    data = {"prev": [_storage(prev, dtype)]}
    if kind != "avgpool" and same_buffer:
        operands.append(operand("srcout", "inout", b * oh * ow, 1, nslices=2))
        nan = torch.full((b * oh * ow, c), float("nan")).to(FU.TORCH_DT[dtype])
        data["srcout"] = [_storage(src, dtype), nan]
    else:
        if kind != "avgpool":
            operands.append(operand("src", "in", b * oh * ow, 1))
            data["src"] = [_storage(src, dtype)]
        operands.append(operand("out", "out", b * oh * ow, 2))
    lay = FU.Layout(operands)
    alloc = torch.empty(lay.total, dtype=torch.uint8, device="cuda")
    FU.fill(alloc, lay, data, poisoned=True)
    base = alloc.data_ptr()
    op = _hip.Y3Op()
    op.kind, op.dtype, op.batch, op.block_idx = KIND_CODE[kind], FU.DT_CODE[dtype], b, 5
    op.ksize = op.stride = 1
    op.in_h, op.in_w, op.in_c, op.in_ld = hp, wp, c, lay["prev"].ld
    op.out_h, op.out_w, op.out_c = oh, ow, c
    op.d_in = lay["prev"].ptr(base)
    if lay.has("srcout"):
        o = lay["srcout"]
        op.d_res, op.res_ld, op.d_out, op.out_ld = o.ptr(base, 0), o.ld, o.ptr(base, 1), o.ld
    else:
        if kind != "avgpool":
            op.d_res, op.res_ld = lay["src"].ptr(base), lay["src"].ld
        op.d_out, op.out_ld = lay["out"].ptr(base), lay["out"].ld
    before = alloc.clone()
    zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    arr = (_hip.Y3Op * 1)(op)
    handle = ctypes.c_void_p()
    opt = _hip.options(**(options or {}))
    _hip.check(lib.y3_plan_create_ex(arr, 1, zero.data_ptr(), ctypes.byref(opt), ctypes.byref(handle)))
    try:
        name = lib.y3_plan_op_kernel(handle, 0).decode()
        dims = _hip.plan_op_dims(handle, 0)
        symbols = []
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())
        with (torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()):
            with _hip.launch_log() as log:
                _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
            symbols.append(log.names)
            for n in range(1, runs):          # (use_graph: the second run captures and launches, later ones replay)
                FU.fill(alloc, lay, data, poisoned=True)          # the output slice is NaN again, on the same stream
                _hip.check(lib.y3_plan_run(handle, None, _hip.stream_ptr()))
        torch.cuda.synchronize()
    finally:
        lib.y3_plan_destroy(handle)
    bad = FU.footprint_violations(before, alloc, lay)
    assert bad is None, "%s %s %s: %s" % (kind, dtype, form, bad)
    if lay.has("srcout"):
        o, k = lay["srcout"], 1
        assert torch.equal(FU.read_slice(alloc, o, 0, torch.uint8), FU.read_slice(before, o, 0, torch.uint8)), "src was written"
    else:
        o, k = lay["out"], 0
    out = FU.read_slice(alloc, o, k, FU.TORCH_DT[dtype]).float().cpu().numpy().reshape(b, oh, ow, c)
    return dict(out=out, kernel=name, symbols=symbols, dims=dims)


# ---- inputs -----------------------------------------------------------------------------------------------------------------

def random_storage(shape, dtype, seed, scale=1.5):
    rng = np.random.default_rng([20259, seed])
    return to_storage((rng.standard_normal(shape) * scale).astype(np.float32), dtype)


def integer_storage(shape, dtype, seed):
    """integer values every storage type holds exactly (|v| <= 128, eight significant bits): a frame's sum of up to 2^16 of
    them stays below 2^24 in every partial sum, so the float32 sum is exact in any order"""
    rng = np.random.default_rng([20260, seed])
    return rng.integers(-128, 129, size=shape).astype(np.float32)


def census_case(key):
    """(kind, form, dtype, prev, src) of the recorded case of one compiled instance: small, several workgroups, odd map"""
    kind, form, dtype = key[len("attn_"):].rsplit("-", 1)[0].rsplit("_", 1) + [key.rsplit("-", 1)[1]]
    c = 3 * vec_of(dtype) if form == "vec" else 13
    seed = CENSUS_KEYS.index(key)
    if kind == "avgpool":
        return kind, form, dtype, random_storage((3, 13, 10, c), dtype, seed), None
    src = random_storage((3, 13, 10, c), dtype, seed)
    prev = random_storage((3, 1, 1, c) if kind == "scale_channels" else (3, 13, 10, c), dtype, seed + 100)
    return kind, form, dtype, prev, src


def run_census_case(key):
    """run the case, hold its values and its footprint, return the sorted symbols it launched"""
    kind, form, dtype, prev, src = census_case(key)
    r = run_op(kind, dtype, prev, src, form=form)
    want = avgpool_ordered_expected(prev, dtype) if kind == "avgpool" else product_expected(src, prev, dtype)
    assert r["kernel"] == "%s_%s" % (kind, TAG[dtype]), (key, r["kernel"])
    assert same_bits(r["out"], want).all(), key
    syms = sorted(set(r["symbols"][0]))
    assert len(syms) == 1 and symbol_matches(syms[0], kind, form, dtype), (key, syms)
    return syms
