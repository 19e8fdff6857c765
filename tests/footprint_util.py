"""Memory footprint of every kernel family: layout, fills, checks and the case table (tests/test_footprint_host.py checks
the table, the arithmetic and the helpers without a GPU; tests/test_gpu_footprint.py runs the cases on an MI355X).

Every operand of a one-op or one-fused-group plan lies inside ONE device allocation as ``[guard | body | guard]``:

  body    pixels x ld elements; the operand's channels are the slice [c0, c0 + c) of every pixel, with c0 > 0 and
          c0 + c < ld in the strided layout (a margin on both sides, as in a route-concat buffer of the arena), c0 = 0 and
          ld = c in the dense layout.  c0 and ld are ODD multiples of the alignment unit the family's chooser demands, so
          they are multiples of nothing larger.  Parameters, the zero page, frames and decode outputs are flat bodies.
  guard   on each side at least max(64 KiB, 256 pixels x ld x element size) -- the widest tile of any kernel is 256 pixels --
          and bodies start on 4 KiB boundaries.  Guards are part of the allocation: a stray access is recorded, it never
          faults.  No operand is ever placed at the end of an allocation.

Input-side operands are surrounded by quiet NaN of their storage type (margins and guards), so a result that depends on a
byte the op does not own is NaN or differs from the dense run.  Output-side operands are surrounded by a fixed byte pattern
and their slice is pre-filled with NaN, so a stray store and a missing store both show.  The whole allocation is compared as
bytes before and after the run."""
import ctypes

import torch

GUARD_MIN = 64 * 1024
TILE_PIXELS = 256
ALIGN = 4096
ES = {"float32": 4, "bf16": 2, "fp16": 2}
TAG = {"float32": "f32", "bf16": "bf16", "fp16": "f16"}
TORCH_DT = {"float32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
# quiet NaN of each storage type, as the little-endian bytes of one element
NAN_BYTES = {"float32": (0x00, 0x00, 0xC0, 0x7F), "bf16": (0xC0, 0x7F), "fp16": (0x00, 0x7E)}
PATTERN_PERIOD = 251            # output-side fill: byte i of the allocation holds 1 + i % 251 (never 0, no power-of-two period)


def round_up(a, b):
    return (a + b - 1) // b * b


class Operand:
    """One ``[guard | body | guard]`` of the allocation.  ``side``: "in" (read only), "out" (the slices are written),
    "inout" (written slices that hold data before the run: the in-place add) or "scratch" (private intermediate of a fused
    group: its body may or may not be written).  ``fmt``: "float32" / "bf16" / "fp16" / "u8" / "i32" / "i64" / "f64"."""

    def __init__(self, name, side, fmt, pixels, ld, slices, tile_elems=None):
        """``tile_elems``: elements one pixel of a tile spans, where that is not ``ld`` (flat parameter arrays: 1; the decode's
        output rows: 4 / 1 / 1)"""
        self.name, self.side, self.fmt = name, side, fmt
        self.es = {"u8": 1, "i32": 4, "i64": 8, "f64": 8}.get(fmt) or ES[fmt]
        self.pixels, self.ld, self.slices = int(pixels), int(ld), [(int(a), int(b)) for a, b in slices]
        self.tile_elems = int(tile_elems or ld)
        self.guard = round_up(max(GUARD_MIN, TILE_PIXELS * self.tile_elems * self.es), ALIGN)
        self.body_bytes = self.pixels * self.ld * self.es
        self.front = self.body = self.end = None         # byte offsets in the allocation (Layout sets them)

    def ptr(self, base, k=0):
        return base + self.body + self.slices[k][0] * self.es

    def region(self, off):
        """(region name, pixel, channel) of byte ``off`` of the allocation, which lies in this operand"""
        if off < self.body:
            return "front guard", -1, -1
        if off >= self.body + self.body_bytes:
            return "back guard", -1, -1
        e = (off - self.body) // self.es
        pix, ch = e // self.ld, e % self.ld
        for k, (c0, c) in enumerate(self.slices):
            if c0 <= ch < c0 + c:
                return "slice %d" % k, pix, ch - c0
        if ch < self.slices[0][0]:
            return "left margin", pix, ch
        if ch >= self.slices[-1][0] + self.slices[-1][1]:
            return "right margin", pix, ch
        return "margin between slices", pix, ch


class Layout:
    def __init__(self, operands):
        self.operands = list(operands)
        off = 0
        for o in self.operands:
            o.front = off
            o.body = off + o.guard
            o.end = round_up(o.body + o.body_bytes + o.guard, ALIGN)
            off = o.end
        self.total = off

    def __getitem__(self, name):
        return next(o for o in self.operands if o.name == name)

    def has(self, name):
        return any(o.name == name for o in self.operands)

    def owner(self, off):
        return next(o for o in self.operands if o.front <= off < o.end)


def strided_ld(c, unit, v, avoid=()):
    """(c0, ld) of a ``c``-channel slice for alignment unit ``unit``; variant ``v`` (0, 1, 2 ...) gives different strides
    to the operands of one op.  c0 and ld are odd multiples of ``unit``; c0 >= unit and ld - c0 - c >= unit."""
    c0 = unit * (1 + 2 * v)
    ld = round_up(c, unit) + c0 + unit * (1 + 2 * v)
    if (ld // unit) % 2 == 0:
        ld += unit
    while ld in avoid:                      # (another operand of the op has this stride already)
        ld += 2 * unit
    return c0, ld


# ------------------------------------------------------------------------------------------------ fills and checks (torch)

def _bytes_tensor(vals, n, device):
    t = torch.tensor(vals, dtype=torch.uint8, device=device)
    return t.repeat(n // len(vals))


def fill(alloc, layout, data, poisoned, u8_guard=0):
    """Lay ``data`` ({operand name: [tensor per slice]}; "out" operands have none) into ``alloc`` (uint8, layout.total bytes).
    ``poisoned``: NaN / pattern around the operands (the strided and aliasing runs); else zeros (the dense run)."""
    dev = alloc.device
    if poisoned:
        pat = (torch.arange(PATTERN_PERIOD, device=dev) + 1).to(torch.uint8)
        alloc.copy_(pat.repeat(layout.total // PATTERN_PERIOD + 1)[:layout.total])
    else:
        alloc.zero_()
    for o in layout.operands:
        whole = alloc[o.front:o.end]
        body = alloc[o.body:o.body + o.body_bytes]
        if o.side in ("in", "inout") and poisoned:
            if o.fmt in NAN_BYTES:
                whole.copy_(_bytes_tensor(NAN_BYTES[o.fmt], o.end - o.front, dev))
            elif o.fmt == "u8":
                whole.fill_(u8_guard)
            else:                                    # integer inputs have no NaN: all-ones (-1; float64: a NaN)
                whole.fill_(0xFF)
        b2 = body.view(o.pixels, o.ld * o.es)
        for k, (c0, c) in enumerate(o.slices):
            sl = b2[:, c0 * o.es:(c0 + c) * o.es]
            if o.side in ("in", "inout"):
                src = data[o.name][k].contiguous().to(dev)
                sl.copy_(src.view(torch.uint8).reshape(o.pixels, c * o.es))
            elif o.side == "out":
                if o.fmt in NAN_BYTES:
                    sl.copy_(_bytes_tensor(NAN_BYTES[o.fmt], o.pixels * c * o.es, dev).view(o.pixels, c * o.es))
                else:
                    sl.fill_(0x7F)                   # integer outputs: a value no kernel here writes (0x7F7F... )
            elif o.side == "pad":
                pass                                 # (the pad of the big-operand layouts: it keeps the fill around it)
            else:
                sl.fill_(0xFF if poisoned else 0)    # scratch / workspace: no kernel may rely on what it finds there


def read_slice(alloc, o, k, dtype):
    """slice ``k`` of operand ``o`` as a (pixels, c) tensor of ``dtype`` (a copy)"""
    c0, c = o.slices[k]
    b2 = alloc[o.body:o.body + o.body_bytes].view(o.pixels, o.ld * o.es)
    return b2[:, c0 * o.es:(c0 + c) * o.es].contiguous().view(dtype).reshape(o.pixels, -1)


def footprint_violations(before, after, layout, writable=("out", "inout", "scratch")):
    """None, or a message naming the first byte that changed outside the slices the run may write: which operand, which
    region (left / right margin, front / back guard, or the slice of a read-only operand), pixel, channel, bytes changed."""
    diff = before != after
    for o in layout.operands:
        if o.side not in writable:
            continue
        b2 = diff[o.body:o.body + o.body_bytes].view(o.pixels, o.ld * o.es)
        if o.side == "scratch":
            b2.zero_()
            continue
        for c0, c in o.slices:
            b2[:, c0 * o.es:(c0 + c) * o.es] = False
    if not bool(diff.any()):
        return None
    offs = torch.nonzero(diff).flatten().cpu().numpy()
    return describe(offs, layout)


def describe(offs, layout):
    """message for the changed byte offsets ``offs`` (sorted, non-empty)"""
    first = int(offs[0])
    o = layout.owner(first)
    region, pix, ch = o.region(first)
    in_op = offs[(offs >= o.front) & (offs < o.end)]
    same = sum(1 for x in in_op[:100000] if o.region(int(x))[0] == region)
    where = "" if pix < 0 else ", first at pixel %d channel %d" % (pix, ch)
    return "operand '%s' (%s): %s changed%s (allocation byte %d, %d bytes of it inside the operand); %d bytes changed in that region, %d in all" % (
        o.name, o.side, region, where, first, first - o.front, same, len(offs))


# ------------------------------------------------------------------------------------------------ the case table

def _H():
    from yolov3 import _hip
    return _hip


def _opts():
    """option sets that force each family (the masks of tests/kernel_choice_util.py OPTION_SETS and tests/test_gpu_parity.py)"""
    H = _H()
    halo = H.AM_HALO_ALL | H.AM_NO_SMALL_GRID
    return dict(
        igemm1=dict(auto_mask=0, igemm_version=1),
        igemm2=dict(auto_mask=0),
        igemm2_noshrink=dict(auto_mask=H.AM_NO_BN_SHRINK),
        igemm2_96=dict(auto_mask=0, igemm_bm=96),
        igemm3=dict(auto_mask=0, igemm_version=3),
        igemm3_64=dict(auto_mask=0, igemm_version=3, igemm_bm=64),
        igemm3_ns4=dict(auto_mask=0, igemm_version=3, igemm_ns=4),
        igemm3_64_ns4=dict(auto_mask=0, igemm_version=3, igemm_bm=64, igemm_ns=4),
        halo192=dict(auto_mask=halo),
        halo256=dict(auto_mask=halo | H.AM_HALO_TILE256),
        halo_dw=dict(auto_mask=halo | H.AM_HALO_DW_ALWAYS),
        patch=dict(auto_mask=halo | H.AM_PATCH_WIDE),
        wres=dict(auto_mask=H.AM_WRES_ALWAYS),
        dw1x1=dict(auto_mask=H.AM_1X1_DW),
        dw48=dict(auto_mask=H.AM_SMALL_DW | H.AM_SMALL_DW_ALWAYS),
        default={},
        stem_phased=dict(fuse_stem=2),
        fuse_block=dict(fuse_block=2),
        # the sets under which a chooser rule that reads the CU count decides (tests/cu_count_util.py ONE_OP_ROWS): the fused block only
        # where its rectangles fill 70 % of the chip, the direct-weights strip kernel only where its cost model says it pays, the
        # small-grid kernel with the wave count and the grid limits its chooser picks, the default set without that kernel (the small-grid rule of
        # the 3x3 layers), the deep-1x1 rule alone
        fuse_block1=dict(fuse_block=1),
        # the direct-weights form of the fused block wherever supported (tests/block_dw_cases.py: a table of its own, the kernel
        # lives in libyolov3_hip_block.so, the "block" library of tests/kernel_census.py)
        fuse_block4=dict(fuse_block=4),
        # ... and only where its rectangles fill 70 % of the chip, the rule of fuse_block = 1 (tests/test_cu_count_host.py)
        fuse_block3=dict(fuse_block=3),
        halo_dw_pays=dict(auto_mask=halo | H.AM_HALO_DW),
        dw48_auto=dict(auto_mask=H.AM_SMALL_DW | H.AM_SMALL_DW_WIDE),
        no_small_dw=dict(auto_mask=H.AM_DEFAULT & ~(H.AM_SMALL_DW | H.AM_SMALL_DW_WIDE)),
        deep_1x1=dict(auto_mask=H.AM_IGEMM3_1X1_DEEP),
        head_tiled=dict(fuse_head=2),
        head48=dict(fuse_head=3),
        head96=dict(fuse_head=4),
        head_unfused=dict(fuse_head=0),
    )


F32, B16, ALL = ("float32",), ("bf16", "fp16"), ("float32", "bf16", "fp16")


def _conv(cid, family, opt, dtypes, B, h, w, cin, cout, k, s, res=False, inp="act", out_unit=None, pad=None, **kw):
    """``pad``: None is a cfg block with ``pad=1`` ((k - 1) // 2); 0 is one that leaves the key out"""
    return dict(id=cid, group="conv", family=family, opt=opt, dtypes=dtypes, B=B, h=h, w=w, cin=cin, cout=cout, k=k, s=s,
                res=res, inp=inp, out_unit=out_unit, pad=conv_pad(k, pad), **kw)


def conv_pad(k, pad=None):
    return (k - 1) // 2 if pad is None else pad


def _layer(cid, family, kind, dtypes, B, h, w, c, k=1, s=1, wide=True, dk=False, alias=False, opt="default"):
    return dict(id=cid, group="layer", family=family, kind=kind, opt=opt, dtypes=dtypes, B=B, h=h, w=w, c=c, k=k, s=s,
                wide=wide, dk=dk, alias=alias)


def cases():
    """Every case: at least a full-tile and a ragged shape per family (the last pixel tile partial, the map not square where
    the family allows it), with and without the shortcut operand where the family takes one.  ``family`` is the kernel name
    with %s for the dtype tag.  Shapes stay at or below 16 x 76 x 76 x 512.  The rows of ``tiny_cases()`` follow them: every
    family once more on maps of one pixel a side.

    Below the family name the library is compiled by INSTANCE (the y3_ints lists of the .hip files): the rows marked
    "instance" are there for one compiled device function that no other row launches (tests/kernel_census.py has the proof that
    none is left out).  A row with ``nkt`` is for a direct-weights instance of that K depth, which dictates its channel count,
    in_c = 64 x nkt per halo image: the only rows that may exceed 512 channels.  ``wide_map``: the two-image stride-2 form of
    conv_dw48 at 256 channels, whose halo image outgrows LDS only on rows of 124 pixels and more."""
    C = []
    # ---- implicit GEMMs (conv_igemm.hip).  Tile widths follow Cout (128 / 64 / 32); version 2 shrinks them on small grids
    # unless AM_NO_BN_SHRINK; pixel tiles are 128 (96, 64): "full" shapes have B*Ho*Wo a multiple of the tile
    for ver, opt, fam in (("igemm1", "igemm1", "conv_igemm_%s"), ("igemm2", "igemm2_noshrink", "conv_igemm2_%s")):
        C += [
            _conv(ver + "_128_full", fam + "_128x128", opt, ALL, 2, 16, 16, 64, 128, 3, 1, res=True),
            _conv(ver + "_128_ragged", fam + "_128x128", opt, ALL, 3, 13, 11, 128, 256, 1, 1),
            _conv(ver + "_128_ragged_s2_res", fam + "_128x128", opt, ALL, 1, 27, 21, 128, 128, 3, 2, res=True),
            _conv(ver + "_64_full", fam + "_128x64", opt, ALL, 1, 16, 16, 128, 64, 1, 1),
            _conv(ver + "_64_ragged_res", fam + "_128x64", opt, ALL, 2, 15, 9, 32, 64, 3, 1, res=True),
            _conv(ver + "_32_full", fam + "_128x32", opt, ALL, 1, 16, 8, 64, 32, 1, 1, res=True),
            _conv(ver + "_32_ragged", fam + "_128x32", opt, ALL, 1, 19, 13, 16, 32, 3, 1),
            # K-tilings and kernel geometry that only a user's own cfg reaches (igemm_ktiles: KMODE 0 when in_c is a multiple of
            # the K-tile -- 32 float32 / 64 16-bit elements --, 2 when the K-tile is a multiple of in_c, 1 otherwise).
            # KMODE 1, every tap but the first straddles two K-tiles, K = 216 ends inside a K-tile in every dtype
            _conv(ver + "_k3_c24_res", fam + "_128x64", opt, ALL, 2, 15, 9, 24, 64, 3, 1, res=True),
            _conv(ver + "_k3s2_c40", fam + "_128x128", opt, ALL, 1, 27, 21, 40, 128, 3, 2),                    # KMODE 1
            # KMODE 2 with the 25-bit tap mask: 4 (float32) / 8 (16-bit) taps per K-tile, the last K-tile holds one tap
            _conv(ver + "_k5_c8", fam + "_128x32", opt, ALL, 2, 13, 11, 8, 32, 5, 1),
            _conv(ver + "_1x1_c72", fam + "_128x128", opt, ALL, 3, 13, 11, 72, 128, 1, 1),      # KMODE 1: 2.25 / 1.125 K-tiles
            _conv(ver + "_k5s2_c64", fam + "_128x64", opt, ALL, 1, 27, 21, 64, 64, 5, 2),       # KMODE 0 with 25 taps
            _conv(ver + "_k4s2_c16", fam + "_128x32", opt, ALL, 1, 26, 22, 16, 32, 4, 2),       # an even kernel, pad 1
            # a 3x3 block without a pad= key: no tap is ever masked, 15 x 9 -> 13 x 7
            _conv(ver + "_k3_pad0_c32", fam + "_128x64", opt, ALL, 2, 15, 9, 32, 64, 3, 1, pad=0),
        ]
    C += [
        # ragged channel tail: 255 float32 head channels (the head conv: bias only, float32 out).  Under the DEFAULT igemm_version
        # 2 a 16-bit conv with Y3_F_OUT_F32 runs on the version-1 kernel, whose direct epilogue measured faster
        # (conv_igemm.hip, y3_choose_conv_igemm): this is the form the shipped plans run, hence option set "igemm2"
        _conv("igemm_head_f32out", "conv_igemm_%s_128x128", "igemm2", B16, 2, 13, 13, 256, 255, 1, 1, out_f32=True, leaky=False, dense_out_ld=256),
        _conv("igemm2_96_full", "conv_igemm2_%s_96x64", "igemm2_96", ALL, 2, 12, 12, 128, 128, 1, 1, res=True),
        _conv("igemm2_96_ragged", "conv_igemm2_%s_96x64", "igemm2_96", ALL, 3, 13, 7, 128, 192, 3, 1),
        _conv("igemm3_128_full", "conv_igemm3_%s_128x128", "igemm3", ALL, 2, 16, 16, 128, 128, 3, 1, res=True),
        _conv("igemm3_128_ragged", "conv_igemm3_%s_128x128", "igemm3", ALL, 3, 19, 13, 256, 256, 1, 1),
        _conv("igemm3_128_ragged_s2", "conv_igemm3_%s_128x128", "igemm3", ALL, 2, 27, 21, 64, 128, 3, 2),
        _conv("igemm3_64_full", "conv_igemm3_%s_64x128", "igemm3_64", B16, 1, 16, 16, 256, 128, 1, 1, res=True),
        _conv("igemm3_64_ragged", "conv_igemm3_%s_64x128", "igemm3_64", B16, 3, 13, 9, 128, 256, 3, 1),
    ]
    for ver, opt, fam, dts in (("igemm3_128", "igemm3", "conv_igemm3_%s_128x128", ALL), ("igemm3_64", "igemm3_64", "conv_igemm3_%s_64x128", B16)):
        C += [
            _conv(ver + "_k3s2_c40", fam, opt, dts, 1, 27, 21, 40, 128, 3, 2),                   # KMODE 1
            _conv(ver + "_1x1_c72", fam, opt, dts, 3, 13, 11, 72, 128, 1, 1),                    # KMODE 1
            _conv(ver + "_k5_c16_res", fam, opt, dts, 2, 13, 11, 16, 128, 5, 1, res=True),       # KMODE 2, 25 taps
            _conv(ver + "_k3_c160_res", fam, opt, dts, 1, 19, 19, 160, 128, 3, 1, res=True),     # KMODE 1 in 16 bits (0 in float32)
        ]
    C += [
        _conv("igemm2_96_k3s2_c40", "conv_igemm2_%s_96x64", "igemm2_96", ALL, 1, 27, 21, 40, 128, 3, 2),
        _conv("igemm2_96_k5_c16_res", "conv_igemm2_%s_96x64", "igemm2_96", ALL, 2, 13, 11, 16, 128, 5, 1, res=True),
        # the route by which an unforced plan reaches KMODE 1: the chooser's own small-grid rule (api.hip choose_conv) sends a
        # 160 -> 128 3x3 layer on a 19 x 19 map to the wave-specialised implicit GEMM
        _conv("default_k3_c160", "conv_igemm3_%s_128x128", "default", B16, 1, 19, 19, 160, 128, 3, 1, res=True),
        # instances: the LDS-DMA kernel's K-tilings on the tiles the rows above leave out (KMODE 2 at 128 x 128 and, in float32, at
        # 128 x 64; KMODE 1 at 128 x 32) ...
        _conv("igemm2_128_k3_c16", "conv_igemm2_%s_128x128", "igemm2_noshrink", ALL, 2, 13, 11, 16, 128, 3, 1, res=True),
        _conv("igemm2_64_k3_c16", "conv_igemm2_%s_128x64", "igemm2_noshrink", ALL, 1, 19, 13, 16, 64, 3, 1),
        _conv("igemm2_32_k3_c24", "conv_igemm2_%s_128x32", "igemm2_noshrink", ALL, 2, 15, 9, 24, 32, 3, 1, res=True),
        # ... and the wave-specialised kernel with FOUR LDS stages (igemm_ns = 4; every row above runs the default three), each
        # K-tiling on both tiles
        _conv("igemm3_128_ns4_full", "conv_igemm3_%s_128x128", "igemm3_ns4", ALL, 2, 16, 16, 128, 128, 3, 1, res=True),
        _conv("igemm3_128_ns4_k3s2_c40", "conv_igemm3_%s_128x128", "igemm3_ns4", ALL, 1, 27, 21, 40, 128, 3, 2),
        _conv("igemm3_128_ns4_k5_c16_res", "conv_igemm3_%s_128x128", "igemm3_ns4", ALL, 2, 13, 11, 16, 128, 5, 1, res=True),
        _conv("igemm3_64_ns4_ragged", "conv_igemm3_%s_64x128", "igemm3_64_ns4", B16, 3, 13, 9, 128, 256, 3, 1),
        _conv("igemm3_64_ns4_1x1_c72", "conv_igemm3_%s_64x128", "igemm3_64_ns4", B16, 3, 13, 11, 72, 128, 1, 1),
        _conv("igemm3_64_ns4_k5_c16_res", "conv_igemm3_%s_64x128", "igemm3_64_ns4", B16, 2, 13, 11, 16, 128, 5, 1, res=True),
        # ---- halo-reuse strip kernels (conv_halo.hip): 192- / 256-pixel strips of whole rows x 128 channels; float32 too
        _conv("halo192_full", "conv_halo_ws_%s_192x128", "halo192", ALL, 2, 24, 16, 128, 128, 3, 1, res=True, out_unit=8),
        _conv("halo192_ragged", "conv_halo_ws_%s_192x128", "halo192", ALL, 3, 19, 13, 128, 256, 3, 1, out_unit=8),
        _conv("halo192_ragged_res", "conv_halo_ws_%s_192x128", "halo192", ALL, 2, 38, 26, 256, 128, 3, 1, res=True, out_unit=8),
        _conv("halo256_full", "conv_halo_ws_%s_256x128", "halo256", ALL, 2, 16, 16, 128, 128, 3, 1, res=True, out_unit=8),
        _conv("halo256_ragged", "conv_halo_ws_%s_256x128", "halo256", ALL, 3, 19, 13, 128, 256, 3, 1, out_unit=8),
        _conv("halo256_ragged_76", "conv_halo_ws_%s_256x128", "halo256", ALL, 1, 76, 52, 128, 128, 3, 1, res=True, out_unit=8),
        # instance: rows of 63 px and more leave the 256-pixel tile THREE weight slots (conv_halo.hip launch_conv_halo: na > 12)
        _conv("halo256_ring3_w76", "conv_halo_ws_%s_256x128", "halo256", ALL, 1, 26, 76, 128, 128, 3, 1, res=True, out_unit=8),
        # direct-weights strip kernel: 192 pixels x 256 channels, fragment-order weights
        _conv("halo_dw_full", "conv_halo_dw_%s_192x256", "halo_dw", B16, 2, 24, 16, 128, 256, 3, 1, res=True),
        _conv("halo_dw_ragged", "conv_halo_dw_%s_192x256", "halo_dw", B16, 3, 19, 13, 256, 512, 3, 1),
        _conv("halo_dw_ragged_res", "conv_halo_dw_%s_192x256", "halo_dw", B16, 2, 38, 26, 128, 256, 3, 1, res=True),
        # 13 tiles of 192 pixels x 2 channel tiles: one round on 32 CUs, where 10 tiles of 256 x 4 of the wave-specialised kernel are
        # two -- the shape at which y3_conv_halo_dw_pays decides by the CU count (tests/cu_count_util.py: option set halo_dw_pays)
        _conv("halo_dw_ragged_29x27", "conv_halo_dw_%s_192x256", "halo_dw", B16, 3, 29, 27, 256, 512, 3, 1),
        # instances: five halo passes per chunk (rows of 31 .. 62 px) and six (63 .. 94); the rows above have four
        _conv("halo_dw_na5_w38", "conv_halo_dw_%s_192x256", "halo_dw", B16, 1, 19, 38, 128, 256, 3, 1, res=True),
        _conv("halo_dw_na6_w76", "conv_halo_dw_%s_192x256", "halo_dw", B16, 1, 13, 76, 128, 256, 3, 1),
        # 2-D patch kernel: 8 x 32 output tiles; its chooser asks rows wider than 128 px (api.hip: `w > 128`), so these maps are
        # wide and low: h * w stays below 76 * 76
        _conv("patch_full", "conv_patch_wsp_%s_8x32x128", "patch", ALL, 1, 16, 160, 64, 128, 3, 1, res=True, out_unit=8),
        _conv("patch_ragged", "conv_patch_wsp_%s_8x32x128", "patch", ALL, 2, 13, 139, 64, 128, 3, 1, out_unit=8),
        _conv("patch_ragged_res", "conv_patch_wsp_%s_8x32x128", "patch", ALL, 1, 21, 150, 64, 256, 3, 1, res=True, out_unit=8),
        # 6 x 4 tiles x 2 frames x 2 channel tiles = 96 tiles: on 20 CUs a workgroup owns 5 or 4 of them, in two frames and both channel tiles
        _conv("patch_strided_tiles", "conv_patch_wsp_%s_8x32x128", "patch", ALL, 2, 29, 161, 64, 256, 3, 1, res=True, out_unit=8),
        # ---- 1x1 kernels (conv_1x1.hip): weights-resident persistent (128-pixel tiles), direct-weights (48 / 96 pixels)
        _conv("wres_128_full", "conv1x1_wres_%s_128x128", "wres", B16, 2, 16, 16, 256, 128, 1, 1),
        _conv("wres_128_ragged", "conv1x1_wres_%s_128x128", "wres", B16, 3, 19, 13, 256, 128, 1, 1),
        _conv("wres_64_full", "conv1x1_wres_%s_128x64", "wres", B16, 2, 16, 16, 128, 64, 1, 1),
        _conv("wres_64_ragged", "conv1x1_wres_%s_128x64", "wres", B16, 3, 21, 17, 128, 64, 1, 1),
        # persistent grids whose workgroups own SEVERAL tiles each, and unequal numbers of them, on a device of 20 CUs
        # (tests/cu_count_util.py; on 256 CUs the rows above and these give every workgroup one tile): 40 pixel tiles x 3 channel
        # tiles on 18 workgroups, six per channel tile -- 20 is no multiple of 3 -- which stream 7 or 6 pixel tiles each
        _conv("wres_128_strided_tiles", "conv1x1_wres_%s_128x128", "wres", B16, 3, 39, 43, 256, 384, 1, 1),
        _conv("wres_64_strided_tiles", "conv1x1_wres_%s_128x64", "wres", B16, 3, 39, 43, 128, 192, 1, 1),
        # (the direct-weights kernel takes grids of one round only: 96-pixel tiles from 192 tiles on, 48-pixel tiles for 64 ..
        # 191 -- conv_1x1.hip dw1x1_bm -- hence the batches)
        _conv("dw1x1_96_full", "conv1x1_dw_%s_96x256", "dw1x1", B16, 16, 36, 32, 512, 256, 1, 1),
        _conv("dw1x1_96_ragged", "conv1x1_dw_%s_96x256", "dw1x1", B16, 16, 38, 37, 512, 256, 1, 1),
        _conv("dw1x1_48_full", "conv1x1_dw_%s_48x256", "dw1x1", B16, 8, 24, 16, 512, 256, 1, 1),
        _conv("dw1x1_48_ragged", "conv1x1_dw_%s_48x256", "dw1x1", B16, 9, 19, 19, 512, 256, 1, 1),
        # instances: the K depths 4, 6 and 12 at both tile heights and 16 at 48 pixels (the rows above: 8), on the maps of the rows
        # above (768 channels: on the fewest 96-pixel tiles the chooser takes, 197)
        _conv("dw1x1_96_c256", "conv1x1_dw_%s_96x256", "dw1x1", B16, 16, 38, 37, 256, 256, 1, 1, nkt=4),
        _conv("dw1x1_96_c384", "conv1x1_dw_%s_96x256", "dw1x1", B16, 16, 38, 37, 384, 256, 1, 1, nkt=6),
        _conv("dw1x1_96_c768", "conv1x1_dw_%s_96x256", "dw1x1", B16, 16, 38, 31, 768, 256, 1, 1, nkt=12),
        _conv("dw1x1_48_c256", "conv1x1_dw_%s_48x256", "dw1x1", B16, 9, 19, 19, 256, 256, 1, 1, nkt=4),
        _conv("dw1x1_48_c384", "conv1x1_dw_%s_48x256", "dw1x1", B16, 9, 19, 19, 384, 256, 1, 1, nkt=6),
        _conv("dw1x1_48_c768", "conv1x1_dw_%s_48x256", "dw1x1", B16, 9, 19, 19, 768, 256, 1, 1, nkt=12),
        _conv("dw1x1_48_c1024", "conv1x1_dw_%s_48x256", "dw1x1", B16, 9, 19, 19, 1024, 256, 1, 1, nkt=16),
        # ---- small-grid direct-weights kernel (conv_dw48.hip): 48-pixel tiles, one frame at a time
        _conv("dw48_k1_full", "conv_dw48_k1_%s", "dw48", B16, 1, 24, 16, 256, 128, 1, 1, res=True),
        _conv("dw48_k1_ragged", "conv_dw48_k1_%s", "dw48", B16, 2, 19, 13, 512, 256, 1, 1),
        _conv("dw48_k3_full", "conv_dw48_k3_%s", "dw48", B16, 1, 24, 16, 128, 256, 3, 1, res=True),
        _conv("dw48_k3_ragged", "conv_dw48_k3_%s", "dw48", B16, 2, 19, 13, 256, 512, 3, 1),
        _conv("dw48_k3_ragged_res", "conv_dw48_k3_%s", "dw48", B16, 1, 38, 23, 128, 256, 3, 1, res=True),
        _conv("dw48_k3s2_full", "conv_dw48_k3s2_%s", "dw48", B16, 1, 48, 32, 128, 256, 3, 2),
        _conv("dw48_k3s2_ragged", "conv_dw48_k3s2_%s", "dw48", B16, 2, 38, 26, 256, 512, 3, 2),
        _conv("dw48_k3s2_ragged_1frame", "conv_dw48_k3s2_%s", "dw48", B16, 1, 38, 22, 256, 512, 3, 2),
        # instances: 1x1 with 2, 6, 12 and 16 K-steps (the rows above: 4 and 8); 3x3 with 8; stride 2 with one K-step (64 channels)
        # and as two halo images of half the channels each, 4 K-steps per image (512 channels on any map) and 2 (256 channels,
        # where one image of all channels outgrows LDS: 124 px and wider)
        _conv("dw48_k1_c128_res", "conv_dw48_k1_%s", "dw48", B16, 1, 19, 13, 128, 128, 1, 1, res=True, nkt=2),
        _conv("dw48_k1_c384", "conv_dw48_k1_%s", "dw48", B16, 2, 13, 11, 384, 256, 1, 1, nkt=6),
        _conv("dw48_k1_c768", "conv_dw48_k1_%s", "dw48", B16, 1, 19, 13, 768, 256, 1, 1, nkt=12),
        _conv("dw48_k1_c1024_res", "conv_dw48_k1_%s", "dw48", B16, 2, 13, 11, 1024, 128, 1, 1, res=True, nkt=16),
        _conv("dw48_k3_c512_res", "conv_dw48_k3_%s", "dw48", B16, 1, 19, 13, 512, 256, 3, 1, res=True, nkt=8),
        _conv("dw48_k3s2_c64", "conv_dw48_k3s2_%s", "dw48", B16, 1, 38, 26, 64, 128, 3, 2, nkt=1),
        _conv("dw48_k3s2_c512_two_images", "conv_dw48_k3s2_%s", "dw48", B16, 1, 26, 22, 512, 256, 3, 2, nkt=4),
        _conv("dw48_k3s2_c256_two_images", "conv_dw48_k3s2_%s", "dw48", B16, 1, 6, 126, 256, 128, 3, 2, nkt=2, wide_map=True),
        # ---- stems (conv_small.hip): the network input is a whole dense tensor by definition (no pixel stride), so only the
        # output is a slice; the input is an exact-size body between guards (uint8 frames: guards 0x00 and 0xFF)
        _conv("stem_nchw_full", "conv_stem3x3_nchw_%s", "default", ALL, 2, 32, 32, 3, 32, 3, 1, inp="nchw"),
        _conv("stem_nchw_ragged", "conv_stem3x3_nchw_%s", "default", ALL, 3, 29, 21, 3, 16, 3, 1, inp="nchw"),
        _conv("stem_u8_f32_full", "conv_stem3x3_u8_%s", "default", F32, 2, 32, 32, 3, 32, 3, 1, inp="u8"),
        _conv("stem_u8_f32_ragged", "conv_stem3x3_u8_%s", "default", F32, 3, 29, 21, 3, 16, 3, 1, inp="u8"),
        _conv("stem_mfma_full", "conv_stem_mfma_u8_%s", "default", B16, 2, 32, 32, 3, 32, 3, 1, inp="u8"),
        _conv("stem_mfma_ragged", "conv_stem_mfma_u8_%s", "default", B16, 3, 29, 21, 3, 32, 3, 1, inp="u8"),
        _conv("stem_mfma_ragged_16ch", "conv_stem_mfma_u8_%s", "default", B16, 1, 45, 37, 3, 16, 3, 1, inp="u8"),
        # instance: uint8 frames into a 16-bit network where the MFMA stem declines (stride 2; more than 32 output channels): the
        # VALU stem kernel with 16-bit stores.  No shipped cfg reaches it
        _conv("stem_u8_16bit_s2", "conv_stem3x3_u8_%s", "default", B16, 2, 32, 32, 3, 32, 3, 2, inp="u8"),
        _conv("stem_u8_16bit_c48", "conv_stem3x3_u8_%s", "default", B16, 3, 29, 21, 3, 48, 3, 1, inp="u8"),
        # ---- the direct fallback (conv_small.hip conv_direct_kernel, one thread per output element): what api.hip conv_path gives
        # a conv on activations that the implicit GEMMs decline (in_c no multiple of the 16-byte chunk, size > 5, out_ld % 4 != 0)
        # and a network-input conv that is not 3 channels x 3x3.  No shipped cfg reaches it
        _conv("direct_odd_cin_res", "conv_direct_%s", "default", ALL, 2, 13, 11, 13, 24, 3, 1, res=True),
        _conv("direct_odd_both_s2", "conv_direct_%s", "default", ALL, 3, 19, 13, 21, 13, 3, 2),
        _conv("direct_k7_s2", "conv_direct_%s", "default", ALL, 1, 19, 13, 16, 32, 7, 2),
        _conv("direct_f32_logits", "conv_direct_%s", "default", ALL, 2, 7, 5, 21, 18, 1, 1, out_f32=True, leaky=False),
        _conv("direct_nchw_k5_s2", "conv_direct_%s", "default", ALL, 2, 21, 17, 3, 16, 5, 2, inp="nchw"),
        _conv("direct_nchw_grey", "conv_direct_%s", "default", ALL, 2, 16, 16, 1, 16, 3, 1, inp="nchw"),
        _conv("direct_u8_k5", "conv_direct_%s", "default", ALL, 2, 21, 17, 3, 16, 5, 1, inp="u8"),
        _conv("direct_u8_grey_s2", "conv_direct_%s", "default", ALL, 2, 22, 18, 1, 16, 3, 2, inp="u8"),
    ]
    # ---- fused groups, laid out as the plan lays them: private intermediate, input and output are slices
    C += [
        dict(id="stem_s2_full", group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="default", dtypes=B16, B=2, h=64, w=64),
        dict(id="stem_s2_ragged", group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="default", dtypes=B16, B=3, h=45, w=37),
        # instance: the phase-by-phase form of the fused stem pair (fuse_stem = 2), one name with the pipelined form
        dict(id="stem_s2_phased_full", group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="stem_phased", dtypes=B16, B=2, h=64, w=64),
        dict(id="stem_s2_phased_ragged", group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="stem_phased", dtypes=B16, B=3, h=45, w=37),
        # 3 x 5 tiles of 16 x 8 (pipelined) / 3 x 3 of 16 x 16 (phased, and the residual block) x 5 frames = 75 / 45 tiles: on 20 CUs a
        # workgroup owns 4 or 3 / 3 or 2 of them; on one CU one workgroup owns them all (tests/cu_count_util.py)
        dict(id="stem_s2_strided_tiles", group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="default", dtypes=B16, B=5, h=74, w=70),
        dict(id="stem_s2_phased_strided_tiles", group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="stem_phased", dtypes=B16, B=5, h=74, w=70),
        dict(id="resblock_strided_tiles", group="resblock", family="conv_resblock_fused_%s_64_32_64", opt="default", dtypes=B16, B=5, h=45, w=37),
        # the shortcut operand of the fused residual block IS the group's input (always: the chooser requires it)
        dict(id="resblock_full", group="resblock", family="conv_resblock_fused_%s_64_32_64", opt="default", dtypes=B16, B=2, h=32, w=32),
        dict(id="resblock_ragged", group="resblock", family="conv_resblock_fused_%s_64_32_64", opt="default", dtypes=B16, B=3, h=29, w=21),
        dict(id="block_full_res", group="block", family="conv_block_fused_%s_x128", opt="fuse_block", dtypes=B16, B=2, h=32, w=32, cin=256, cout=256, res=True),
        dict(id="block_ragged_res", group="block", family="conv_block_fused_%s_x128", opt="fuse_block", dtypes=B16, B=3, h=19, w=13, cin=256, cout=256, res=True),
        dict(id="block_ragged_nores", group="block", family="conv_block_fused_%s_x128", opt="fuse_block", dtypes=B16, B=2, h=21, w=17, cin=192, cout=128, res=False),
        # a 19 x 19 map is ONE rectangle of 361 of the 384 pixels a workgroup takes: on one CU three frames fill 94 % of three rounds,
        # which passes the 70 % rule of fuse_block = 1 (tests/cu_count_util.py); on 256 CUs they fill 1 % of one
        dict(id="block_19x19_res", group="block", family="conv_block_fused_%s_x128", opt="fuse_block", dtypes=B16, B=3, h=19, w=19, cin=256, cout=256, res=True),
        dict(id="head_tiled_full", group="head", family="conv_head_decode_%s_64x256", opt="head_tiled", dtypes=B16, B=2, h=16, w=16, cin=256),
        dict(id="head_tiled_ragged", group="head", family="conv_head_decode_%s_64x256", opt="head_tiled", dtypes=B16, B=3, h=13, w=11, cin=192),
        dict(id="head48_full", group="head", family="conv_head_decode_dw_%s_48x256", opt="head48", dtypes=B16, B=2, h=12, w=12, cin=256),
        dict(id="head48_ragged", group="head", family="conv_head_decode_dw_%s_48x256", opt="head48", dtypes=B16, B=3, h=19, w=13, cin=512),
        dict(id="head96_full", group="head", family="conv_head_decode_dw_%s_96x256", opt="head96", dtypes=B16, B=2, h=12, w=12, cin=256),
        dict(id="head96_ragged", group="head", family="conv_head_decode_dw_%s_96x256", opt="head96", dtypes=B16, B=3, h=19, w=13, cin=512),
        # instance: sixteen K-steps (48-pixel tiles only: conv_1x1.hip dw_head_bm)
        dict(id="head48_c1024", group="head", family="conv_head_decode_dw_%s_48x256", opt="head48", dtypes=B16, B=1, h=13, w=11, cin=1024, nkt=16),
    ]
    # ---- layer kernels (layers.hip): the wide form (16-byte vectors) and the element-wise form, which is chosen when in_c or a
    # stride is not a multiple of the vector width
    for wide, tag, c in ((True, "wide", 64), (False, "elem", 13)):
        C += [
            _layer("maxpool_s1_" + tag, "maxpool_%s", "maxpool", ALL, 2, 13, 11, c, k=2, s=1, wide=wide),
            _layer("maxpool_s1_k5_" + tag, "maxpool_%s", "maxpool", ALL, 1, 19, 13, c, k=5, s=1, wide=wide),
            _layer("maxpool_s2_" + tag, "maxpool_%s", "maxpool", ALL, 3, 26, 22, c, k=2, s=2, wide=wide),
            _layer("maxpool_dk_s1_" + tag, "maxpool_dk_%s", "maxpool", ALL, 2, 13, 11, c, k=5, s=1, wide=wide, dk=True),
            _layer("maxpool_dk_s2_" + tag, "maxpool_dk_%s", "maxpool", ALL, 3, 27, 21, c, k=2, s=2, wide=wide, dk=True),
            _layer("upsample_" + tag, "upsample_%s", "upsample", ALL, 2, 13, 11, c, s=2, wide=wide),
            _layer("add_" + tag, "add_%s", "add", ALL, 3, 19, 13, c, wide=wide),
            _layer("add_inplace_" + tag, "add_%s", "add", ALL, 3, 19, 13, c, wide=wide, alias=True),
            _layer("copy_" + tag, "copy_%s", "copy", ALL, 3, 19, 13, c, wide=wide),
        ]
    # Darknet's [reorg] (layers.hip reorg_kernel: one instance per element size), the flat form and the space-to-depth form
    C += [
        dict(id="reorg_full", group="reorg", family="reorg_%s", opt="default", dtypes=ALL, B=2, h=16, w=16, c=64, s=2, form3d=False),
        dict(id="reorg_ragged", group="reorg", family="reorg_%s", opt="default", dtypes=ALL, B=3, h=14, w=10, c=12, s=2, form3d=False),
        dict(id="reorg3d_full", group="reorg", family="reorg3d_%s", opt="default", dtypes=ALL, B=2, h=16, w=16, c=64, s=2, form3d=True),
        dict(id="reorg3d_ragged", group="reorg", family="reorg3d_%s", opt="default", dtypes=ALL, B=3, h=15, w=9, c=13, s=3, form3d=True),
    ]
    C += [
        dict(id="spp_full", group="spp", family="maxpool_spp_pyramid_%s", opt="default", dtypes=ALL, B=2, h=16, w=16, c=64, dk=False),
        dict(id="spp_ragged", group="spp", family="maxpool_spp_pyramid_%s", opt="default", dtypes=ALL, B=3, h=19, w=13, c=48, dk=False),
        dict(id="spp_dk_full", group="spp", family="maxpool_spp_pyramid_dk_%s", opt="default", dtypes=ALL, B=2, h=16, w=16, c=64, dk=True),
        dict(id="spp_dk_ragged", group="spp", family="maxpool_spp_pyramid_dk_%s", opt="default", dtypes=ALL, B=3, h=19, w=13, c=48, dk=True),
        # yolo decode: 255 channels at stride 256 (channel 255 poisoned) and a wider stride; rows at row_offset > 0 of more rows
        dict(id="yolo_ld256", group="yolo", family="yolo_decode_f32", opt="default", dtypes=ALL, B=2, h=13, w=11, n_anchor=3, ncls=80, ld=256, c0=0),
        dict(id="yolo_wide_stride", group="yolo", family="yolo_decode_f32", opt="default", dtypes=ALL, B=3, h=7, w=9, n_anchor=3, ncls=80, ld=268, c0=4),
        dict(id="yolo_few_classes", group="yolo", family="yolo_decode_f32", opt="default", dtypes=ALL, B=2, h=5, w=6, n_anchor=2, ncls=7, ld=36, c0=4),
    ]
    return C + tiny_cases()


# ------------------------------------------------------------------------------------------------ degenerate maps
# Every family once more on maps of one pixel a side: every pixel is a border pixel on two or four sides, a pixel tile holds
# many whole frames and ends inside one, a halo row is W + 1 = 2 pixels and wraps through several frames, a 13-wide pool window
# has one tap inside the image.  Three shapes per family, named by the OUTPUT map; a stride-2 family reads the input that gives it:
TINY_SHAPES = (("dot", 37, 1, 1), ("row", 5, 1, 5), ("column", 5, 5, 1))


def _tiny_dw1x1_batch(bm, h, w):
    """conv1x1_dw takes grids of ONE round of workgroups (conv_1x1.hip dw1x1_bm: 48-pixel tiles for 64 .. 191 of them, 96-pixel
    tiles from 192 tiles on): the smallest batch of an h x w map that reaches the tile height, one more frame where that would be
    whole tiles, so that the last tile is partial"""
    pixels = {48: 64 * 48, 96: 192 * 96}[bm] + 1
    return -(-pixels // (h * w)) + 1


def tiny_cases():
    """Channel counts are the smallest each family takes (the K depths and widths of the rows of cases()); batches are 37 / 5 / 5 but
    for conv1x1_dw, whose chooser wants one round of workgroups (``_tiny_dw1x1_batch``).  Every family of cases() has the three
    rows, the two below excepted.

    Declined (family, shape) pairs, which have NO row (``TINY_DECLINED``; tests/test_footprint_host.py
    test_tiny_rows_cover_every_family_or_a_declined_entry proves each entry through plan creation):

    =========================  =========  =================================================================  ========================
    family                     shapes     the chooser line that declines                                     plan creation gives the
                                                                                                             op to
    =========================  =========  =================================================================  ========================
    conv_patch_wsp_*_8x32x128  all three  csrc/api.hip choose_conv: ``w > 128`` -- the 2-D patch kernel is   conv_igemm2_*_128x32
                                          for rows wider than any strip tile                                 (three workgroups of a
                                                                                                             128-wide tile idle)
    conv_block_fused_*_x128    all three  csrc/conv_block.hip choose_tile: ``if (tw > W || th < 4)           the pair as two launches:
                                          continue`` -- rectangles are 8 .. 24 pixels wide and at least 4    conv_dw48_k1_*, then
                                          high, so a map under 8 x 4 has no tile                             conv_dw48_k3_*
    =========================  =========  =================================================================  ========================
    """
    C = []

    def conv(name, family, opt, dtypes, cin, cout, k, s=1, res=False, **kw):
        for tag, B, h, w in TINY_SHAPES:
            C.append(_conv("tiny_%s_%s" % (name, tag), family, opt, dtypes, B, h * s, w * s, cin, cout, k, s, res=res, tiny=tag, **kw))

    conv("igemm1_128", "conv_igemm_%s_128x128", "igemm1", ALL, 64, 128, 3, res=True)
    conv("igemm1_64", "conv_igemm_%s_128x64", "igemm1", ALL, 32, 64, 3, res=True)
    conv("igemm1_32_k1", "conv_igemm_%s_128x32", "igemm1", ALL, 64, 32, 1)
    conv("igemm2_64", "conv_igemm2_%s_128x64", "igemm2_noshrink", ALL, 32, 64, 3, res=True)
    conv("igemm2_128", "conv_igemm2_%s_128x128", "igemm2_noshrink", ALL, 64, 128, 3, res=True)
    conv("igemm2_32", "conv_igemm2_%s_128x32", "igemm2_noshrink", ALL, 16, 32, 3, res=True)
    conv("igemm2_96", "conv_igemm2_%s_96x64", "igemm2_96", ALL, 128, 128, 3, res=True)
    conv("igemm3_128", "conv_igemm3_%s_128x128", "igemm3", ALL, 128, 128, 3, res=True)
    conv("igemm3_128_s2", "conv_igemm3_%s_128x128", "igemm3", ALL, 64, 128, 3, s=2)
    conv("igemm3_64", "conv_igemm3_%s_64x128", "igemm3_64", B16, 128, 128, 3, res=True)
    conv("halo192", "conv_halo_ws_%s_192x128", "halo192", ALL, 128, 128, 3, res=True, out_unit=8)
    conv("halo256", "conv_halo_ws_%s_256x128", "halo256", ALL, 128, 128, 3, res=True, out_unit=8)
    conv("halo_dw", "conv_halo_dw_%s_192x256", "halo_dw", B16, 128, 256, 3, res=True)
    conv("wres_128", "conv1x1_wres_%s_128x128", "wres", B16, 256, 128, 1)
    conv("wres_64", "conv1x1_wres_%s_128x64", "wres", B16, 128, 64, 1)
    conv("dw48_k1", "conv_dw48_k1_%s", "dw48", B16, 128, 128, 1, res=True, nkt=2)
    conv("dw48_k3", "conv_dw48_k3_%s", "dw48", B16, 128, 256, 3, res=True)
    conv("dw48_k3s2", "conv_dw48_k3s2_%s", "dw48", B16, 64, 128, 3, s=2, nkt=1)
    conv("direct", "conv_direct_%s", "default", ALL, 13, 24, 3, res=True)
    conv("direct_s2", "conv_direct_%s", "default", ALL, 21, 13, 3, s=2)
    conv("direct_f32_logits", "conv_direct_%s", "default", ALL, 21, 18, 1, out_f32=True, leaky=False)
    conv("direct_nchw_grey", "conv_direct_%s", "default", ALL, 1, 16, 3, inp="nchw")
    conv("direct_u8_k5", "conv_direct_%s", "default", ALL, 3, 16, 5, inp="u8")
    # the stems on a network input of one pixel a side (no shipped cfg: the planner takes such an input all the same)
    conv("stem_nchw", "conv_stem3x3_nchw_%s", "default", ALL, 3, 16, 3, inp="nchw")
    conv("stem_u8_f32", "conv_stem3x3_u8_%s", "default", F32, 3, 16, 3, inp="u8")
    conv("stem_mfma", "conv_stem_mfma_u8_%s", "default", B16, 3, 16, 3, inp="u8")
    conv("stem_u8_16bit_s2", "conv_stem3x3_u8_%s", "default", B16, 3, 32, 3, s=2, inp="u8")
    for bm in (48, 96):
        for tag, _, h, w in TINY_SHAPES:
            C.append(_conv("tiny_dw1x1_%d_%s" % (bm, tag), "conv1x1_dw_%%s_%dx256" % bm, "dw1x1", B16, _tiny_dw1x1_batch(bm, h, w), h, w,
                           256, 256, 1, 1, nkt=4, tiny=tag))
    for tag, B, h, w in TINY_SHAPES:
        C += [
            # the fused stem pair ends in a stride-2 conv: 2 x 2, 2 x 10 and 10 x 2 frames
            dict(id="tiny_stem_s2_" + tag, group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="default", dtypes=B16, B=B, h=2 * h, w=2 * w, tiny=tag),
            dict(id="tiny_stem_s2_phased_" + tag, group="stem_pair", family="conv_stem_s2_fused_u8_%s", opt="stem_phased", dtypes=B16, B=B, h=2 * h, w=2 * w, tiny=tag),
            dict(id="tiny_resblock_" + tag, group="resblock", family="conv_resblock_fused_%s_64_32_64", opt="default", dtypes=B16, B=B, h=h, w=w, tiny=tag),
            dict(id="tiny_head_tiled_" + tag, group="head", family="conv_head_decode_%s_64x256", opt="head_tiled", dtypes=B16, B=B, h=h, w=w, cin=192, tiny=tag),
            dict(id="tiny_head48_" + tag, group="head", family="conv_head_decode_dw_%s_48x256", opt="head48", dtypes=B16, B=B, h=h, w=w, cin=256, tiny=tag),
            dict(id="tiny_head96_" + tag, group="head", family="conv_head_decode_dw_%s_96x256", opt="head96", dtypes=B16, B=B, h=h, w=w, cin=256, tiny=tag),
        ]
        for wide, form, c in ((True, "wide", 64), (False, "elem", 13)):
            t = "_%s_%s" % (form, tag)
            C += [
                dict(_layer("tiny_maxpool_s1" + t, "maxpool_%s", "maxpool", ALL, B, h, w, c, k=2, s=1, wide=wide), tiny=tag),
                dict(_layer("tiny_maxpool_s2" + t, "maxpool_%s", "maxpool", ALL, B, 2 * h, 2 * w, c, k=2, s=2, wide=wide), tiny=tag),
                dict(_layer("tiny_maxpool_dk_s1" + t, "maxpool_dk_%s", "maxpool", ALL, B, h, w, c, k=5, s=1, wide=wide, dk=True), tiny=tag),
                dict(_layer("tiny_maxpool_dk_s2" + t, "maxpool_dk_%s", "maxpool", ALL, B, 2 * h, 2 * w, c, k=2, s=2, wide=wide, dk=True), tiny=tag),
                dict(_layer("tiny_upsample" + t, "upsample_%s", "upsample", ALL, B, h, w, c, s=2, wide=wide), tiny=tag),
                dict(_layer("tiny_add" + t, "add_%s", "add", ALL, B, h, w, c, wide=wide), tiny=tag),
                dict(_layer("tiny_add_inplace" + t, "add_%s", "add", ALL, B, h, w, c, wide=wide, alias=True), tiny=tag),
                dict(_layer("tiny_copy" + t, "copy_%s", "copy", ALL, B, h, w, c, wide=wide), tiny=tag),
            ]
        C += [
            # reorg reads the multiples of its stride that give the shape: 2 x 2, 2 x 10, 10 x 2 (flat form), 3 x 3, 3 x 15, 15 x 3
            dict(id="tiny_reorg_" + tag, group="reorg", family="reorg_%s", opt="default", dtypes=ALL, B=B, h=2 * h, w=2 * w, c=12, s=2, form3d=False, tiny=tag),
            dict(id="tiny_reorg3d_" + tag, group="reorg", family="reorg3d_%s", opt="default", dtypes=ALL, B=B, h=3 * h, w=3 * w, c=13, s=3, form3d=True, tiny=tag),
            dict(id="tiny_spp_" + tag, group="spp", family="maxpool_spp_pyramid_%s", opt="default", dtypes=ALL, B=B, h=h, w=w, c=48, dk=False, tiny=tag),
            dict(id="tiny_spp_dk_" + tag, group="spp", family="maxpool_spp_pyramid_dk_%s", opt="default", dtypes=ALL, B=B, h=h, w=w, c=48, dk=True, tiny=tag),
            # the pixel stride wider than the channels: 255 channels at 268, from channel 4
            dict(id="tiny_yolo_wide_stride_" + tag, group="yolo", family="yolo_decode_f32", opt="default", dtypes=ALL, B=B, h=h, w=w, n_anchor=3, ncls=80, ld=268, c0=4, tiny=tag),
            dict(id="tiny_yolo_few_classes_" + tag, group="yolo", family="yolo_decode_f32", opt="default", dtypes=ALL, B=B, h=h, w=w, n_anchor=2, ncls=7, ld=36, c0=4, tiny=tag),
        ]
    return C


# family -> (the row of cases() whose channels, kernel and option set force the family everywhere else, the kernels plan creation
# gives the op(s) to on each of TINY_SHAPES instead): the table of tiny_cases()
TINY_DECLINED = {
    "conv_patch_wsp_%s_8x32x128": ("patch_full", ("conv_igemm2_%s_128x32",)),
    "conv_block_fused_%s_x128": ("block_full_res", ("conv_dw48_k1_%s", "conv_dw48_k3_%s")),
}


# Families whose chooser declines every strided operand: none, every chooser takes pixel strides (the strided half of
# test_every_case_gets_the_family_it_claims is the proof).  A family that comes to need one is entered here with the chooser
# line that declines, and tests/test_footprint_host.py then gets the decline / fall-back assertions.
DENSE_ONLY = {}

# kernel names the choosers can produce that no plan of the shipped cfgs under kernel_choice_util.OPTION_SETS reaches, so
# tests/golden/kernel_choice.json does not hold them: covered here all the same
# (an entry without %s is one name: the float32 VALU stem on uint8 frames IS in the fixture, its 16-bit forms are not)
NOT_IN_FIXTURE = ("add_%s", "copy_%s", "maxpool_dk_%s", "maxpool_spp_pyramid_dk_%s", "conv_direct_%s", "reorg_%s", "reorg3d_%s",
                  "conv_stem3x3_u8_bf16", "conv_stem3x3_u8_f16")


def case_ids():
    return [(c["id"], d) for c in cases() for d in c["dtypes"]]


def case_by_id(cid):
    return next(c for c in cases() if c["id"] == cid)


def family_name(case, dtype):
    fam = case["family"]
    if "%s" not in fam:
        return fam
    return fam % TAG[dtype]


# ------------------------------------------------------------------------------------------------ ops of a case

DT_CODE = {"float32": 0, "bf16": 1, "fp16": 2}


def _act(used, name, side, dtype, pixels, c, mode, unit, v, fmt=None):
    """an activation operand; ``used``: the strides the op's other activation operands have (this one's is added)"""
    if mode == "dense":
        return Operand(name, side, fmt or dtype, pixels, c, [(0, c)])
    c0, ld = strided_ld(c, unit, v, used)
    used.add(ld)
    return Operand(name, side, fmt or dtype, pixels, ld, [(c0, c)])


def flat(name, side, fmt, n, tile=1):
    """a flat array of ``n`` elements between guards (parameters, frames, workspaces, the buffers of the other entry points)"""
    return _flat(name, side, fmt, n, tile)


def _flat(name, side, fmt, n, tile=1):
    return Operand(name, side, fmt, 1, n, [(0, n)], tile_elems=tile)


def _conv_weights(prefix, dtype, cin, cout, k, path, operands):
    """weight / scale / bias operands of one conv in the layout of kernel family ``path``; returns (cout_pad, k_ld)"""
    H = _H()
    es = ES[dtype]
    if path == H.PATH_STEM_MFMA:
        cp, k_ld, wfmt = 32, 32, dtype
    elif path == H.PATH_STEM:
        cp = k_ld = round_up(cout, 8)
        wfmt = "float32"
    else:
        cp, k_ld, wfmt = round_up(cout, 128), round_up(k * k * cin, 128 // es), dtype
    n = (k * k * cin * cp) if path == H.PATH_STEM else cp * k_ld
    operands += [_flat(prefix + "weight", "in", wfmt, n), _flat(prefix + "scale", "in", "float32", cp),
                 _flat(prefix + "bias", "in", "float32", cp)]
    return cp, k_ld


def _set_conv(op, dtype, B, h, w, cin, cout, k, s, flags, pad=None):
    H = _H()
    pad = conv_pad(k, pad)
    op.kind, op.dtype, op.flags, op.batch = H.OP_CONV, DT_CODE[dtype], flags, B
    op.in_h, op.in_w, op.in_c = h, w, cin
    op.out_h, op.out_w, op.out_c = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1, cout
    op.ksize, op.stride, op.pad = k, s, pad


def build(case, dtype, mode, opt, base=None, lead=()):
    """(ops, layout, n_frag) of ``case`` in layout ``mode`` ("dense", "strided"; the aliasing cases alias in both); ``base``: the allocation's device
    address, or None for fake addresses (the chooser only decides).  ``n_frag``: {op index: operand name} of fragment-order
    weight copies to make with y3_conv_make_fragment_weights before the run.  ``lead``: operands laid out before the case's own
    (the pad of the big-operand layouts)."""
    H = _H()
    lib = H.lib()
    es = ES[dtype]
    unit = 16 // es
    g = case["group"]
    B, h, w = case["B"], case["h"], case["w"]
    P = B * h * w
    operands, frag = [], {}
    used = set()
    zero = _flat("zero page", "in", dtype, 4096 // es)

    def finish(ops, ptrs):
        """lay out, then point the ops at their operands: ptrs = [(op index, field, operand name, slice)]"""
        for i in list(frag):
            # (the size of a fragment-order copy depends on the op's shape and flags only, not on its pointers)
            n = int(lib.y3_conv_fragment_weight_bytes(ctypes.byref(ops[i]), ctypes.byref(opt)))
            if n:
                operands.append(_flat(frag[i], "in", dtype, n // es))
            else:
                del frag[i]
        lay = Layout(list(lead) + operands + [zero])
        b = base if base is not None else (1 << 44)
        for i, field, name, k in ptrs:
            setattr(ops[i], field, lay[name].ptr(b, k))
        for i in frag:
            ops[i].d_weight_frag = lay[frag[i]].ptr(b)
        return ops, lay, frag

    if g == "conv":
        cin, cout, k, s = case["cin"], case["cout"], case["k"], case["s"]
        flags = H.F_LEAKY if case.get("leaky", True) else 0
        ops = (H.Y3Op * 1)()
        op = ops[0]
        out_f32 = bool(case.get("out_f32"))
        if out_f32:
            flags |= H.F_OUT_F32
        if case["inp"] == "u8":
            flags |= H.F_PLAN_INPUT | H.F_IN_NHWC_U8BGR
        elif case["inp"] == "nchw":
            flags |= H.F_PLAN_INPUT | H.F_IN_NCHW_F32
        if case["res"]:
            flags |= H.F_RESIDUAL
        _set_conv(op, dtype, B, h, w, cin, cout, k, s, flags, case["pad"])
        Po = B * op.out_h * op.out_w
        ptrs = []
        if case["inp"] == "act":
            x = _act(used, "input", "in", dtype, P, cin, mode, unit, 0)
            ptrs.append((0, "d_in", "input", 0))
        elif case["inp"] == "u8":
            x = _flat("input", "in", "u8", P * cin, cin)
        else:
            x = _flat("input", "in", "float32", P * cin, cin)
        operands.append(x)
        op.in_ld = x.ld if case["inp"] == "act" else cin
        ofmt = "float32" if out_f32 else dtype
        ounit = case["out_unit"] or (4 if out_f32 else unit)
        o = _act(used, "output", "out", dtype, Po, cout, mode, ounit, 1, fmt=ofmt)
        if mode == "dense" and case.get("dense_out_ld"):          # (255 head channels: the densest stride the kernels take)
            o = Operand("output", "out", ofmt, Po, case["dense_out_ld"], [(0, cout)])
        operands.append(o)
        op.out_ld = o.ld
        ptrs.append((0, "d_out", "output", 0))
        if case["res"]:
            r = _act(used, "residual", "in", dtype, Po, cout, mode, ounit, 2, fmt=ofmt)
            operands.append(r)
            op.res_ld = r.ld
            ptrs.append((0, "d_res", "residual", 0))
        # the weight layout follows the conv path, which needs provisional igemm-layout sizes to be asked
        op.cout_pad, op.k_ld = round_up(cout, 128), round_up(k * k * cin, 128 // es)
        path = lib.y3_conv_path(ctypes.byref(op))
        op.cout_pad, op.k_ld = _conv_weights("", dtype, cin, cout, k, path, operands)
        ptrs += [(0, "d_weight", "weight", 0), (0, "d_scale", "scale", 0), (0, "d_bias", "bias", 0)]
        frag[0] = "fragment weights"
        return finish(ops, ptrs) + (path,)

    if g in ("stem_pair", "resblock", "block", "head"):
        n_ops = 2
        ops = (H.Y3Op * n_ops)()
        ptrs = []
        if g == "stem_pair":
            shp = ((3, 32, 3, 1), (32, 64, 3, 2))
        elif g == "resblock":
            shp = ((64, 32, 1, 1), (32, 64, 3, 1))
        elif g == "block":
            shp = ((case["cin"], 128, 1, 1), (128, case["cout"], 3, 1))
        else:
            nattr = 85
            shp = ((case["cin"], 3 * nattr, 1, 1),)
        fl0 = H.F_LEAKY | H.F_FUSE_NEXT
        if g == "stem_pair":
            fl0 |= H.F_PLAN_INPUT | H.F_IN_NHWC_U8BGR
        if g == "head":
            fl0 = H.F_OUT_F32
        _set_conv(ops[0], dtype, B, h, w, shp[0][0], shp[0][1], shp[0][2], shp[0][3], fl0)
        if g == "stem_pair":
            operands.append(_flat("input", "in", "u8", P * 3, 3))
            ops[0].in_ld = 3
        else:
            x = _act(used, "input", "in", dtype, P, shp[0][0], mode, unit, 0)
            operands.append(x)
            ops[0].in_ld = x.ld
            ptrs.append((0, "d_in", "input", 0))
        if g == "head":
            mid = Operand("logits", "scratch", "float32", P, 256, [(0, 255)])
        else:
            mid = Operand("intermediate", "scratch", dtype, P, shp[0][1], [(0, shp[0][1])])
        operands.append(mid)
        ops[0].out_ld = mid.ld
        ptrs.append((0, "d_out", mid.name, 0))
        ops[0].cout_pad, ops[0].k_ld = round_up(shp[0][1], 128), round_up(shp[0][2] ** 2 * shp[0][0], 128 // es)
        path0 = lib.y3_conv_path(ctypes.byref(ops[0]))
        ops[0].cout_pad, ops[0].k_ld = _conv_weights("op0 ", dtype, shp[0][0], shp[0][1], shp[0][2], path0, operands)
        if g == "head":
            ops[0].cout_pad = 256
            operands[-3:] = []
            _conv_weights("op0 ", dtype, shp[0][0], 256, 1, path0, operands)
        ptrs += [(0, "d_weight", "op0 weight", 0), (0, "d_scale", "op0 scale", 0), (0, "d_bias", "op0 bias", 0)]
        if g == "head":
            yo = ops[1]
            rows = 3 * h * w
            yo.kind, yo.dtype, yo.batch = H.OP_YOLO, DT_CODE[dtype], B
            yo.in_h, yo.in_w, yo.in_c, yo.in_ld = h, w, 255, 256
            yo.out_h, yo.out_w = h, w
            yo.n_anchor, yo.n_attr = 3, 85
            for a, (aw, ah) in enumerate(((116, 90), (156, 198), (373, 326))):
                yo.anchor_w[a], yo.anchor_h[a] = float(aw), float(ah)
            yo.row_offset, yo.rows_total = 0, rows
            yo.net_w = yo.net_h = 608.0
            yo.block_idx = 1
            operands += [_flat("bbox", "out", "float32", B * rows * 4, 4), _flat("prob", "out", "float32", B * rows),
                         _flat("cls", "out", "i64", B * rows)]
            ptrs += [(1, "d_in", "logits", 0), (1, "d_bbox", "bbox", 0), (1, "d_prob", "prob", 0), (1, "d_cls", "cls", 0)]
            frag[0] = "fragment weights"
            return finish(ops, ptrs) + (path0,)
        fl1 = H.F_LEAKY | (H.F_RESIDUAL if (g == "resblock" or (g == "block" and case["res"])) else 0)
        _set_conv(ops[1], dtype, B, h, w, shp[1][0], shp[1][1], shp[1][2], shp[1][3], fl1)
        ops[1].block_idx = 1
        ops[1].in_ld = mid.ld
        ptrs.append((1, "d_in", mid.name, 0))
        Po = B * ops[1].out_h * ops[1].out_w
        # (``same_ld``: the output gets the input's stride -- big_cases(): both operands of the fused block one frame below 2^32 bytes)
        o = _act(set() if case.get("same_ld") else used, "output", "out", dtype, Po, shp[1][1], mode, unit, 0 if case.get("same_ld") else 1)
        operands.append(o)
        ops[1].out_ld = o.ld
        ptrs.append((1, "d_out", "output", 0))
        if fl1 & H.F_RESIDUAL:
            ops[1].res_ld = ops[0].in_ld
            ptrs.append((1, "d_res", "input", 0))
        ops[1].cout_pad, ops[1].k_ld = _conv_weights("op1 ", dtype, shp[1][0], shp[1][1], shp[1][2], H.PATH_IGEMM, operands)
        ptrs += [(1, "d_weight", "op1 weight", 0), (1, "d_scale", "op1 scale", 0), (1, "d_bias", "op1 bias", 0)]
        if g == "block" and opt.fuse_block >= 3:
            # the direct-weights form reads BOTH convs' weights from fragment-order copies (finish() drops a copy the library
            # does not ask for: y3_conv_fragment_weight_bytes answers for the members of such a pair)
            frag[0], frag[1] = "op0 fragment weights", "op1 fragment weights"
        return finish(ops, ptrs) + (path0,)

    if g == "layer":
        c, k, s, kind = case["c"], case["k"], case["s"], case["kind"]
        lunit = unit if case["wide"] else 1
        ops = (H.Y3Op * 1)()
        op = ops[0]
        op.kind = {"maxpool": H.OP_MAXPOOL, "upsample": H.OP_UPSAMPLE, "add": H.OP_ADD, "copy": H.OP_COPY}[kind]
        op.dtype, op.batch, op.in_h, op.in_w, op.in_c, op.out_c = DT_CODE[dtype], B, h, w, c, c
        op.ksize, op.stride = k, s
        if kind == "maxpool" and case["dk"]:
            op.flags |= H.F_POOL_DARKNET
            op.pad = k - 1
            op.out_h, op.out_w = (h + op.pad - k) // s + 1, (w + op.pad - k) // s + 1
        elif kind == "maxpool":
            op.out_h, op.out_w = (h, w) if s == 1 else ((h - k) // s + 1, (w - k) // s + 1)
        elif kind == "upsample":
            op.out_h, op.out_w = h * s, w * s
        else:
            op.out_h, op.out_w = h, w
        Po = B * op.out_h * op.out_w
        ptrs = []
        if case["alias"]:
            # the in-place add: d_out == d_in (the plan's shortcut into the buffer of one of its operands)
            x = _act(used, "input/output", "inout", dtype, P, c, mode if mode == "dense" else "strided", lunit, 0)
            operands.append(x)
            op.in_ld = op.out_ld = x.ld
            ptrs += [(0, "d_in", x.name, 0), (0, "d_out", x.name, 0)]
        else:
            x = _act(used, "input", "in", dtype, P, c, mode, lunit, 0)
            o = _act(used, "output", "out", dtype, Po, c, mode, lunit, 1)
            operands += [x, o]
            op.in_ld, op.out_ld = x.ld, o.ld
            ptrs += [(0, "d_in", "input", 0), (0, "d_out", "output", 0)]
        if kind == "add":
            r = _act(used, "residual", "in", dtype, P, c, mode, lunit, 2)
            operands.append(r)
            op.res_ld = r.ld
            ptrs.append((0, "d_res", "residual", 0))
        return finish(ops, ptrs) + (None,)

    if g == "reorg":
        c, st = case["c"], case["s"]
        co = c * st * st
        ops = (H.Y3Op * 1)()
        op = ops[0]
        op.kind, op.dtype, op.batch, op.stride = H.OP_REORG, DT_CODE[dtype], B, st
        op.flags = H.F_REORG_3D if case["form3d"] else 0
        op.in_h, op.in_w, op.in_c, op.out_h, op.out_w, op.out_c = h, w, c, h // st, w // st, co
        # (an element-wise kernel: strides are multiples of nothing, as for the element-wise layer forms)
        x = _act(used, "input", "in", dtype, P, c, mode, 1, 0)
        o = _act(used, "output", "out", dtype, B * op.out_h * op.out_w, co, mode, 1, 1)
        operands += [x, o]
        op.in_ld, op.out_ld = x.ld, o.ld
        return finish(ops, [(0, "d_in", "input", 0), (0, "d_out", "output", 0)]) + (None,)

    if g == "spp":
        c = case["c"]
        ops = (H.Y3Op * 3)()
        x = _act(used, "input", "in", dtype, P, c, mode, unit, 0)
        # three output slices of ONE concat buffer (the route the pyramid feeds), margins left, between and right
        if mode == "dense":
            cat = Operand("concat", "out", dtype, P, 3 * c, [(0, c), (c, c), (2 * c, c)])
        else:
            ld = 3 * c + 5 * unit
            ld += unit if (ld // unit) % 2 == 0 else 0
            cat = Operand("concat", "out", dtype, P, ld, [(unit, c), (c + 2 * unit, c), (2 * c + 3 * unit, c)])
        operands += [x, cat]
        ptrs = []
        for i, k in enumerate((5, 9, 13)):
            op = ops[i]
            op.kind, op.dtype, op.batch = H.OP_MAXPOOL, DT_CODE[dtype], B
            op.in_h = op.out_h = h
            op.in_w = op.out_w = w
            op.in_c = op.out_c = c
            op.in_ld, op.out_ld, op.ksize, op.stride, op.block_idx = x.ld, cat.ld, k, 1, i
            if case["dk"]:
                op.flags |= H.F_POOL_DARKNET
                op.pad = k - 1
            ptrs += [(i, "d_in", "input", 0), (i, "d_out", "concat", i)]
        return finish(ops, ptrs) + (None,)

    if g == "yolo":
        na, nattr = case["n_anchor"], case["ncls"] + 5
        c = na * nattr
        ops = (H.Y3Op * 1)()
        yo = ops[0]
        rows = na * h * w
        # this head's rows sit at row_offset > 0 of a longer output (as the second head of a network's do)
        off, total = (0, rows) if mode == "dense" else (37, rows + 37 + 53)
        x = Operand("input", "in", "float32", P, round_up(c, 4) if mode == "dense" else case["ld"], [(0 if mode == "dense" else case["c0"], c)])
        yo.kind, yo.dtype, yo.batch = H.OP_YOLO, DT_CODE[dtype], B
        yo.in_h, yo.in_w, yo.in_c, yo.in_ld = h, w, c, x.ld
        yo.out_h, yo.out_w = h, w
        yo.n_anchor, yo.n_attr = na, nattr
        for a in range(na):
            yo.anchor_w[a], yo.anchor_h[a] = 30.0 + 40 * a, 60.0 + 25 * a
        yo.row_offset, yo.rows_total = off, total
        yo.net_w, yo.net_h = 416.0, 352.0
        # outputs: (B, rows_total, 4 | 1 | 1); as operands: B "pixels" of rows_total * n elements, the op's rows one slice
        operands += [x, Operand("bbox", "out", "float32", B, total * 4, [(off * 4, rows * 4)], tile_elems=4),
                     Operand("prob", "out", "float32", B, total, [(off, rows)], tile_elems=1),
                     Operand("cls", "out", "i64", B, total, [(off, rows)], tile_elems=1)]
        lay = Layout(list(lead) + operands + [zero])
        b = base if base is not None else (1 << 44)
        yo.d_in = lay["input"].ptr(b)
        # d_bbox / d_prob / d_cls are the bases of the WHOLE outputs: the op adds row_offset itself
        yo.d_bbox, yo.d_prob, yo.d_cls = b + lay["bbox"].body, b + lay["prob"].body, b + lay["cls"].body
        return ops, lay, {}, None
    raise AssertionError(g)


def chosen(case, dtype, mode, base=None):
    """kernel names of the case's ops under its options (plan creation only decides when the addresses are fake: every conv
    that reads fragment-order weights has a d_weight_frag)"""
    H = _H()
    lib = H.lib()
    opt = H.options(**_opts()[case["opt"]])
    ops, lay, frag, _ = build(case, dtype, mode, opt, base)
    handle = ctypes.c_void_p()
    zero = lay["zero page"].ptr(base if base is not None else (1 << 44))
    H.check(lib.y3_plan_create_ex(ops, len(ops), zero, ctypes.byref(opt), ctypes.byref(handle)))
    try:
        return [lib.y3_plan_op_kernel(handle, i).decode() for i in range(len(ops))], lay
    finally:
        lib.y3_plan_destroy(handle)


# ------------------------------------------------------------------------------------------------ operands past 4 GiB
# tests/test_big_operands_host.py (no GPU) and tests/test_gpu_big_operands.py: every kernel family on operands whose byte
# offsets pass 2^32, and the refusal of ops of 2^31 pixels.  The rows are NOT census cases: cases() stays as it is.

SPAN = 1 << 32
PAD_BYTES = 1 << 32            # in front of the first operand: a 32-bit wrap or a sign-extended offset lands inside the allocation
MAX_PIXELS = (1 << 31) - 1 - TILE_PIXELS     # csrc/api.hip check_size: both pixel counts of every op, one widest tile below 2^31
MAX_THREADS = ((1 << 32) - 1) // 256 * 256   # csrc/common.h kY3MaxThreads: grid x block of any one launch (api.hip check_launch)

# One row per kernel family, from the family's ragged row of cases() (same channels, kernel, stride, shortcut form, option set
# and map; the batch comes from big_batch).  Families without a row called "ragged" give the row named here: the direct
# fallback its stride-2 row with odd channel counts on both sides, the layer kernels their wide (16-byte vector) rows, the
# 16-bit VALU stem its 48-channel row.  Maps are odd x odd, so a frame's byte size divides neither 2^31 nor 2^32 and a wrapped
# address lands mid-frame -- but where the op itself demands even sides: the stride-2 conv_dw48 (dw48_shape: in_h % 2 == 0)
# and the flat reorg at stride 2 keep their even maps (38 x 26, 14 x 10), whose OUTPUT maps are odd (19 x 13, 7 x 5) and whose frame
# sizes have odd factors too; the stride-2 max-pool is moved from 26 x 22 to 27 x 23.
_BIG_ROWS = (
    ("igemm1_128_ragged", {}), ("igemm1_64_ragged_res", {}), ("igemm1_32_ragged", {}),
    ("igemm2_128_ragged", {}), ("igemm2_64_ragged_res", {}), ("igemm2_32_ragged", {}), ("igemm2_96_ragged", {}),
    ("igemm3_128_ragged", {}), ("igemm3_64_ragged", {}),
    ("halo256_ragged", {}), ("halo_dw_ragged", {}), ("patch_ragged", {}),
    ("wres_128_ragged", {}), ("wres_64_ragged", {}),
    ("dw48_k1_ragged", {}), ("dw48_k3_ragged", {}), ("dw48_k3s2_ragged", {}),
    ("stem_nchw_ragged", {}), ("stem_u8_f32_ragged", {}), ("stem_u8_16bit_c48", {}), ("stem_mfma_ragged", {}),
    ("direct_odd_both_s2", {}),
    ("stem_s2_ragged", {}), ("resblock_ragged", {}),
    # the fused block keeps 32-bit byte offsets and diverts at 2^32 bytes (conv_block.hip y3_choose_conv_block_fused): its row has
    # x and z at ONE stride, both within one frame below 2^32 bytes
    ("block_ragged_res", {"same_ld": True}),
    ("head_tiled_ragged", {}), ("head48_ragged", {}), ("head96_ragged", {}),
    ("maxpool_s2_wide", {"h": 27, "w": 23}), ("maxpool_dk_s2_wide", {}), ("upsample_wide", {}), ("add_wide", {}), ("copy_wide", {}),
    ("reorg_ragged", {}), ("reorg3d_ragged", {}), ("spp_ragged", {}), ("spp_dk_ragged", {}), ("yolo_wide_stride", {}),
)

# Families whose own chooser rule bounds the grid, so that no operand of theirs comes near 2^31 bytes: no GPU row, the host test
# proves the bound on the row named here.  conv1x1_dw: one round of workgroups (conv_1x1.hip dw1x1_bm: at most one 96- or
# 48-pixel tile per CU).  conv_halo_ws 192 x 128: the 192-pixel tile is taken only while it saves rounds of workgroups
# (conv_halo.hip halo_tile_fragments: cost = rounds x time per tile, and a 192-pixel tile takes at least 0.8 of a 256-pixel
# tile's time, so from about ten rounds on -- rounds(192) / rounds(256) -> 4 / 3 -- the 256-pixel tile always wins).
# (The stride-2 conv_dw48 and the 256-pixel and direct-weights halo kernels are NOT bounded: row width, LDS and even sides limit
# the map, nothing limits the batch under the option sets that force them.  They have rows above.)
BIG_BOUNDED = {"conv1x1_dw_%s_96x256": "dw1x1_96_ragged", "conv1x1_dw_%s_48x256": "dw1x1_48_ragged",
               "conv_halo_ws_%s_192x128": "halo192_ragged"}


def big_cases():
    rows = []
    for src, over in _BIG_ROWS:
        c = dict(case_by_id(src))
        c.update(over)
        c["src"] = src
        c["dtypes"] = tuple(d for d in c["dtypes"] if d != "fp16")     # (fp16 shares the ES = 2 address code with bf16)
        rows.append(c)
    return rows


def big_case_ids():
    return [(c["id"], d) for c in big_cases() for d in c["dtypes"]]


def big_row(cid):
    return next(c for c in big_cases() if c["id"] == cid)


def _is_frames_input(case):
    """the op reads the network input (uint8 frames / float NCHW): a dense tensor a few bytes per pixel"""
    return case["group"] == "stem_pair" or (case["group"] == "conv" and case["inp"] != "act")


def span_operands(case, lay):
    """the activation operands of ``lay`` that big_batch holds past 2^32 bytes: every one, but the network-input forms (there
    the output), and the input alone of the ops whose outputs are detections (the decode, the fused heads)"""
    g = case["group"]
    if g in ("yolo", "head"):
        return [lay["input"]]
    names = ("input", "output", "residual", "concat", "input/output")
    return [o for o in lay.operands if o.name in names and not (o.name == "input" and _is_frames_input(case))]


def frame_pixels(case, dtype):
    """the largest pixel count per frame among the inputs and outputs of the case's ops"""
    ops, _, _, _ = build(dict(case, B=3), dtype, "strided", _H().options(**_opts()[case["opt"]]))
    return max(max(op.in_h * op.in_w, op.out_h * op.out_w) for op in ops)


def big_batch(case, dtype):
    """frames that put every operand of span_operands more than 2^32 bytes plus one frame long (the fused block: the largest batch
    that keeps x and z below 2^32 bytes)"""
    _, lay, _, _ = build(dict(case, B=3), dtype, "strided", _H().options(**_opts()[case["opt"]]))
    frames = [o.body_bytes // 3 for o in span_operands(case, lay)]
    assert frames and all(f * 3 == o.body_bytes for f, o in zip(frames, span_operands(case, lay)))
    if case["group"] == "block":
        assert len(set(frames)) == 1, frames
        return (SPAN - 1) // frames[0]
    return max((SPAN + f) // f + 1 for f in frames)


def big_case(row, dtype):
    return dict(row, B=big_batch(row, dtype))


def pad_operand():
    return Operand("pad", "pad", "u8", 1, PAD_BYTES, [(0, PAD_BYTES)], tile_elems=1)


# ---- the checker (torch, any device; nothing here allocates a temporary of the allocation's size)

CHUNK = 1 << 28


def _first_difference(before, after, lo, hi, chunk=CHUNK):
    """None, or the (first 100000) offsets in [lo, hi) where the two byte tensors differ"""
    for a in range(lo, hi, chunk):
        b = min(hi, a + chunk)
        if not torch.equal(before[a:b], after[a:b]):
            return (torch.nonzero(before[a:b] != after[a:b]).flatten()[:100000] + a).cpu().numpy()
    return None


def region_violations(before, after, layout, chunk=CHUNK):
    """footprint_violations region by region: the pad, every guard, the body of every read-only operand and the margins of
    every written one must be byte for byte what they were.  None, or describe()'s message for the first region that is not."""
    for o in layout.operands:
        regions = [(o.front, o.body), (o.body + o.body_bytes, o.end)]
        if o.side in ("in", "pad"):
            regions.insert(1, (o.body, o.body + o.body_bytes))
        for lo, hi in regions:
            offs = _first_difference(before, after, lo, hi, chunk)
            if offs is not None:
                return describe(offs, layout)
        if o.side not in ("out", "inout"):
            continue
        row = o.ld * o.es
        cols, at = [], 0                                   # byte columns of a pixel outside every slice
        for c0, c in o.slices:
            if c0 * o.es > at:
                cols.append((at, c0 * o.es))
            at = (c0 + c) * o.es
        if at < row:
            cols.append((at, row))
        step = max(1, chunk // row)
        for p0 in range(0, o.pixels if cols else 0, step):
            p1 = min(o.pixels, p0 + step)
            bb = before[o.body + p0 * row:o.body + p1 * row].view(-1, row)
            ab = after[o.body + p0 * row:o.body + p1 * row].view(-1, row)
            for lo, hi in cols:
                if not torch.equal(bb[:, lo:hi], ab[:, lo:hi]):
                    ix = torch.nonzero(bb[:, lo:hi] != ab[:, lo:hi])[:100000]
                    offs = (o.body + (ix[:, 0] + p0) * row + ix[:, 1] + lo).cpu().numpy()
                    return describe(offs, layout)
    return None


def _frames(t, n_frames):
    assert t.numel() % n_frames == 0, (tuple(t.shape), n_frames)
    return t.reshape(n_frames, -1)


def frame_violations(t, n_frames, base=None, chunk=CHUNK):
    """``t``: one written slice as bytes (read_slice's (pixels, bytes)); frame b is its b-th of ``n_frames`` equal parts.  None, or a
    message naming the first frame that is not, byte for byte, frame b % 3 of ``base`` ((3, frame bytes); default: the tensor's
    own first three frames) -- position independence: the inputs' frame b is their frame b % 3."""
    f = _frames(t, n_frames)
    base = f[:3] if base is None else base.to(f.device).reshape(3, -1)
    assert base.shape[1] == f.shape[1], (tuple(base.shape), tuple(f.shape))
    step = max(3, chunk // f.shape[1] // 3 * 3)
    for f0 in range(0, n_frames, step):
        x = f[f0:f0 + step]
        want = base.repeat(x.shape[0] // 3 + 1, 1)[:x.shape[0]]
        if torch.equal(x, want):
            continue
        bad = torch.nonzero((x != want).any(1)).flatten()
        b = int(bad[0])
        where = torch.nonzero(x[b] != want[b]).flatten()
        return "frame %d differs from frame %d (%d %% 3) in %d of %d bytes, first at byte %d of the frame; %d frames of %d .. %d differ" % (
            f0 + b, (f0 + b) % 3, f0 + b, where.numel(), f.shape[1], int(where[0]), bad.numel(), f0, f0 + x.shape[0] - 1)
    return None


def nan_violations(t, n_frames, fmt, chunk=CHUNK):
    """None, or a message naming the first frame of the slice ``t`` (bytes) that holds a NaN of storage type ``fmt``: an element
    left at its prefill, or computed from a byte the op does not own"""
    if fmt not in NAN_BYTES:
        return None
    f = _frames(t, n_frames)
    step = max(1, chunk // f.shape[1])
    for f0 in range(0, n_frames, step):
        nan = torch.isnan(f[f0:f0 + step].contiguous().view(TORCH_DT[fmt]))
        if bool(nan.any()):
            b = int(torch.nonzero(nan.any(1)).flatten()[0])
            return "frame %d holds NaN: %d of its %d elements never written or poisoned" % (f0 + b, int(nan[b].sum()), nan.shape[1])
    return None


def block_tile(H, W):
    """(tile width, tile height) of the fused bottleneck block on an H x W map, restated from csrc/conv_block.hip choose_tile: widths
    8 .. 24, the tallest rectangle of at most 384 pixels whose one-pixel border fits 448 halo rows, no taller than its number of tile
    rows needs; of those the one with the fewest tiles, the narrowest first.  The chooser ranks by ROUNDS of workgroups over the CU
    count before it ranks by tiles; rounds never fall as tiles rise, so the count cannot change the pick (it enters the 70 % rule of
    fuse_block = 1 only): tests/test_cu_count_host.py holds the library to that."""
    cd = lambda a, b: -(-a // b)
    best = None
    for tw in range(8, 25):
        th = 384 // tw
        while th > 0 and (tw + 2) * (th + 2) > 448:
            th -= 1
        th = min(th, H)
        if tw > W or th < 4:
            continue
        rows = cd(H, th)
        th = cd(H, rows)
        tiles = cd(W, tw) * rows
        if best is None or tiles < best[0]:
            best = (tiles, tw, th)
    return None if best is None else best[1:]


def persistent_grid(case, op, B, n_cu):
    """workgroups of the four families with a persistent grid on a device of ``n_cu`` CUs, and of the fused block (one workgroup a
    rectangle), restated from the op's fields (csrc/conv_1x1.hip wres_geom, csrc/conv_halo.hip patch_geom, csrc/conv_fused.hip
    fused_geom, csrc/conv_block.hip block_geom); None for another family"""
    cd = lambda a, b: -(-a // b)
    fam = case["family"].split("_%s")[0]
    if fam == "conv1x1_wres":
        # a whole number of workgroups per channel tile, about one per CU, at least one per channel tile, at most one per tile
        bn = int(case["family"].rsplit("x", 1)[1])
        n_tiles, m_tiles = op.out_c // bn, cd(B * op.in_h * op.in_w, 128)
        per_tile = max(1, n_cu // n_tiles)
        return n_tiles * min(per_tile, m_tiles)
    if fam == "conv_patch_wsp":
        return min(n_cu, cd(op.in_w, 32) * cd(op.in_h, 8) * B * (op.out_c // 128))
    if fam == "conv_stem_s2_fused_u8":
        # the OUTPUT map of the pair's stride-2 conv in tiles of 16 x 8 (the pipelined kernel) or 16 x 16 (phase by phase)
        ho, wo = (op.in_h + 2 - 3) // 2 + 1, (op.in_w + 2 - 3) // 2 + 1
        return min(n_cu, cd(wo, 16) * cd(ho, 16 if case["opt"] == "stem_phased" else 8) * B)
    if fam == "conv_resblock_fused":
        return min(n_cu, cd(op.in_w, 16) * cd(op.in_h, 16) * B)
    if fam == "conv_block_fused":
        tw, th = block_tile(op.in_h, op.in_w)
        return cd(op.in_w, tw) * cd(op.in_h, th) * B      # (one workgroup a rectangle: no persistent grid, the count picks nothing)
    return None


PERSISTENT_BLOCK = {"conv1x1_wres": 512, "conv_patch_wsp": 768, "conv_stem_s2_fused_u8": 1024, "conv_resblock_fused": 512,
                    "conv_block_fused": 512}


def launch_threads(case, dtype, B, n_cu=None):
    """grid x block of the launch of ``case`` at batch ``B``, restated from the launchers of csrc/*.hip.  Five families give None
    without ``n_cu`` -- four persistent grids of about one workgroup per CU, and the fused block, which its 2^32-byte rule bounds first
    --; with it, their launch on a device of that many CUs (persistent_grid).  A launch holds fewer than 2^32 threads: MAX_THREADS
    (csrc/api.hip check_launch)."""
    H = _H()
    ops, _, _, _ = build(dict(case, B=3), dtype, "strided", H.options(**_opts()[case["opt"]]))
    op = ops[0]
    cd = lambda a, b: -(-a // b)
    P, Po, es = B * op.in_h * op.in_w, B * op.out_h * op.out_w, ES[dtype]
    fam, cout = case["family"], op.out_c
    if n_cu is not None and fam.split("_%s")[0] in PERSISTENT_BLOCK:
        block = PERSISTENT_BLOCK[fam.split("_%s")[0]]
        if fam.startswith("conv_stem_s2") and case["opt"] == "stem_phased":
            block = 512
        return persistent_grid(case, op, B, n_cu) * block
    if fam.startswith("conv_igemm"):                    # conv_igemm.hip launch_cfg / 2 / 3: 256 threads a tile, version 3 512
        bm, bn = (int(x) for x in fam.rsplit("_", 1)[1].split("x"))
        return cd(Po, bm) * cd(cout, bn) * (512 if fam.startswith("conv_igemm3") else 256)
    if fam.startswith("conv_halo_ws"):
        return cd(P, int(fam.rsplit("_", 1)[1].split("x")[0])) * (cout // 128) * 768
    if fam.startswith("conv_halo_dw"):
        return cd(P, 192) * (cout // 256) * 512
    if fam.startswith("conv1x1_dw"):
        return cd(P, int(fam.rsplit("_", 1)[1].split("x")[0])) * (cout // 256) * 512
    if fam.startswith("conv_dw48"):                     # under SMALL_DW_ALWAYS: the widest workgroup the channel count allows
        nw = next(n for n in (8, 4, 2, 1) if cout % (32 * n) == 0)
        return cd(Po, 48) * (cout // (32 * nw)) * 512
    if fam.startswith("conv_stem3x3"):
        return cd(Po, 256) * 256
    if fam.startswith("conv_stem_mfma"):
        return cd(op.in_w, 32) * cd(op.in_h, 8) * B * 256
    if fam.startswith("conv_direct"):
        return cd(Po * cout, 256) * 256
    if fam.startswith("conv_head_decode_dw"):
        return cd(P, int(fam.rsplit("_", 1)[1].split("x")[0])) * 512
    if fam.startswith("conv_head_decode"):
        return cd(P, 64) * 256
    if case["group"] == "layer":
        return cd(Po * (op.in_c // (16 // es) if case["wide"] else op.in_c), 256) * 256
    if case["group"] == "reorg":
        return cd(Po * cout, 256) * 256
    if case["group"] == "spp":
        return B * (op.in_c * es // 32) * 256
    if case["group"] == "yolo":
        return cd(P, 32) * (256 if dtype == "float32" else 384)
    assert fam.split("_%s")[0] in ("conv_patch_wsp", "conv1x1_wres", "conv_stem_s2_fused_u8", "conv_resblock_fused", "conv_block_fused"), fam
    return None


def largest_batch(case, dtype):
    """(the largest batch plan creation takes for ``case``, what refuses the next one: "pixels" or "threads")"""
    fp = frame_pixels(case, dtype)
    ok = MAX_PIXELS // fp
    if (launch_threads(case, dtype, ok) or 0) <= MAX_THREADS:
        return ok, "pixels"
    lo, hi = 1, ok                                      # threads grow with the batch
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if launch_threads(case, dtype, mid) <= MAX_THREADS else (lo, mid - 1)
    return lo, "threads"
