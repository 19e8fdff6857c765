"""A CPU interpreter of ``yolov3.plan.build_plan(...)["ops"]`` -- TEST INFRASTRUCTURE (tests/test_plan_graph_host.py).

``run`` executes the ops one after the other on ONE byte arena of ``arena_bytes``, every byte pre-filled with 0xFF (a NaN in
float32, bf16 and fp16).  Every read and write goes through the op's ``Tensor``: byte ``offsets[buf] + off * es`` of the arena,
pixel stride ``ld`` elements, ``c`` channels, ``es`` = 4 where ``Tensor.f32`` is set and the plan's element size otherwise.  So the
planner's offsets, slices, aliases, copies and liveness are what the data flows through; a value that the plan never routes to its
reader, or frees too early, arrives as NaN or as another tensor's bytes, and an op whose output shares a byte with one of its
operands is an error of its own (``check_no_overlap``).  The arithmetic of each op kind is the oracle's and
knows nothing of the graph: ``oracle.darknet_oracle.conv_block`` / ``maxpool`` / ``upsample``, a plain add rounded once, a
slice copy, the reorg loops of tests/yolov2_restate.py, 16-bit storage rounding by ``storage_round`` (fp16 on the CPU).

Two modes:

* ``"literal"``: every op writes its output.
* ``"as_fused"``: what the executor may skip is skipped.  The output of a conv marked ``fuse_next`` is handed to the next op in
  memory and not written; in the 16-bit modes a head conv's float32 logits are handed to the decode directly after it and
  not written (the fused head kernels; float32 has none).  Any other reader meets the NaN fill.

What the device code does regardless of the ``Tensor`` is stated once each: the decode loads 4-byte elements
(``yolo_decode_kernel``), whatever its input's ``f32`` says, and a shortcut operand is addressed with the plan's element size
(``plan_ops.fill_ops``: ``d_res``).

``reference_blocks`` is the other side: a forward of the same cfg by block index, which knows nothing of the planner and calls
the same arithmetic functions on the same values, so the comparison is bit for bit.
"""
import os

import torch

from oracle import darknet_oracle as orc
from oracle import ref_io
from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.synthdata import synth_frames

import yolov2_restate as R2
import yolov4_restate as R4
from golden_util import GOLDEN

GRAPH_CFGS = ("graph_shortcuts", "graph_concat", "graph_routes", "graph_pools", "graph_heads")
F32_ONLY = ("graph_heads",)          # refused when elem_size != 4 (plan.check_head_readers)
BATCH, HEIGHT, WIDTH = 2, 32, 48
EMULATE = {4: None, 2: "f16"}
_cases = {}


def cfg_path(name):
    return os.path.join(GOLDEN, "cfg", name + ".cfg")


def abs_routes(blocks):
    for i, blk in enumerate(blocks):
        if blk["type"] == "route":
            blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
    return blocks


def synth_case(path, height, width, batch=BATCH, seed=0):
    """(blocks with absolute routes, net_info, params, frames uint8 (B,H,W,3), x float32 (B,3,H,W)) of one cfg: procedural
    parameters as tests/test_gpu_odd_cfg.py makes them, procedural frames."""
    blocks, net_info = parse_config(path)
    calib = [[0.0, 1.0]] * sum(1 for b in blocks if b["type"] == "convolutional" and b.get("batch_normalize"))
    params = W.synth_params(blocks, net_info, seed=seed, obj_bias=-2.0, calib=calib)
    abs_routes(blocks)
    frames = synth_frames(17, batch, height, width)
    x = torch.from_numpy(orc.frames_to_input(list(frames)))
    return dict(path=path, blocks=blocks, net_info=net_info, params=params, frames=frames, x=x)


def graph_case(name):
    """one of GRAPH_CFGS at batch 2, 32 x 48; made once and left unchanged"""
    if name not in _cases:
        _cases[name] = synth_case(cfg_path(name), HEIGHT, WIDTH)
    return _cases[name]


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: a forward by block index
# ---------------------------------------------------------------------------------------------------------------------------

def reference_blocks(path, params, x, emulate=None, accumulate="f32"):
    """{block: float32 tensor} of every block of the cfg at ``path`` (read with ``oracle.ref_io``).  The walk of
    ``OracleDarknet.forward`` / ``yolov4_restate.Restatement.forward``, with the grouped route of the latter and the reorg of
    ``yolov2_restate``; ``emulate``: None or "f16" / "bf16" storage at ``Restatement.rounding_points``; ``accumulate="f64"``: every
    conv summed in float64 (the GPU tests' float32 reference).  A [yolo] / [region] block's entry is its input, the logits."""
    net = R4.Restatement(path, params)
    rnd = orc.storage_round(emulate)
    rounds = net.rounding_points()
    for i, blk in enumerate(net.blocks[1:]):
        if blk["type"] == "region":
            rounds[i] = False                  # float32 logits in front of a [region] as well (yolov2_restate.rounding_points)
    outs = []
    with torch.no_grad():
        x = rnd(x) if rnd is not None else x
        for i, blk in enumerate(net.blocks):
            kind = blk["type"]
            if kind == "convolutional":
                assert blk["activation"] in ("leaky", "linear"), (i, blk["activation"])
                x = orc.conv_block(x, params[net.slot[i]], blk["stride"], (blk["size"] - 1) // 2 if "pad" in blk else 0,
                                   blk["activation"] == "leaky", round_weights=emulate, accumulate=accumulate)
                if rnd is not None and rounds[i]:
                    x = rnd(x)
            elif kind == "maxpool":
                x = orc.maxpool(x, blk["size"], blk["stride"])
            elif kind == "upsample":
                x = orc.upsample(x, blk["stride"])
            elif kind == "route":
                x = R4.route(outs, blk)
            elif kind == "shortcut":
                x = outs[i - 1] + outs[i + blk["from"]]
                if rnd is not None:
                    x = rnd(x)
            elif kind in ("reorg", "reorg3d"):
                x = R2.reorg_block(x.contiguous(), blk)
            elif kind not in ("yolo", "region"):
                raise AssertionError("block %d: %s" % (i, kind))
            outs.append(x)
    return dict(enumerate(outs))


def plain_oracle_can_walk(path):
    blocks, _ = ref_io.read_cfg(path)
    return all(b["type"] in ("convolutional", "maxpool", "upsample", "route", "shortcut", "yolo") and
               int(b.get("groups", 1)) == 1 for b in blocks)


# ---------------------------------------------------------------------------------------------------------------------------
# the interpreter
# ---------------------------------------------------------------------------------------------------------------------------

class PlanError(AssertionError):
    pass


def bit_equal(a, b):
    """same shape and the same bits (a NaN equals only the same NaN; -0.0 differs from 0.0)"""
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int32), b.view(torch.int32))


class Interp(object):
    def __init__(self, plan, params, x, es, mode):
        assert mode in ("literal", "as_fused") and es in (2, 4)
        self.plan, self.params, self.es, self.mode = plan, params, es, mode
        self.batch = x.shape[0]
        self.emulate = EMULATE[es]
        self.rnd = orc.storage_round(self.emulate)
        self.x = self.rnd(x) if self.rnd is not None else x
        self.arena = torch.full((plan["arena_bytes"],), 0xFF, dtype=torch.uint8)
        self.handed = None          # (Tensor it stands for, value) kept on chip between two ops of a fused group

    # -- memory ---------------------------------------------------------------------------------------------------------------
    def _view(self, t, es):
        """the (B, h, w, c) strided view of Tensor ``t`` with ``es``-byte elements; inside its own buffer or an error"""
        dt = torch.float32 if es == 4 else torch.float16
        lo = self.plan["offsets"][t.buf] + t.off * es
        span = (self.batch * t.h * t.w - 1) * t.ld + t.c
        end = self.plan["offsets"][t.buf] + self.plan["buffers"][t.buf]
        if t.off + t.c > t.ld or lo % es or lo + span * es > end or end > self.plan["arena_bytes"]:
            raise PlanError("%r read with %d-byte elements leaves its buffer (%d bytes at %d)" % (
                t, es, self.plan["buffers"][t.buf], self.plan["offsets"][t.buf]))
        flat = self.arena[lo:lo + span * es].view(dt)
        return flat.as_strided((self.batch, t.h, t.w, t.c), (t.h * t.w * t.ld, t.w * t.ld, t.ld, 1))

    def _bytes(self, mask, t, es):
        """the bytes of Tensor ``t`` in a byte mask of the arena, as (pixels, c * es)"""
        lo = self.plan["offsets"][t.buf] + t.off * es
        return mask.as_strided((self.batch * t.h * t.w, t.c * es), (t.ld * es, 1), lo)

    def check_no_overlap(self, n, op):
        """An op's output must share no byte with its operands: a kernel's workgroups run in no order, so such a plan is a
        race on the device whatever this interpreter, which reads before it writes, would compute."""
        out = op.get("out")
        if out is None:
            return
        self._view(out, 4 if out.f32 else self.es)
        mask = torch.zeros(self.plan["arena_bytes"], dtype=torch.bool)
        self._bytes(mask, out, 4 if out.f32 else self.es).fill_(True)
        for key, es in (("inp", None), ("res", self.es)):
            t = op.get(key)
            if t is None or t.buf == "input" or (self.handed is not None and self.handed[0] is t):
                continue
            es = es or (4 if t.f32 else self.es)
            self._view(t, es)
            if bool(self._bytes(mask, t, es).any()):
                raise PlanError("op %d (%s, block %d): its output %r shares arena bytes with its operand %r" % (
                    n, op["kind"], op["block"], out, t))

    def read(self, t, es=None):
        """(B, c, h, w) float32 of a Tensor"""
        if t.buf == "input":
            return self.x
        if self.handed is not None and self.handed[0] is t:
            return self.handed[1]
        return self._view(t, es or (4 if t.f32 else self.es)).permute(0, 3, 1, 2).float().contiguous()

    def write(self, t, y, keep_on_chip=False):
        if not t.f32 and self.rnd is not None:
            y = self.rnd(y)
        assert tuple(y.shape) == (self.batch, t.c, t.h, t.w), (t, tuple(y.shape))
        if keep_on_chip:
            self.handed = (t, y)
        else:
            self._view(t, 4 if t.f32 else self.es).copy_(y.permute(0, 2, 3, 1))
        return y

    # -- ops --------------------------------------------------------------------------------------------------------------------
    def run(self, on_block=None):
        """Execute the plan.  ``on_block(i, value)`` is called for every block as soon as its value exists: before the first op
        of a later block, read back through ``tensor_of[i]`` (or the value handed on chip); a head block's value is what its
        decode read.  Returns {head block: logits}."""
        ops, tensor_of = self.plan["ops"], self.plan["tensor_of"]
        heads, on_chip = {}, {}
        nxt = 0

        def flush(upto):
            nonlocal nxt
            for j in range(nxt, upto):
                if on_block is None or tensor_of[j] is None:
                    continue                                  # (a conv fused into its shortcut: never a tensor)
                if j in heads:
                    on_block(j, heads[j])
                elif j in on_chip:
                    on_block(j, on_chip[j])
                else:
                    on_block(j, self.read(tensor_of[j]))
            nxt = max(nxt, upto)

        for n, op in enumerate(ops):
            flush(op["block"])
            kind = op["kind"]
            produced = None
            self.check_no_overlap(n, op)
            if kind == "conv":
                y = orc.conv_block(self.read(op["inp"]), self.params[op["slot"]], op["stride"], op["pad"], op["leaky"],
                                   round_weights=self.emulate)
                assert not op.get("mish") and not op.get("logistic")
                if op["res"] is not None:
                    y = y + self.read(op["res"], self.es)     # d_res: the plan's element size, whatever res.f32 says
                nxt_op = ops[n + 1] if n + 1 < len(ops) else {}
                skip = self.mode == "as_fused" and (
                    op["fuse_next"] or
                    (self.es != 4 and op["out"].f32 and nxt_op.get("kind") == "yolo" and nxt_op["inp"] is op["out"]))
                y = self.write(op["out"], y, keep_on_chip=skip)
                if skip:
                    produced = self.handed
                    on_chip[op["block"] if op["res"] is None else op["block"] + 1] = y
            elif kind == "maxpool":
                assert "pool" not in op
                self.write(op["out"], orc.maxpool(self.read(op["inp"]), op["ksize"], op["stride"]))
            elif kind == "upsample":
                self.write(op["out"], orc.upsample(self.read(op["inp"]), op["stride"]))
            elif kind == "add":
                self.write(op["out"], self.read(op["inp"]) + self.read(op["res"], self.es))
            elif kind == "copy":
                self.write(op["out"], self.read(op["inp"]))
            elif kind == "reorg":
                y = R2.reorg(self.read(op["inp"]).numpy(), op["stride"], bool(op.get("form3d")))
                self.write(op["out"], torch.from_numpy(y))
            elif kind == "yolo":
                heads[op["block"]] = self.read(op["inp"], 4)  # the decode kernels load float32, always
            else:
                raise AssertionError(kind)
            # a value kept on chip lives for exactly one op: the one directly after its producer
            self.handed = produced
        flush(len(tensor_of))
        return heads


def check_plan(case, plan, es, mode, want=None):
    """Run ``plan`` of ``case`` and compare every block, at the moment it exists, bit for bit with ``reference_blocks``.  Returns
    the number of blocks compared; raises PlanError naming the first block that differs."""
    if want is None:
        want = reference_blocks(case["path"], case["params"], case["x"], EMULATE[es])
    seen = []

    def on_block(i, got):
        if not bit_equal(got, want[i]):
            bad = ~(got.view(torch.int32) == want[i].view(torch.int32)) if got.shape == want[i].shape else None
            raise PlanError("block %d (%s), %s, es=%d: %s values differ from the reference, %s NaN" % (
                i, case["blocks"][i]["type"], mode, es, "all" if bad is None else int(bad.sum()), int(torch.isnan(got).sum())))
        seen.append(i)

    Interp(plan, case["params"], case["x"], es, mode).run(on_block)
    fused_convs = sum(1 for t in plan["tensor_of"] if t is None)
    assert len(seen) == len(case["blocks"]) - fused_convs, (len(seen), len(case["blocks"]), fused_convs)
    return len(seen)
