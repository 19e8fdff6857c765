"""tests/plan_interp.py's CPU interpreter with the attention ops -- TEST INFRASTRUCTURE (tests/test_attention_host.py).

``AttnInterp`` runs a plan of ``yolov3.plan.build_plan`` literally (every op writes its output) on plan_interp's NaN-filled byte
arena, through its ``read`` / ``write`` / ``check_no_overlap``, and adds what tests/golden/cfg/attention.cfg needs beyond the graph
cfgs: the ``avgpool`` / ``scale_channels`` / ``sam`` ops and convs with ``mish`` and ``logistic``.  The arithmetic of every op is
tests/attention_restate.py's, which knows nothing of the planner; ``reference_blocks`` is that restatement's forward by block
index, so the two sides call the same functions on the same values and are compared bit for bit."""
import torch

import attention_restate as AR
import plan_interp as PI


def reference_blocks(path, params, x, emulate=None):
    return dict(enumerate(AR.Restatement(path, params).blocks_forward(x, emulate)))


class AttnInterp(PI.Interp):
    def __init__(self, plan, params, x, es, blocks):
        PI.Interp.__init__(self, plan, params, x, es, "literal")
        self.blocks = blocks

    def run(self, on_block=None):
        ops, tensor_of = self.plan["ops"], self.plan["tensor_of"]
        heads = {}
        nxt = 0

        def flush(upto):
            nonlocal nxt
            for j in range(nxt, upto):
                if on_block is not None and tensor_of[j] is not None:
                    on_block(j, heads[j] if j in heads else self.read(tensor_of[j]))
            nxt = max(nxt, upto)

        for n, op in enumerate(ops):
            flush(op["block"])
            kind = op["kind"]
            self.check_no_overlap(n, op)
            if kind == "conv":
                blk = self.blocks[op["block"]]
                y = AR.conv(self.read(op["inp"]), self.params[op["slot"]], blk, self.emulate)
                if op["res"] is not None:
                    y = y + self.read(op["res"], self.es)
                self.write(op["out"], y)
            elif kind == "add":
                self.write(op["out"], self.read(op["inp"]) + self.read(op["res"], self.es))
            elif kind == "copy":
                self.write(op["out"], self.read(op["inp"]))
            elif kind in AR.KINDS:
                src = None if kind == "avgpool" else self.read(op["res"], self.es)      # d_res: the plan's element size
                self.write(op["out"], AR.attention_block({"type": kind}, self.read(op["inp"]), src, torch.float32))
            elif kind == "yolo":
                heads[op["block"]] = self.read(op["inp"], 4)
            else:
                raise AssertionError(kind)
        flush(len(tensor_of))
        return heads


def check_plan(case, plan, es):
    """run ``plan`` of ``case`` and compare every block, at the moment it exists, bit for bit with ``reference_blocks``; returns
    the number of blocks compared, raises plan_interp.PlanError naming the first block that differs"""
    want = reference_blocks(case["path"], case["params"], case["x"], PI.EMULATE[es])
    seen = []

    def on_block(i, got):
        if not PI.bit_equal(got, want[i]):
            raise PI.PlanError("block %d (%s), es=%d: differs from the forward by block index, %d NaN" % (
                i, case["blocks"][i]["type"], es, int(torch.isnan(got).sum())))
        seen.append(i)

    AttnInterp(plan, case["params"], case["x"], es, case["blocks"]).run(on_block)
    return len(seen)
