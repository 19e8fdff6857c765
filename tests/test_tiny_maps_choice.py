"""The rows of tests/tiny_maps_util.py held to their (kernel, map) pairs through the planner, without a GPU: plan creation only
decides when every address is fake (tests/kernel_choice_util.py).  tests/test_gpu_tiny_maps.py runs the same rows on an MI355X
and asserts the same pairs on the plans it ran; a chooser rule that takes a kernel off maps of one or two pixels fails here
first, and is then to be stated in the row that loses the pair."""
import pytest
import torch

import kernel_choice_util as kc
import tiny_maps_util as tm

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")


@pytest.mark.parametrize("row", tm.ROWS + tm.FP16_ROWS + tm.RECT_ROWS, ids=lambda r: r["id"])
def test_row_gets_its_pairs_at_both_batches(row):
    odd = tm.SQUARE_ODD_BATCH if row["h"] == row["w"] else tm.RECT_ODD_BATCH
    for batch in (1, odd):
        got = tm.planner_pairs(row, batch)
        missing = sorted(set(tm.pairs_of(row)) - got)
        assert not missing, "%s at batch %d: the planner no longer gives %s; it gives %s" % (row["id"], batch, missing, sorted(got))


def _producible(dims, dtypes, batch):
    out = set()
    for model in tm.MODELS:
        for dim in dims:
            for dtype in dtypes:
                for oname, over in kc.OPTION_SETS:
                    ch = kc.plan_choice(model, dim, dtype, batch, "u8", over)
                    out |= tm.plan_pairs(ch["kernel"], ch["map"])
    return out


def test_rows_reach_every_pair_the_planner_can_produce():
    """Every (kernel, map of one or two pixels a side) pair of the three yolov3 cfgs at 32- and 64-pixel inputs under every
    option set of kernel_choice_util.OPTION_SETS, float32 and bf16, is a pair of some row -- and no row names a pair that the
    planner cannot produce."""
    want = _producible((32, 64), ("float32", "bf16"), 1)
    have = {p for r in tm.ROWS for p in r["pairs"]}
    assert sorted(want - have) == [], "pairs no row is there for"
    assert sorted(have - want) == [], "pairs the planner never produces"
    families = {k for k, _ in want}
    print("%d (kernel, map) pairs of %d kernels on maps of one or two pixels a side" % (len(want), len(families)))
    assert len(want) >= 51


def test_fp16_pairs_are_the_bf16_pairs_renamed():
    for row in tm.FP16_ROWS:
        bf = next(r for r in tm.ROWS if r["id"] == row["id"].replace("fp16", "bf16"))
        got = tm.planner_pairs(row, 1)
        assert got == {(k.replace("bf16", "f16"), m) for k, m in tm.planner_pairs(bf, 1)}, row["id"]


def test_rectangular_rows_name_every_kernel_on_the_one_by_seven_maps():
    """the kernel lists of RECT_KERNELS / RECT_MODEL_KERNELS are exactly what the planner puts on the 1 x 7 and 7 x 1 maps"""
    for row in tm.RECT_ROWS:
        got = tm.planner_pairs(row, tm.RECT_ODD_BATCH, keep=lambda m: sorted(m) == [1, 7])
        assert got == set(row["pairs"]), (row["id"], sorted(got ^ set(row["pairs"])))
