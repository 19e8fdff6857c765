"""Whole networks at 32 x 32, 64 x 64, 32 x 224 and 224 x 32, block by block against the oracle (-m gpu): every kernel the planner
puts on a map of one or two pixels a side -- 1 x 1, 2 x 2, 1 x 7 / 7 x 1 and 2 x 14 / 14 x 2 maps, where every pixel is a border
pixel, a pixel tile holds dozens of frames, a halo row wraps through several frames, an op at batch 1 is less than one MFMA
fragment and a 13-wide pool window has one tap inside the image.

The rows, the (kernel, map) pairs each is there for and the two batches are those of tests/tiny_maps_util.py;
tests/test_tiny_maps_choice.py holds them to the planner without a GPU, and every test here asserts its pairs on the plan that
ran.  The walk and the gates are those of tests/test_gpu_bf16.py (``_every_block`` / ``_teacher_forced``), unchanged:

* bf16 / fp16: every block from the product's own input at one storage ulp plus its floor (``_close_bf16``), pools, upsamples
  and routes bit for bit, heads through the decode.  ``MISMATCH_MAX``, the share of values that may differ at all, is asserted
  per block at both batches: at batch 1, where a checked tensor holds as few as 512 values, the worst block measured has 3 of
  512 values on the other side of a rounding boundary (0.6 %, against the cap of 2 %; profiles/r18_tiny_maps_gpu_tests.log).
* float32: every conv from the product's own input against float64 accumulation at rtol 1e-4, atol 2e-5, the logits likewise,
  and the network outputs against the oracle in free run at the tolerances of
  tests/test_gpu_parity.py test_yolov3_float32_matches_oracle_at_other_input_sizes.
"""
import pytest

import tiny_maps_util as tm
from test_gpu_bf16 import _every_block

pytestmark = pytest.mark.gpu


def _run(row, batch, frames_checked):
    mode = row["dtype"]
    pairs = tm.pairs_of(row)
    # (expect_kernels are bf16 names that _teacher_forced renames for fp16; the pairs carry the row's own names)
    kernels = tuple(sorted({k for k, _ in row["pairs"]}))
    _every_block(row["model"], row["h"], row["w"], batch, tm.OPTIONS[row["opt"]], kernels, mode, pairs=pairs,
                 frames_checked=frames_checked)


@pytest.mark.parametrize("batch", [1, tm.SQUARE_ODD_BATCH])
@pytest.mark.parametrize("row", tm.ROWS + tm.FP16_ROWS, ids=lambda r: r["id"])
def test_every_block_on_maps_of_one_and_two_pixels(row, batch):
    """every frame of the batch is compared: 37 frames of 32 x 32 are fewer pixels than one frame of 208 x 208"""
    _run(row, batch, tuple(range(batch)))


@pytest.mark.parametrize("row", tm.RECT_ROWS, ids=lambda r: r["id"])
def test_every_block_on_one_by_seven_and_seven_by_one_maps(row):
    """61 frames run; the first, every eighth and the last are compared (the float64 oracle is this test's time)"""
    batch = tm.RECT_ODD_BATCH
    _run(row, batch, tuple(range(0, batch, 8)) + (batch - 1,))
