"""Plans at the CU counts of a partitioned GPU, without a GPU (tests/cu_count_util.py; tests/test_gpu_cu_count.py runs them).

The library asks the device for its CU count at plan creation, in more than a dozen chooser rules and in the grids of the
persistent kernels; an MI355X answers 256, and so does a machine without a GPU.  ``y3_set_tuning("device_cus", n)`` is the seam:
these tests hold that it changes nothing by itself, that every shipped cfg still gets a plan whose recorded launches are sane
at 1, 20, 32, 64, 128 and 256 CUs, that the grids which read the count are what an independent restatement from the op's fields
says, and that the configurations the GPU file runs really cross every rule that reads the count.

The ops carry fake device addresses (tests/kernel_choice_util.py): never hand them to a library that can launch."""
import ctypes
import json
import os

import pytest
import torch

import cu_count_util as cu
import footprint_util as fu
import kernel_choice_util as kc
from yolov3 import _hip

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake device addresses must never reach a library that can launch")


def _count_in_force():
    """the count the choosers see, read back through a persistent grid: the patch kernel on 96 tiles launches min(96, CUs) workgroups"""
    case = fu.case_by_id("patch_strided_tiles")
    return cu.case_steps(case, "bf16")[0]["dims"][0]


# ------------------------------------------------------------------------------------------------ the seam is inert

def _assert_fixture_reproduced():
    with open(kc.FIXTURE) as fh:
        want = json.load(fh)
    got = kc.all_choices()
    assert sorted(got["configs"]) == sorted(want["configs"])
    bad = [key for key in want["configs"] if kc.config_rows(got, key) != kc.config_rows(want, key)]
    assert not bad, "%d of %d configurations changed, e.g. %s" % (len(bad), len(want["configs"]), bad[:5])


def test_seam_at_256_and_at_0_reproduces_every_recorded_plan():
    assert _hip.capabilities() & _hip.CAP_PLAN_OP_DIMS
    with _hip.device_cus(cu.OWN):
        _assert_fixture_reproduced()
    with _hip.device_cus(0):
        _assert_fixture_reproduced()
    _assert_fixture_reproduced()


@pytest.mark.parametrize("value", [-1, 4097, -(1 << 31), (1 << 31) - 1])
def test_out_of_range_count_is_refused_and_changes_nothing(value):
    lib = _hip.lib()
    with _hip.device_cus(20):
        rc = lib.y3_set_tuning(b"device_cus", value)
        assert rc != 0 and b"device_cus" in lib.y3_last_error() and str(value).encode() in lib.y3_last_error()
        assert _count_in_force() == 20
    assert _count_in_force() == 96
    with pytest.raises(RuntimeError, match="device_cus"):
        with _hip.device_cus(value):
            pass
    assert _count_in_force() == 96


@pytest.mark.parametrize("value", [1, 4096])
def test_the_ends_of_the_range_are_taken(value):
    with _hip.device_cus(value):
        assert _count_in_force() == min(96, value)
    assert _count_in_force() == 96


def test_context_manager_restores_the_device_count_after_an_exception():
    with pytest.raises(ZeroDivisionError):
        with _hip.device_cus(32):
            assert _count_in_force() == 32
            1 // 0
    assert _count_in_force() == 96
    with _hip.device_cus(64):                       # nested use: the inner block ends at 0, as documented, not at 64
        with _hip.device_cus(20):
            assert _count_in_force() == 20
        assert _count_in_force() == 96


def test_plan_op_dims_reports_zeros_for_absorbed_ops_and_refuses_bad_arguments():
    lib = _hip.lib()
    steps = cu.case_steps(fu.case_by_id("resblock_ragged"), "bf16")
    assert steps[0]["kernel"].startswith("conv_resblock_fused_") and steps[0]["dims"] == (12, 512, 113152)
    assert steps[1]["kernel"].startswith("(fused") and steps[1]["dims"] == (0, 0, 0)
    out = (ctypes.c_int64 * 3)()
    assert lib.y3_plan_op_dims(None, 0, out) != 0 and b"y3_plan_op_dims" in lib.y3_last_error()


# ------------------------------------------------------------------------------------------------ plans exist and are sane

@pytest.mark.parametrize("count", cu.COUNTS)
@pytest.mark.parametrize("model,dim", cu.MODELS)
def test_every_cfg_gets_a_sane_plan(model, dim, count):
    """three dtypes x batches 1 and 16 x six option sets: creation succeeds, and every launched step recorded at least one workgroup
    of whole waves, at most 1024 threads, at most 160 KiB of LDS and fewer than 2^32 threads in all"""
    n = 0
    with _hip.device_cus(count):
        for dtype in kc.DTYPE_NAMES:
            for batch in (1, 16):
                for oname, over in cu.OPTION_SETS.items():
                    steps = cu.plan_steps(model, dim, dtype, batch, over)
                    what = "%s %s b%d %s at %d CUs" % (model, dtype, batch, oname, count)
                    for i, st in enumerate(steps):
                        if not cu.launched(st):
                            assert st["dims"] == (0, 0, 0), (what, i, st["kernel"], st["dims"])
                            continue
                        bad = cu.sane(st["kernel"], st["dims"])
                        assert bad is None, "%s, op %d (block %d): %s" % (what, i, st["op"].block_idx, bad)
                        n += 1
    assert n > 36 * 20


# ------------------------------------------------------------------------------------------------ geometry, restated

@pytest.mark.parametrize("count", cu.COUNTS)
def test_recorded_launch_is_the_restated_one(count):
    """Every row of the footprint table under its own option set: where the row still gets its family at this count, grid x block
    read back from the plan is what footprint_util.launch_threads restates from the op's fields and the count (the five families
    whose grid reads the count included: footprint_util.persistent_grid, which calls nothing of the library)."""
    compared, moved, families = 0, [], set()
    with _hip.device_cus(count):
        for case in fu.cases():
            for dtype in case["dtypes"]:
                st = cu.case_steps(case, dtype)[0]
                bad = cu.sane(st["kernel"], st["dims"])
                assert bad is None, (case["id"], dtype, count, bad)
                if st["kernel"] != fu.family_name(case, dtype):
                    moved.append((case["id"], dtype, st["kernel"]))
                    continue
                grid, block, _ = st["dims"]
                want = fu.launch_threads(case, dtype, case["B"], n_cu=count)
                assert want is not None, case["id"]
                assert grid * block == want, "%s %s at %d CUs: the plan recorded %d x %d threads, the restatement says %d" % (
                    case["id"], dtype, count, grid, block, want)
                fam = case["family"].split("_%s")[0]
                if fam in fu.PERSISTENT_BLOCK:
                    assert grid == fu.persistent_grid(case, st["op"], case["B"], count), (case["id"], dtype, count, grid)
                if fam == "conv1x1_wres":
                    n_tiles = st["op"].out_c // int(case["family"].rsplit("x", 1)[1])
                    assert grid % n_tiles == 0 and grid >= n_tiles, (case["id"], dtype, count, grid, n_tiles)
                families.add(case["family"])
                compared += 1
    # rows move only where their option set leaves a rule that reads the count in force: conv1x1_dw's one round of n_cu / 4 .. n_cu
    # tiles, the 192-pixel strips, the small-grid and deep-1x1 rules of the default set, the channel-tile shrink
    assert all(k.startswith(("conv_igemm", "conv_halo_ws_", "conv1x1_dw_", "conv_dw48_", "conv_patch_")) for _, _, k in moved), moved
    assert set(f for f in fu.PERSISTENT_BLOCK) <= {f.split("_%s")[0] for f in families}, families
    assert compared > 600 and (count != cu.OWN or not moved), (compared, moved)


def test_new_rows_give_workgroups_two_different_tile_counts_at_20_cus_and_every_tile_at_1():
    for cid in cu.PERSISTENT_ROWS:
        case = fu.case_by_id(cid)
        for dtype in case["dtypes"]:
            with _hip.device_cus(0):
                own = cu.case_steps(case, dtype)[0]
            with _hip.device_cus(20):
                g20 = cu.case_steps(case, dtype)[0]
            with _hip.device_cus(1):
                g1 = cu.case_steps(case, dtype)[0]
            assert own["kernel"] == g20["kernel"] == g1["kernel"] == fu.family_name(case, dtype)
            tiles = fu.persistent_grid(case, own["op"], case["B"], 1 << 30)          # (no CU count caps it: one workgroup a tile)
            # on the whole chip every workgroup owns ONE tile: the tile-to-tile code does not run there
            assert own["dims"][0] == tiles, (cid, own["dims"], tiles)
            why = cu.uneven(case, g20["op"], g20["dims"][0], tiles)
            assert why is None, "%s %s at 20 CUs: %s" % (cid, dtype, why)
            # one workgroup owns them all (the weights-resident kernel: one per channel tile, which owns every pixel tile)
            n_tiles = g1["op"].out_c // int(case["family"].rsplit("x", 1)[1]) if cid.startswith("wres") else 1
            assert g1["dims"][0] == n_tiles, (cid, g1["dims"])


def test_block_rectangle_does_not_depend_on_the_count():
    """csrc/conv_block.hip choose_tile ranks rectangles by rounds of workgroups over the CU count, then by tiles; rounds never fall
    as tiles rise, so the pick is the fewest tiles at every count (footprint_util.block_tile restates it without a count).  The
    library's grid -- one workgroup a rectangle -- says so on maps from 4 x 8 to 76 x 76."""
    base = fu.case_by_id("block_ragged_nores")
    for h, w, B in ((4, 8, 1), (19, 13, 3), (21, 17, 2), (19, 19, 3), (38, 38, 2), (37, 53, 1), (76, 76, 1), (45, 24, 5), (33, 25, 4)):
        case = dict(base, h=h, w=w, B=B)
        # ... and for the direct-weights form of the kernel (fuse_block = 4), which takes its rectangle from the same chooser
        for opt_name, kernel in ((None, "conv_block_fused_bf16_x128"), ("fuse_block4", "conv_block_dw_bf16_x128")):
            grids = set()
            for count in cu.COUNTS + (2, 3, 5, 7, 11):
                with _hip.device_cus(count):
                    st = cu.case_steps(case, "bf16", opt_name)[0]
                assert st["kernel"] == kernel, (h, w, B, count, st["kernel"])
                grids.add(st["dims"][0])
            tw, th = fu.block_tile(h, w)
            assert grids == {-(-w // tw) * -(-h // th) * B}, (h, w, B, grids, tw, th)


def test_fuse_block_3_names_the_direct_weights_form_exactly_where_fuse_block_1_fuses():
    """the 70 % rule reads the count, the launch does not: at every count of the list, on the block rows of the table and on the
    shipped 76 x 76 pair at batches round the rule's edge, fuse_block = 3 names conv_block_dw_* exactly where fuse_block = 1 names
    conv_block_fused_* -- with the same grid -- and both leave the same two launches elsewhere"""
    rows = [(fu.case_by_id(cid), {}) for cid in ("block_full_res", "block_ragged_res", "block_ragged_nores", "block_19x19_res")]
    rows += [(fu.case_by_id("block_full_res"), dict(h=76, w=76, B=B)) for B in (1, 2, 8, 11, 12, 16)]
    fused_at = set()
    for case, over in rows:
        case = dict(case, **over)
        for dtype in case["dtypes"]:
            for count in cu.COUNTS:
                with _hip.device_cus(count):
                    one = cu.case_steps(case, dtype, "fuse_block1")
                    three = cu.case_steps(case, dtype, "fuse_block3")
                fused = one[0]["kernel"] == "conv_block_fused_%s_x128" % fu.TAG[dtype]
                assert fused == one[0]["kernel"].startswith("conv_block")
                what = (case["id"], over, dtype, count, one[0]["kernel"], three[0]["kernel"])
                if fused:
                    assert three[0]["kernel"] == "conv_block_dw_%s_x128" % fu.TAG[dtype], what
                    assert three[0]["dims"][:2] == one[0]["dims"][:2] and cu.sane(three[0]["kernel"], three[0]["dims"]) is None, what
                    assert [s["kernel"] for s in one[1:]] == [s["kernel"] for s in three[1:]] == ["(fused into the previous op)"]
                    fused_at.add(count)
                else:
                    assert [s["kernel"] for s in three] == [s["kernel"] for s in one] and len(three) == 2, what
    assert {1, 256} <= fused_at          # the rule falls on both sides at both ends of the list


# ------------------------------------------------------------------------------------------------ reach

# rules of cu_count_util.RULES that nothing can cross, and why
NEVER = {"block_tile": "test_block_rectangle_does_not_depend_on_the_count"}


def test_gpu_list_crosses_every_rule_that_reads_the_count():
    table = cu.reach_table()
    crossed = {row[0] for row in table}
    assert crossed == set(cu.RULES) - set(NEVER), "not crossed: %s; crossed but listed as never: %s" % (
        sorted(set(cu.RULES) - set(NEVER) - crossed), sorted(crossed & set(NEVER)))
    # every rule but the 70 % rule of the fused block (which needs a workgroup's worth of pixels per CU) is crossed at a count a
    # partition really has, not at the stress values alone
    at_partition = {row[0] for row in table if row[1] in (32, 64, 128)}
    assert at_partition == crossed - {"block_70_percent"}, sorted(crossed - at_partition)
    # DESIGN.md section 1 holds the table
    with open(os.path.join(kc.ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    for row in cu.reach_lines(table):
        assert row in design, "DESIGN.md (Other CU counts) lacks the line\n%s" % row


def test_network_plans_of_the_gpu_list_hold_the_kernels_they_are_run_for():
    """under 32 CUs the small input of the GPU file still gives yolov3 the fused stem pair, the fused residual block and the
    direct-weights 1x1 kernel (which 256 CUs never gives an input this small); the persistent 1x1 pays from 512 pixel tiles on
    whatever the count (csrc/conv_1x1.hip y3_conv1x1_wres_pays), so it runs under its option set"""
    for model, h, w, batch, oname in cu.NETS:
        if model != "yolov3":
            continue
        for dtype in ("bf16", "fp16"):
            with _hip.device_cus(32):
                names = {s["kernel"] for s in cu.plan_steps(model, h, dtype, batch, cu.NET_OPTIONS[oname], width=w)}
            with _hip.device_cus(0):
                own = {s["kernel"] for s in cu.plan_steps(model, h, dtype, batch, cu.NET_OPTIONS[oname], width=w)}
            for frag in cu.NET_EXPECT[oname]:
                frag = frag.replace("bf16", fu.TAG[dtype])
                assert any(frag in k for k in names), (model, dtype, oname, frag, sorted(names))
            if oname == "default":
                assert not any("conv1x1_dw" in k for k in own), sorted(own)
