#!/usr/bin/env python
"""Writes tests/golden/kernel_instances*.json: the census of compiled kernel instances of every library that keeps one
(tests/kernel_census.py ``LIBRARIES``).

Run on an MI355X, after a kernel instance, or a case of one of the GPU tests named below, was added or removed:

    python tools/make_kernel_instances.py [--library main|grouped|block|attn ...] [--out DIR] [--report DIR]

Per library (all four by default) the value-checked GPU tests of ``RECORDERS`` run under ``census.recording()``: with all of
their assertions but the comparison with the fixture, and the sorted set of code-object symbols each one launched is recorded
under its key.  The census rules (``census.report``) are then held against the kernels the built library holds, and the
library's file is written -- in place, or into ``--out`` -- ONLY when they hold; otherwise the tool prints what is missing, goes
on with the next library and exits with status 1 (``--report DIR`` gets what was recorded all the same, for diagnosis)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def record_main():
    """every case of tests/test_gpu_footprint.py (the dense run of each row of footprint_util.cases(), and every other entry
    point's footprint test, the two that live in tests/test_gpu_darknet_scores.py and tests/test_gpu_darknet_resize.py included),
    then the quiet run of every case of tests/test_gpu_contention.py"""
    import footprint_util as fu
    import kernel_census as census
    import test_gpu_contention as TC
    import test_gpu_darknet_resize as TR
    import test_gpu_darknet_scores as TS
    import test_gpu_footprint as TF
    frag = []
    for cname, dtype in fu.case_ids():
        case = fu.case_by_id(cname)
        del census.LAUNCHED[:], census.FRAGMENT_LAUNCHED[:]
        _, msg, names, _, _ = TF._run(case, dtype, "dense")
        assert msg is None and names[0] == fu.family_name(case, dtype), (cname, dtype, names, msg)
        frag += census.FRAGMENT_LAUNCHED
        census.assert_census("%s-%s" % (cname, dtype))
    census.assert_census(census.FRAGMENT_KEY, launched=frag)
    for which in TF.DETECTORS:
        TF.test_detectors_stay_inside_exact_size_workspace_and_outputs(which)
    for which in TF.NMS:
        for n in TF.NMS_SIZES:
            TF.test_nms_entry_points_stay_inside_exact_size_workspace_and_outputs(which, n)
    TF.test_pack_records_stays_inside_exact_size_buffers()
    for src, dst in TF.RESIZES:
        TF.test_resize_stays_inside_exact_size_frames(src, dst)
    TF.test_letterbox_stays_inside_exact_size_frames()
    for nbytes in TF.COPY_SIZES:
        TF.test_copy_bytes_stays_inside_exact_size_buffers(nbytes)
    for which in TF.CXYWH:
        TF.test_cxywh_to_tlbr_stays_inside_exact_size_rows(which)
    TS.test_expand_labels_footprint()
    for net in TR.MIXED_NETS:
        for letterbox in (False, True):
            TR.test_mixed_batch_in_one_launch_stays_inside_its_output(net, letterbox)
    for case in TC._case_ids():
        for dtype in ("bf16", "fp16"):
            TC.test_counted_wait_kernel_beside_a_copy_kernel(case, dtype)
    for res in (True, False):
        TC.test_fused_bottleneck_block_beside_a_copy_kernel(res)
    for mode, kernel, B, h, cin in TC.HEADS:
        for dtype in ("bf16", "fp16"):
            TC.test_head_kernels_beside_a_copy_kernel(mode, kernel, B, h, cin, dtype)


def record_grouped():
    import grouped_cases as GC
    import test_gpu_grouped as TG
    for instance in sorted(TG.FOOTPRINT):
        for dtype in GC.DTYPES:
            TG.test_footprint_and_census(instance, dtype)


def record_block():
    """tests/test_gpu_block_dw.py, the kernel-level suites of tests/test_gpu_block_dw_suites.py (whose fragment-order copies are
    a kernel of the main library, recorded under "main" and so not written here), and one combination of the epilogue pins per
    storage type"""
    import block_dw_cases as BDC
    import block_dw_util as BU
    import test_gpu_block_dw as TG
    import test_gpu_block_dw_suites as TS
    import test_gpu_epilogue as TE
    for m, c, dtype in BU.CASES:
        TG.test_block_dw_is_bit_identical_to_the_two_launches(m, c, dtype)
    TG.test_block_dw_against_the_float64_oracle_at_one_ulp()
    for res, dtype in TG.CONTENTION:
        TG.test_block_dw_beside_a_copy_kernel(res, dtype)
    for cid in TS.IDS:
        TS.test_block_dw_touches_exactly_its_operands(cid)
        for kind in BDC.PLANTS:
            TS.test_block_dw_sum_is_exact_on_planted_integers(cid, kind)
    TS.test_block_dw_one_frame_below_4_gib()
    for dtype in TE.FUSED_DTYPES:
        TE.test_fused_bottleneck_block_epilogues(dtype, 9, 3, ("leaky", "leaky"))


def record_attn():
    import attention_util as AU
    import test_gpu_attention as TA
    for key in sorted(AU.CENSUS_KEYS):
        TA.test_every_compiled_instance_is_launched_where_the_census_says(key)


RECORDERS = {"main": record_main, "grouped": record_grouped, "block": record_block, "attn": record_attn}
# the top-level tables of each file as they have been from the start: the attention fixture has no contention table
TABLES = {"attn": ("footprint",)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--library", action="append", choices=list(RECORDERS), help="(repeatable; default: all four)")
    ap.add_argument("--out", help="write the files into this directory instead of tests/golden")
    ap.add_argument("--report", help="also write what was recorded into this directory, whether or not the rules hold")
    args = ap.parse_args()
    import kernel_census as census
    from yolov3 import _hip
    _hip.require_gpu()
    for d in (args.out, args.report):
        if d:
            os.makedirs(d, exist_ok=True)
    status = 0
    for name in args.library or list(RECORDERS):
        start = time.time()
        with census.recording() as record:
            RECORDERS[name]()
        mine = record.get(name, {})
        fixture = {t: {k: mine[t][k] for k in sorted(mine.get(t, {}))} for t in TABLES.get(name, ("footprint", "contention"))}
        text = json.dumps(fixture, indent=0, sort_keys=True) + "\n"
        base = os.path.basename(census.fixture_path(name))
        if args.report:
            with open(os.path.join(args.report, base), "w") as f:
                f.write(text)
        library = census.symbols(name)
        print("%s kernel census (%.0f s): %s" % (name, time.time() - start, census.summary(name, fixture, library)))
        bad = census.failures(name, fixture, library)
        if bad:
            print("%s NOT written, the census rules fail:\n%s" % (base, "\n".join(bad)))
            status = 1
            continue
        path = os.path.join(args.out, base) if args.out else census.fixture_path(name)
        with open(path, "w") as f:
            f.write(text)
        print("wrote %s: %s" % (os.path.relpath(path, ROOT), ", ".join("%d %s keys" % (len(fixture[t]), t) for t in fixture)))
    return status


if __name__ == "__main__":
    sys.exit(main())
