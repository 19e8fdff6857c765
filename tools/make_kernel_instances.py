#!/usr/bin/env python
"""Writes tests/golden/kernel_instances.json: the census of compiled kernel instances (tests/kernel_census.py).

Run once on an MI355X, after a kernel instance, a footprint row or a contention case was added or removed:

    python tools/make_kernel_instances.py

Every case of tests/test_gpu_footprint.py (the dense run of each row of footprint_util.cases(), and every other entry point's
footprint test, the two that live in tests/test_gpu_darknet_scores.py and tests/test_gpu_darknet_resize.py included) and of
tests/test_gpu_contention.py (the quiet run of each case; no contended rounds) runs with the library's launch log, and the
sorted set of code-object symbols each one launched is recorded under its key.  The census rules are then held against the
built library -- every compiled kernel launched by a footprint case or listed in kernel_census.UNREACHABLE, never both, no
stale symbol, every run-ahead instance under contention -- and the file is written ONLY when they hold; otherwise the tool
prints what is missing and exits with status 1 (``--report PATH`` writes what it recorded there all the same, for diagnosis)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def footprint():
    import footprint_util as fu
    import test_gpu_darknet_resize as TR
    import test_gpu_darknet_scores as TS
    import test_gpu_footprint as TF
    TF.RECORD = rec = {}
    frag = []
    for cname, dtype in fu.case_ids():
        case = fu.case_by_id(cname)
        del TF.LAUNCHED[:], TF.FRAGMENT_LAUNCHED[:]
        _, msg, names, _, _ = TF._run(case, dtype, "dense")
        assert msg is None and names[0] == fu.family_name(case, dtype), (cname, dtype, names, msg)
        frag += TF.FRAGMENT_LAUNCHED
        TF._assert_census("%s-%s" % (cname, dtype))
    TF.LAUNCHED[:] = frag
    TF._assert_census(TF.FRAGMENT_KEY)
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
    TF.RECORD = None
    return rec


def contention():
    import test_gpu_contention as TC
    TC.RECORDING = True
    TC.LAUNCHED.clear()
    for case in TC._case_ids():
        for dtype in ("bf16", "fp16"):
            TC.test_counted_wait_kernel_beside_a_copy_kernel(case, dtype)
    for res in (True, False):
        TC.test_fused_bottleneck_block_beside_a_copy_kernel(res)
    for mode, kernel, B, h, cin in TC.HEADS:
        for dtype in ("bf16", "fp16"):
            TC.test_head_kernels_beside_a_copy_kernel(mode, kernel, B, h, cin, dtype)
    TC.RECORDING = False
    return dict(TC.LAUNCHED)


def library_symbols():
    import test_code_object as T
    with open(T.LIB, "rb") as f:
        data = f.read()
    return {k[".name"] for _, elf in T._code_objects(data) for k in T._kernels(elf)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--report", help="also write what was recorded to this path, whether or not the rules hold")
    args = ap.parse_args()
    import kernel_census as census
    from yolov3 import _hip
    _hip.require_gpu()
    fixture = {"footprint": footprint(), "contention": contention()}
    fixture = {t: {k: fixture[t][k] for k in sorted(fixture[t])} for t in ("footprint", "contention")}
    text = json.dumps(fixture, indent=0, sort_keys=True) + "\n"
    if args.report:
        with open(args.report, "w") as f:
            f.write(text)
    library = library_symbols()
    print("kernel census: %(symbols)d symbols, %(covered)d covered by footprint cases, %(unreachable)d unreachable; "
          "%(run_ahead)d run-ahead instances, %(under_contention)d under contention" % census.totals(fixture, library))
    bad = census.failures(fixture, library)
    if bad:
        print("NOT written, the census rules fail:\n" + "\n".join(bad))
        return 1
    with open(census.FIXTURE, "w") as f:
        f.write(text)
    print("wrote %s: %d footprint keys, %d contention keys" % (os.path.relpath(census.FIXTURE, ROOT), len(fixture["footprint"]),
                                                                len(fixture["contention"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
