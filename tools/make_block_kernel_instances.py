#!/usr/bin/env python
"""Writes tests/golden/kernel_instances_block.json: the census of the kernel instances compiled into libyolov3_hip_block.so
(csrc/conv_block_dw.hip), in the format of tests/golden/kernel_instances.json (tests/kernel_census.py).

Run once on an MI355X, after an instance of conv_block_dw, a case of tests/test_gpu_block_dw.py or a row of
tests/block_dw_cases.py was added or removed:

    python tools/make_block_kernel_instances.py [OUTPUT.json]

Every case of tests/test_gpu_block_dw.py and tests/test_gpu_block_dw_suites.py, and the epilogue pins of the kernel
(tests/test_gpu_epilogue.py), run with the library's launch log -- with all of its assertions but the comparison
with the fixture -- and the symbols it launched are recorded under its key.  The rules of tests/block_dw_util.py census_report
are then held against the kernels the built library holds -- every compiled kernel launched by a case and by a contention case,
no recorded symbol the library lacks -- and the file is written only when they hold."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import block_dw_cases as BDC
    import block_dw_util as BU
    import kernel_census as census
    import test_gpu_block_dw as TG
    import test_gpu_block_dw_suites as TS
    import test_gpu_epilogue as TE
    import test_gpu_footprint as TF
    from yolov3 import _hip
    _hip.require_gpu()
    TG.RECORD = rec = {"footprint": {}, "contention": {}}
    for m, c, dtype in BU.CASES:
        TG.test_block_dw_is_bit_identical_to_the_two_launches(m, c, dtype)
    TG.test_block_dw_against_the_float64_oracle_at_one_ulp()
    for res, dtype in TG.CONTENTION:
        TG.test_block_dw_beside_a_copy_kernel(res, dtype)
    # the kernel-level suites (tests/block_dw_cases.py): they run through the harness of tests/test_gpu_footprint.py, which records
    # under its own switch; the fragment-order copies' kernel belongs to the main library's census and is not recorded here
    TF.RECORD = frec = {}
    for cid in TS.IDS:
        TS.test_block_dw_touches_exactly_its_operands(cid)
        for kind in BDC.PLANTS:
            TS.test_block_dw_sum_is_exact_on_planted_integers(cid, kind)
    TS.test_block_dw_one_frame_below_4_gib()
    TF.RECORD = None
    frec.pop(TF.FRAGMENT_KEY, None)
    assert not set(frec) & set(rec["footprint"])
    rec["footprint"].update(frec)
    # ... and the epilogue pins, which record through tests/test_gpu_block_dw.py's switch: one combination per storage type
    for dtype in TE.FUSED_DTYPES:
        TE.test_fused_bottleneck_block_epilogues(dtype, 9, 3, ("leaky", "leaky"))
    TG.RECORD = None
    fixture = {table: {k: rec[table][k] for k in sorted(rec[table])} for table in ("footprint", "contention")}
    library = {k[".name"] for k in BU.library_kernels()}
    uncovered, stale, quiet_only = BU.census_report(fixture, library)
    print("block kernel census: %d symbols, %d covered by cases" % (len(library), len(library) - len(uncovered)))
    if uncovered or stale or quiet_only:
        names = census.demangle(uncovered + stale + quiet_only)
        print("NOT written: kernels no case launches:\n  %s\nrecorded symbols the library does not hold:\n  %s\nkernels no "
              "contention case launches:\n  %s" % ("\n  ".join(names[s] for s in uncovered), "\n  ".join(names[s] for s in stale),
                                                   "\n  ".join(names[s] for s in quiet_only)))
        return 1
    out = sys.argv[1] if len(sys.argv) > 1 else BU.CENSUS_FIXTURE
    with open(out, "w") as f:
        f.write(json.dumps(fixture, indent=0, sort_keys=True) + "\n")
    print("wrote %s: %d footprint keys, %d contention keys" % (os.path.relpath(out, ROOT), len(fixture["footprint"]), len(fixture["contention"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
