#!/usr/bin/env python
"""Writes tests/golden/kernel_instances_grouped.json: the census of the kernel instances compiled into libyolov3_hip_grouped.so
(csrc/conv_grouped.hip), in the format of tests/golden/kernel_instances.json (tests/kernel_census.py).

Run once on an MI355X, after an instance of conv_dwise / conv_grouped or a footprint case of tests/test_gpu_grouped.py was added
or removed:

    python tools/make_grouped_kernel_instances.py

Every case of ``test_footprint_and_census`` runs with the library's launch log and the symbols it launched are recorded under its
key.  Two rules of tests/kernel_census.py are then held against the kernels the built library holds -- every compiled kernel
launched by a footprint case, no recorded symbol the library lacks -- and the file is written only when they hold."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import grouped_cases as GC
    import kernel_census as census
    import test_gpu_footprint as TF
    import test_gpu_grouped as TG
    from yolov3 import _hip
    _hip.require_gpu()
    TF.RECORD = rec = {}
    for instance in sorted(TG.FOOTPRINT):
        for dtype in GC.DTYPES:
            TG.test_footprint_and_census(instance, dtype)
    TF.RECORD = None
    fixture = {"footprint": {k: rec[k] for k in sorted(rec)}, "contention": {}}
    library = GC.library_symbols()
    uncovered, stale = GC.census_report(fixture, library)
    print("grouped kernel census: %d symbols, %d covered by footprint cases" % (len(library), len(library) - len(uncovered)))
    if uncovered or stale:
        names = census.demangle(uncovered + stale)
        print("NOT written: kernels no footprint case launches:\n  %s\nrecorded symbols the library does not hold:\n  %s" % (
            "\n  ".join(names[s] for s in uncovered), "\n  ".join(names[s] for s in stale)))
        return 1
    with open(GC.CENSUS_FIXTURE, "w") as f:
        f.write(json.dumps(fixture, indent=0, sort_keys=True) + "\n")
    print("wrote %s: %d footprint keys" % (os.path.relpath(GC.CENSUS_FIXTURE, ROOT), len(fixture["footprint"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
