#!/usr/bin/env python
"""Writes tests/golden/kernel_instances_attn.json: the census of the kernel instances compiled into libyolov3_hip_attn.so
(csrc/attention.hip), in the format of tests/golden/kernel_instances.json (tests/kernel_census.py).

Run once on an MI355X, after an instance of attention.hip or a census case of tests/attention_util.py was added or removed:

    python tools/make_attn_kernel_instances.py [OUTPUT.json]

Every census case of tests/attention_util.py (one per compiled instance: kind x form x dtype) runs with the library's launch log --
with all the assertions of tests/test_gpu_attention.py's census test but the comparison with the fixture -- and the symbol it
launched is recorded under its key.  The record is then held against the kernels the built library holds -- every compiled kernel
launched by a case, no recorded symbol the library lacks -- and the file is written only when that holds."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import attention_util as AU
    import kernel_census as census
    from yolov3 import _hip
    _hip.require_gpu()
    fixture = {"footprint": {key: AU.run_census_case(key) for key in sorted(AU.CENSUS_KEYS)}}
    library = {k[".name"] for k in AU.library_kernels()}
    uncovered, stale = AU.census_report(fixture, library)
    print("attention kernel census: %d symbols, %d covered by cases" % (len(library), len(library) - len(uncovered)))
    if uncovered or stale:
        names = census.demangle(uncovered + stale)
        print("NOT written: kernels no case launches:\n  %s\nrecorded symbols the library does not hold:\n  %s" % (
            "\n  ".join(names[s] for s in uncovered), "\n  ".join(names[s] for s in stale)))
        return 1
    out = sys.argv[1] if len(sys.argv) > 1 else AU.CENSUS_FIXTURE
    with open(out, "w") as f:
        f.write(json.dumps(fixture, indent=0, sort_keys=True) + "\n")
    print("wrote %s: %d footprint keys" % (os.path.relpath(out, ROOT), len(fixture["footprint"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
