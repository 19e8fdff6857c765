"""Write tests/golden/kernel_choice.json: the kernel every plan step runs, and each conv's fragment-weight bytes, for the matrix of
tests/kernel_choice_util.py (models x storage types x batches x input modes x option sets), from the library as built.

Runs without a GPU (plan creation only decides: fake device addresses, nothing is allocated or launched) and refuses to run
where torch sees one.  Identical plans are stored once.

    python tools/make_kernel_choice.py            # writes the fixture
    python tools/make_kernel_choice.py --check    # compares with it
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "pytorch-yolov3_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import kernel_choice_util as kc  # noqa: E402


def main():
    if torch.cuda.is_available():
        sys.exit("make_kernel_choice: a GPU is visible; the fake device addresses must not reach it")
    got = kc.all_choices()
    if "--check" in sys.argv[1:]:
        with open(kc.FIXTURE) as fh:
            want = json.load(fh)
        bad = [k for k in want["configs"] if k not in got["configs"] or kc.config_rows(got, k) != kc.config_rows(want, k)]
        print("%d configurations, %d differ" % (len(want["configs"]), len(bad)))
        for k in bad[:20]:
            print("  ", k)
        sys.exit(1 if bad else 0)
    with open(kc.FIXTURE, "w") as fh:
        json.dump(got, fh, separators=(",", ":"), sort_keys=True)
        fh.write("\n")
    names = {r[0] for r in got["rows"]}
    print("%d configurations, %d distinct plans, %d kernel names -> %s (%d bytes)" % (
        len(got["configs"]), len(got["plans"]), len(names), kc.FIXTURE, os.path.getsize(kc.FIXTURE)))


if __name__ == "__main__":
    main()
