"""Writes tests/golden/yolov4_plans.json: the plan descriptions (yolov3.plan.build_plan) of the YOLOv4 cfgs, op for op, for
tests/test_new_coords_host.py to pin.  Made once from the plan compiler before it learned logistic and new_coords:

    git show <commit>:pytorch-yolov3_amd/yolov3/plan.py > plan_before.py
    python tools/make_yolov4_plan_fixture.py plan_before.py
"""
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "pytorch-yolov3_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plan_fixture  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "yolov4_plans.json")
# (cfg, input size, batch, element size, reuse, fuse), as plan_fixture.CASES
CASES = (
    ("yolov4", 608, 16, 2, True, True),
    ("yolov4", 416, 1, 4, False, False),
    ("yolov4-tiny", 416, 16, 2, True, True),
    ("yolov4-tiny", 416, 1, 4, False, True),
)


def snapshot(build_plan):
    saved = plan_fixture.CASES
    plan_fixture.CASES = CASES
    try:
        return plan_fixture.snapshot(build_plan)
    finally:
        plan_fixture.CASES = saved


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "pytorch-yolov3_amd", "yolov3", "plan.py")
    spec = importlib.util.spec_from_file_location("plan_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(FIXTURE, "w") as fh:
        json.dump(snapshot(mod.build_plan), fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", FIXTURE)
