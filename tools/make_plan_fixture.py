"""Writes tests/golden/yolov3_plans.json: the plan descriptions (yolov3.plan.build_plan) of the YOLOv3 cfgs and
tests/golden/cfg/mini.cfg, op for op, for tests/test_yolov4_host.py to pin.  Made once from the plan compiler before it
learned mish, grouped routes and scale_x_y:

    git show <commit>:pytorch-yolov3_amd/yolov3/plan.py > plan_before.py
    python tools/make_plan_fixture.py plan_before.py
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

if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "pytorch-yolov3_amd", "yolov3", "plan.py")
    spec = importlib.util.spec_from_file_location("plan_under_test", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(plan_fixture.FIXTURE, "w") as fh:
        json.dump(plan_fixture.snapshot(mod.build_plan), fh, indent=0, sort_keys=True)
        fh.write("\n")
    print("wrote", plan_fixture.FIXTURE)
