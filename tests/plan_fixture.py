"""Plan descriptions of the YOLOv3 cfgs in a JSON-comparable form (tools/make_plan_fixture.py, tests/test_yolov4_host.py)."""
import os

from yolov3.cfgparse import parse_config

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
FIXTURE = os.path.join(ROOT, "tests", "golden", "yolov3_plans.json")
MODEL_DIR = os.path.join(ROOT, "pytorch-yolov3_amd", "models")
# (cfg, input size, batch, element size, reuse, fuse)
CASES = (
    ("yolov3", 608, 16, 2, True, True),
    ("yolov3", 416, 1, 4, False, False),
    ("yolov3-tiny", 416, 8, 2, True, True),
    ("yolov3-spp", 608, 2, 2, True, True),
    ("yolov3-spp", 320, 1, 4, False, True),
    ("mini", 64, 2, 4, True, True),
)


def cfg_path(model):
    return os.path.join(ROOT, "tests", "golden", "cfg", "mini.cfg") if model == "mini" else os.path.join(MODEL_DIR, model + ".cfg")


def _plain(v):
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    return repr(v)                     # plan.Tensor


def snapshot(build_plan):
    out = {}
    for model, dim, batch, es, reuse, fuse in CASES:
        blocks, net_info = parse_config(cfg_path(model))
        for i, blk in enumerate(blocks):
            if blk["type"] == "route":
                blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
        d = build_plan(blocks, net_info, batch, dim, dim, es, reuse=reuse, fuse=fuse)
        out["%s|%d|b%d|es%d|%d%d" % (model, dim, batch, es, reuse, fuse)] = _plain(
            {k: d[k] for k in ("ops", "buffers", "offsets", "arena_bytes", "rows_total", "shapes", "n_convs", "tensor_of")})
    return out
