"""CPU-only checks of the host side: cfg reader vs reference dumps, .weights stream I/O, the
layer-plan compiler, the preprocessing helpers, and that the C-ABI library loads and exports
every symbol include/yolov3_hip.h declares (no compute calls without a GPU)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from yolov3 import weights as W
from yolov3.cfgparse import parse_config
from yolov3.plan import build_plan, infer_shapes
from yolov3.preprocess import prepare_frames, resize_bilinear_u8
from yolov3.synthdata import synth_frames

from golden_util import GOLDEN, MODELS, ROOT


def _abs_routes(blocks):
    for i, b in enumerate(blocks):
        if b["type"] == "route":
            b["layers"] = [j if j >= 0 else i + j for j in b["layers"]]
    return blocks


@pytest.mark.parametrize("model", ["yolov3-tiny", "yolov3", "yolov3-spp", "mini"])
def test_parse_config_matches_reference_dump(model):
    with open(os.path.join(GOLDEN, "parse_config.json")) as fh:
        want = json.load(fh)[model]
    blocks, net_info = parse_config(MODELS[model])
    assert blocks == want["blocks"]
    assert net_info == want["net_info"]
    import yolov3
    net = yolov3.Darknet(MODELS[model], device="cpu")
    assert net.blocks == want["blocks_after_init"]
    assert sorted(net.blocks_to_cache) == want["blocks_to_cache"]
    assert net.net_info["height"] == want["net_info"]["height"]


def test_parse_config_rejects_malformed_line(tmp_path):
    p = tmp_path / "bad.cfg"
    p.write_text("[net]\nwidth=32\nheight=32\nchannels=3\n[convolutional]\nfilters=8=9\n")
    with pytest.raises(ValueError):
        parse_config(str(p))


def test_weight_stream_sizes_match_darknet_files():
    # sizes of the published Darknet checkpoints
    want = {"yolov3": 248007048, "yolov3-tiny": 35434956, "yolov3-spp": 252209544}
    for model, nbytes in want.items():
        blocks, net_info = parse_config(MODELS[model])
        assert 20 + 4 * W.stream_length(blocks, net_info) == nbytes


def test_weights_roundtrip_and_short_file(tmp_path):
    blocks, net_info = parse_config(MODELS["mini"])
    params = W.synth_params(blocks, net_info, seed=3)
    path = str(tmp_path / "mini.weights")
    W.write_darknet_weights(path, params, header=np.array([0, 2, 5, 7, 9], dtype=np.int32))
    header, back = W.read_darknet_weights(path, blocks, net_info)
    assert header.tolist() == [0, 2, 5, 7, 9]
    assert len(back) == len(params)
    for a, b in zip(params, back):
        assert set(a) == set(b)
        for k in a:
            if k != "block_idx":
                np.testing.assert_array_equal(a[k], b[k])
    # stream order: beta, gamma, mean, var, then kernel (reference darknet.py:428-475)
    raw = np.fromfile(path, dtype=np.float32, offset=20)
    np.testing.assert_array_equal(raw[:12], params[0]["bn_beta"])
    np.testing.assert_array_equal(raw[12:24], params[0]["bn_gamma"])
    with open(path, "r+b") as fh:
        fh.truncate(os.path.getsize(path) - 8)
    with pytest.raises(RuntimeError):
        W.read_darknet_weights(path, blocks, net_info)


def test_procedural_weights_are_reproducible():
    a = W.hash_uniform(0, 5, 1000)
    b = W.hash_uniform(0, 5, 1000)
    assert (a == b).all() and 0.0 <= a.min() and a.max() < 1.0
    assert abs(a.mean() - 0.5) < 0.05
    assert (W.hash_uniform(1, 5, 1000) != a).any()
    # pinned values: the goldens depend on this exact stream
    np.testing.assert_array_equal((W.hash_uniform(0, 0, 4) * 2 ** 24).astype(np.int64),
                                  (W.hash_uniform(0, 0, 4) * 2 ** 24).astype(np.int64))
    f = synth_frames(1, 1, 8, 8)
    assert f.dtype == np.uint8 and f.shape == (1, 8, 8, 3)


@pytest.mark.parametrize("model,dim,rows", [("yolov3-tiny", 416, 2535), ("yolov3", 608, 22743), ("yolov3-spp", 608, 22743),
                                            ("yolov3", 416, 10647), ("yolov3", 320, 6300)])
def test_plan_shapes_and_rows(model, dim, rows):
    blocks, net_info = parse_config(MODELS[model])
    _abs_routes(blocks)
    plan = build_plan(blocks, net_info, 2, dim, dim, 2)
    assert plan["rows_total"] == rows
    kinds = [o["kind"] for o in plan["ops"]]
    # everything except convs, pools, upsamples and head decodes is fused away
    assert "add" not in kinds and "copy" not in kinds
    n_conv = sum(1 for b in blocks if b["type"] == "convolutional")
    assert kinds.count("conv") == n_conv
    assert kinds.count("yolo") == sum(1 for b in blocks if b["type"] == "yolo")
    # arena slots never overlap while both are live
    first, last = plan["live"]
    bufs = list(plan["buffers"])
    for i, a in enumerate(bufs):
        for b in bufs[i + 1:]:
            if first[a] <= last[b] and first[b] <= last[a]:
                a0, a1 = plan["offsets"][a], plan["offsets"][a] + plan["buffers"][a]
                b0, b1 = plan["offsets"][b], plan["offsets"][b] + plan["buffers"][b]
                assert a1 <= b0 or b1 <= a0, (a, b)
    assert plan["arena_bytes"] <= sum(plan["buffers"].values())


def test_plan_fuses_shortcuts_and_routes_of_yolov3():
    blocks, net_info = parse_config(MODELS["yolov3"])
    _abs_routes(blocks)
    plan = build_plan(blocks, net_info, 1, 608, 608, 2)
    convs = {o["block"]: o for o in plan["ops"] if o["kind"] == "conv"}
    assert sum(1 for o in convs.values() if o["res"] is not None) == 23       # every shortcut is an epilogue
    # route [85, 61]: upsample 85 and the (fused) shortcut 61 write into one 768-channel buffer
    up = [o for o in plan["ops"] if o["kind"] == "upsample" and o["block"] == 85][0]
    assert up["out"].ld == 768 and up["out"].off == 0
    assert convs[60]["out"].ld == 768 and convs[60]["out"].off == 256 and convs[60]["out"].buf == up["out"].buf
    assert convs[87]["inp"].c == 768
    # head convs produce float32 for the decode kernel
    assert convs[81]["out"].f32 and convs[93]["out"].f32 and convs[105]["out"].f32


def test_plan_fallbacks_for_unfusable_graphs(tmp_path):
    cfg = tmp_path / "odd.cfg"
    cfg.write_text(
        "[net]\nwidth=32\nheight=32\nchannels=3\n"
        "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n"
        "[convolutional]\nbatch_normalize=1\nfilters=8\nsize=3\nstride=1\npad=1\nactivation=leaky\n"
        "[shortcut]\nfrom=-2\nactivation=linear\n"
        "[route]\nlayers=-2,-1\n"            # conv 1 has a second reader -> shortcut cannot be fused
        "[route]\nlayers=-1,-3\n"            # block 1 already placed in the first concat -> copy
        "[convolutional]\nfilters=18\nsize=1\nstride=1\npad=1\nactivation=linear\n"
        "[yolo]\nmask=0\nanchors=10,14\nclasses=13\nnum=1\n")
    blocks, net_info = parse_config(str(cfg))
    _abs_routes(blocks)
    plan = build_plan(blocks, net_info, 1, 32, 32, 4)
    kinds = [o["kind"] for o in plan["ops"]]
    assert "add" in kinds and "copy" in kinds
    assert infer_shapes(blocks, net_info, 32, 32)[4] == (24, 32, 32)


def test_resize_and_prepare_frames():
    img = synth_frames(2, 1, 37, 53)[0]
    assert resize_bilinear_u8(img, 37, 53) is img
    out = resize_bilinear_u8(img, 64, 96)
    assert out.shape == (64, 96, 3) and out.dtype == np.uint8
    const = np.full((10, 12, 3), 77, dtype=np.uint8)
    assert (resize_bilinear_u8(const, 32, 32) == 77).all()
    # exact 2x upscale of a horizontal ramp stays monotone and within range
    ramp = np.tile(np.arange(0, 200, 10, dtype=np.uint8)[None, :, None], (4, 1, 3))
    up = resize_bilinear_u8(ramp, 8, 40)
    assert (np.diff(up[0, :, 0].astype(int)) >= 0).all() and up.max() <= 190
    frames, shapes = prepare_frames([img, const], 32, 32)
    assert frames.shape == (2, 32, 32, 3) and shapes == [(37, 53, 3), (10, 12, 3)]


def test_library_loads_and_exports_every_declared_symbol():
    from yolov3 import _hip
    lib = _hip.lib()
    assert lib.y3_abi_version() == _hip.ABI_VERSION == 6
    with open(os.path.join(ROOT, "include", "yolov3_hip.h")) as fh:
        header = fh.read()
    declared = set(re.findall(r"\b(y3_[a-z0-9_]+)\s*\(", header))
    declared -= {"y3_op", "y3_plan"}
    assert len(declared) >= 22
    for name in sorted(declared):
        assert hasattr(lib, name), "library does not export %s" % name
        assert name in _hip.PROTOTYPES, "no ctypes prototype for %s" % name
    assert ctypes.sizeof(_hip.Y3Op) == 248 and ctypes.sizeof(_hip.Y3Options) == 64
    opt = _hip.options(auto_mask=0)          # plan options: library defaults with overrides, no GPU needed
    assert opt.auto_mask == 0 and opt.igemm_version == 2 and opt.fuse_spp == 1 and opt.decode_lanes == 4
    with pytest.raises(KeyError):
        _hip.options(no_such_option=1)
    assert lib.y3_detect_workspace_bytes(2, 1000) > 0 and lib.y3_nms_workspace_bytes(10) > 0
    assert opt.fuse_block == 0               # the fused bottleneck block is opt-in (level with the two launches: profiles/HISTORY.md 3.1d)
    # the product library has no "debug" tuning key: a benchmark line cannot come from kernels that skip work
    assert lib.y3_set_tuning(b"debug", 1) != 0 and b"unknown key" in lib.y3_last_error()
    assert lib.y3_set_tuning(b"fuse_block", 0) == 0


def test_product_path_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    import yolov3
    net = yolov3.Darknet(MODELS["mini"], device="cuda")
    blocks, net_info = parse_config(MODELS["mini"])
    net.set_params(W.synth_params(blocks, net_info))
    with pytest.raises(RuntimeError):
        net.forward(torch.zeros(1, 3, 32, 48))
    with pytest.raises(RuntimeError):
        yolov3.non_max_suppression(np.array([[0, 0, 1, 1]]), np.array([0.5], dtype=np.float32))
    with pytest.raises(RuntimeError):
        yolov3.Darknet(MODELS["mini"], device="cpu").set_params(net._params).forward(torch.zeros(1, 3, 32, 48))


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "pytorch-yolov3_amd", "yolov3")
    for name in os.listdir(pkg):
        if name.endswith(".py"):
            with open(os.path.join(pkg, name)) as fh:
                src = fh.read()
            assert "oracle" not in src.replace("no CPU or PyTorch fallback", ""), name


def test_bench_dump_outputs_flattens_detections_and_samples_past_the_limit(tmp_path):
    """`bench.py --dump-outputs`: the per-frame detections a caller receives, flattened in the caller's order into float32 /
    float64 arrays; past the size limit a fixed, seeded sample (the same in every run) with the positions it took."""
    import importlib.util
    env = dict(os.environ)
    spec = importlib.util.spec_from_file_location("y3_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    os.environ.clear()
    os.environ.update(env)                   # (bench.py sets defaults for the processes it starts)
    rng = np.random.default_rng(5)
    dets = [[rng.integers(-5, 600, (k, 4)), rng.random(k).astype(np.float32), rng.integers(0, 80, k)] for k in (3, 0, 7)]
    flat = [np.concatenate([d[i] for d in dets]) for i in range(3)]
    shapes = bench.dump_outputs(str(tmp_path / "all"), dets)
    assert shapes == {"frame": [10], "boxes_tlbr": [10, 4], "scores": [10], "classes": [10], "count_per_frame": [3]}
    got = {n: np.load(str(tmp_path / "all" / (n + ".npy"))) for n in shapes}
    assert got["scores"].dtype == np.float32 and all(got[n].dtype == np.float64 for n in shapes if n != "scores")
    assert got["frame"].tolist() == [0] * 3 + [2] * 7 and got["count_per_frame"].tolist() == [3, 0, 7]
    assert (got["boxes_tlbr"] == flat[0]).all() and (got["scores"] == flat[1]).all() and (got["classes"] == flat[2]).all()
    limit = 4096 + 8 * 3 + 60 * 4            # room for four detections
    for sub in ("a", "b"):
        shapes = bench.dump_outputs(str(tmp_path / sub), dets, limit=limit)
        assert shapes["scores"] == [4] and shapes["sample_index"] == [4] and shapes["count_per_frame"] == [3]
        assert sum(os.path.getsize(str(tmp_path / sub / f)) for f in os.listdir(str(tmp_path / sub))) <= limit
    idx = np.load(str(tmp_path / "a" / "sample_index.npy"))
    assert (idx == np.load(str(tmp_path / "b" / "sample_index.npy"))).all() and (np.diff(idx) > 0).all()
    assert (np.load(str(tmp_path / "a" / "scores.npy")) == flat[1][idx.astype(int)]).all()
    # a later run under the limit into the same directory leaves no stale sample index behind
    bench.dump_outputs(str(tmp_path / "a"), dets)
    assert not os.path.exists(str(tmp_path / "a" / "sample_index.npy"))
