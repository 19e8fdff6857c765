"""The ops a ``Darknet`` on the GPU hands the library against ``kernel_choice_util.build_ops`` of the same configuration on fake
addresses (-m gpu): the host tests that pin kernel choice, launch dimensions and fusion refusals plan the product's own op list.

The test only fills and compares: no plan is created from the fake addresses."""
import ctypes

import numpy as np
import pytest

import yolov3
from yolov3 import _hip
from yolov3 import weights as W
from yolov3.plan_ops import multi_label_options

import kernel_choice_util as kc

pytestmark = pytest.mark.gpu

BATCH = 2
DARKNET_MULTI = dict(pool="darknet", scores="darknet", multi_label=True)
# (cfg, input side: the smallest tests/tiny_maps_util.py runs for it, and 64; constructor modes)
CASES = [pytest.param("yolov3-tiny", 32, {}, id="yolov3-tiny-32"), pytest.param("yolov3-tiny", 64, {}, id="yolov3-tiny-64"),
         pytest.param("yolov4-csp", 64, DARKNET_MULTI, id="yolov4-csp-64-darknet-multi_label")]
POINTERS = [name for name, ctype in _hip.Y3Op._fields_ if ctype is ctypes.c_void_p]
ARENA = ("d_in", "d_out", "d_res")
OUTPUTS = ("d_bbox", "d_prob", "d_cls")
_PARAMS = {}


def _params(model):
    if model not in _PARAMS:
        net = kc.network(model, "float32")
        _PARAMS[model] = W.synth_params(net.blocks, net.net_info, seed=0)
    return _PARAMS[model]


def _plain(v):
    return list(v) if isinstance(v, ctypes.Array) else v


@pytest.mark.parametrize("dtype", ["bf16", "float32"])
@pytest.mark.parametrize("model,dim,modes", CASES)
def test_compiled_ops_are_the_fake_address_ops(model, dim, modes, dtype):
    net = yolov3.Darknet(kc.network(model, dtype).config_fpath, device="cuda", dtype=dtype, **modes).set_params(_params(model)).eval()
    net.forward_frames(np.zeros((BATCH, dim, dim, 3), dtype=np.uint8))
    cp = net._last_plan
    opt = _hip.options(**(multi_label_options(None, net.multi_label) or {}))
    ops, _, fake = kc.build_ops(model, dim, dtype, BATCH, "u8", opt, **modes)
    assert cp.n_ops == len(cp.ops) == len(ops)
    assert len(POINTERS) == 10
    for n, (real, want) in enumerate(zip(cp.ops, ops)):
        for name, _ in _hip.Y3Op._fields_:
            a, b = getattr(real, name), getattr(want, name)
            if name not in POINTERS:
                assert _plain(a) == _plain(b), (n, name, _plain(a), _plain(b))
            else:
                assert (a is None) == (b is None), (n, name, a, b)
                if name in ARENA and a is not None:
                    assert a - cp.arena.data_ptr() == b - fake.base, (n, name)
    yolo = [op for op in cp.ops if op.kind == _hip.OP_YOLO]
    assert yolo
    for name, buf in zip(OUTPUTS, (cp.bbox, cp.prob, cp.cls)):
        assert {getattr(op, name) for op in yolo} == {buf.data_ptr()}, name
        assert len({getattr(op, name) for op in ops if op.kind == _hip.OP_YOLO}) == 1, name
