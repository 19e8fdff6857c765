"""``Darknet``: the reference's model object, executed by HIP kernels on MI355X.

Keeps the surface callers use (/root/reference/yolov3/darknet.py:318-476):
``Darknet(config_fpath, device)``, ``.load_weights(path) -> self``, ``.eval()``,
``.cuda(device)``, ``.forward(x) -> {"bbox_xywh", "class_prob", "class_idx"}`` plus the
attributes ``.blocks .net_info .device .blocks_to_cache .header .modules_``.

What is different underneath: no nn.Module graph.  ``forward`` compiles (once per input
shape) a flat op plan (yolov3/plan.py) and hands it to libyolov3_hip.so through the C ABI
(include/yolov3_hip.h); activations are NHWC in an arena, BN is a per-channel scale/bias in
the conv epilogue, shortcuts/routes/head-concat are fused away.  Extension over the
reference: ``dtype="bf16"`` / ``dtype="fp16"`` (16-bit storage, fp32 accumulate: the same kernels on the
bf16 / f16 MFMA, same rate; fp16 keeps 11 significand bits instead of 8) and uint8 BGR frame input with
the BGR->RGB, /255 preprocessing fused into the first conv (``forward_frames``).
"""
import ctypes

import numpy as np
import torch

from . import _hip
from .cfgparse import parse_config
from .plan import build_plan, check_blocks, check_grouped_conv, check_pool_mode
from .plan_ops import STORAGE, fill_ops, head_views, multi_label_options, padded_weight_dims
from .plan_ops import _round_up, fill_maxpool_op, yolo_decode_flags  # noqa: F401  (lived here; callers import them from here)
from .weights import conv_layout, read_darknet_weights

BN_EPS = np.float32(1e-5)


def f32_to_bf16_bits(a):
    """Round-to-nearest-even float32 -> bfloat16 bit patterns (uint16)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> np.uint64(16)) & np.uint64(1)) + np.uint64(0x7FFF)
    return ((u + r) >> np.uint64(16)).astype(np.uint16)


def f32_to_f16_bits(a):
    """Round-to-nearest-even float32 -> IEEE half bit patterns (uint16); subnormals kept, overflow -> inf (numpy's
    conversion, the same rounding as v_cvt_f16_f32 and torch's ``.half()``)."""
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(a, dtype=np.float32).astype(np.float16).view(np.uint16)


# storage modes: name -> (C ABI element type, bytes per element, torch view dtype, host rounding to bit patterns)
DTYPES = {
    "float32": STORAGE["float32"] + (torch.float32, None),
    "bf16": STORAGE["bf16"] + (torch.bfloat16, f32_to_bf16_bits),
    "fp16": STORAGE["fp16"] + (torch.float16, f32_to_f16_bits),
}
DTYPE_ALIASES = {"float32": "float32", "fp32": "float32", "f32": "float32", "bf16": "bf16", "bfloat16": "bf16",
                 "fp16": "fp16", "f16": "fp16", "float16": "fp16", "half": "fp16"}


def grouped_weight_layout(path, w, groups, cout_pad, k_ld):
    """Host array (float32, zero padded) of a grouped conv's kernel ``w`` (Cout, Cin / groups, k, k) in the layout of kernel
    family ``path`` (include/yolov3_hip.h: y3_conv_path).  PATH_GROUPED: [cout_pad][k_ld], row = output channel, column
    (ky * k + kx) * (Cin / groups) + c: the implicit-GEMM layout with the group's channel count.  PATH_DWISE (one channel per
    group): [k * k][k_ld], row = tap ky * k + kx, column = channel."""
    cout, cg, k = w.shape[0], w.shape[1], w.shape[2]
    if path == _hip.PATH_DWISE:
        if cg != 1 or groups != cout:
            raise ValueError("depthwise layout asked for a kernel of shape {} with groups={}".format(w.shape, groups))
        host = np.zeros((k * k, k_ld), dtype=np.float32)
        host[:, :cout] = w.reshape(cout, k * k).T
        return host
    host = np.zeros((cout_pad, k_ld), dtype=np.float32)
    host[:cout, :k * k * cg] = w.transpose(0, 2, 3, 1).reshape(cout, k * k * cg)
    return host


class BlockInfo(object):
    """Lightweight stand-in for the reference's per-block nn.Sequential (``modules_[i]``)."""

    def __init__(self, index, block):
        self.index = index
        self.type = block["type"]
        self.block = block

    def __repr__(self):
        return "BlockInfo({}, {})".format(self.index, self.type)


class _CompiledPlan(object):
    def __init__(self):
        self.handle = None
        self.arena = None
        self.keep = []
        self.ops = None
        self.n_ops = 0
        self.rows_total = 0
        self.batch = 0
        self.heads = None        # multi_label networks: y3_head_view array of the head convs' outputs

    def destroy(self):
        if self.handle is not None:
            _hip.lib().y3_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class _PlanMemory(object):
    """What ``plan_ops.fill_ops`` asks for addresses, backed by tensors: the compiled plan ``cp`` owns its arena and output
    buffers and keeps the network's shared device weights alive."""

    def __init__(self, net, cp, dev):
        self.net, self.cp, self.dev = net, cp, dev

    def arena(self, nbytes):
        self.cp.arena = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        return self.cp.arena.data_ptr()

    def conv(self, slot, path):
        wts = self.net._device_weights(slot, path, self.net.dtype, self.dev)
        self.cp.keep.append(wts)
        return wts["weight"].data_ptr(), wts["scale"].data_ptr(), wts["bias"].data_ptr()

    def fragment(self, slot, op, nbytes):
        frag = self.net._fragment_weights(slot, self.dev, op, nbytes)
        self.cp.keep.append(frag)
        return frag.data_ptr()

    def outputs(self, batch, rows_total):
        cp = self.cp
        cp.bbox = torch.empty((batch, rows_total, 4), dtype=torch.float32, device=self.dev)
        cp.prob = torch.empty((batch, rows_total), dtype=torch.float32, device=self.dev)
        cp.cls = torch.empty((batch, rows_total), dtype=torch.int64, device=self.dev)
        return cp.bbox.data_ptr(), cp.prob.data_ptr(), cp.cls.data_ptr()


class Darknet(object):
    def __init__(self, config_fpath, device="cpu", dtype="float32", keep_all=False, fuse=None, options=None, pool="reference",
                 scores="reference", multi_label=False):
        """
        Args:
            config_fpath (str): Darknet .cfg file.
            device (str): "cpu" [default, like the reference: darknet.py:319] only builds the description;
                ``forward`` needs "cuda" / "cuda:N" (an MI355X): pass it here or call ``.cuda()`` as the
                reference's command line does (__main__.py:119-120).
            dtype (str): "float32" (parity path, exact fp32 MFMA), "bf16" (bf16 activations/weights, fp32
                accumulation; the benchmarked throughput path) or "fp16" (IEEE half storage, same kernels and rate,
                eight times finer rounding: the throughput path closest to the reference's float32 results).
            pool (str): max-pool semantics of every [maxpool] block.  "reference" [default]: the reference's (stride 1:
                window [y, y+k), out-of-range taps count as 0.0).  "darknet": Darknet's (window centred by padding / 2,
                out-of-range taps ignored, out = (in + padding - size) / stride + 1), what yolov3-spp / yolov4 / yolov4-csp
                weights trained by Darknet expect from their SPP block.  Fixed for the life of the object; keys of the cfg
                never switch it on.
            scores (str): how a box's classes are scored by heads without ``new_coords``.  "reference" [default]: the
                reference's ``softmax(class logits).max() * sigmoid(obj)``.  "darknet": Darknet's independent logistic per class,
                ``sigmoid(obj) * sigmoid(class_c)``, what yolov3 / yolov3-tiny / yolov3-spp / yolov4 / yolov4-tiny weights were
                trained with (Y3_F_SCORES_DARKNET on every YOLO op; the heads stay fused).  ``new_coords`` heads (yolov4-csp)
                score the Darknet way already: the mode changes nothing there, nor on a [region] head (YOLOv2, softmax=1), whose
                Darknet rule is the soft-max.  Fixed for the life of the object; no cfg key
                switches it on.
            multi_label (bool): Darknet reports every class of a box whose score passes the threshold, the reference the
                arg-max class only.  True keeps the head convs' float32 outputs (``label_heads``) so that ``inference()``,
                ``detect_in_frames()`` ... and ``Pipeline`` expand them into one candidate per (box, class) before the
                detection tail (``y3_expand_labels``).  It needs ``scores="darknet"`` or a network all of whose heads are
                ``new_coords``: under the reference's soft-max the classes of a box are one distribution, not independent
                labels; a cfg with a [region] head (YOLOv2) is refused for the same reason.  ``forward()`` returns the
                single-label dict in every mode.
        """
        self._pool = check_pool_mode(pool)
        self._scores = _hip.check_scores_mode(scores)
        self._multi_label = bool(multi_label)
        self.blocks, self.net_info = parse_config(config_fpath)
        if self.net_info is None:
            raise ValueError("cfg {!r} has no [net] section".format(config_fpath))
        if self._multi_label:
            for i, blk in enumerate(self.blocks):
                if blk["type"] == "region":
                    raise ValueError("region block {}: multi_label=True is not supported on a [region] head: its soft-max scores "
                                     "the classes of a box as ONE distribution, so they are not independent labels".format(i))
        if self._multi_label and self._scores != "darknet":
            heads = [b for b in self.blocks if b["type"] == "yolo"]
            if not heads or not all(int(b.get("new_coords", 0)) != 0 for b in heads):
                raise ValueError("multi_label=True needs scores=\"darknet\" (or a cfg all of whose [yolo] heads are new_coords): "
                                 "the reference's soft-max scores the classes of a box as ONE distribution, so they are not "
                                 "independent labels")
        self.config_fpath = config_fpath
        self.keep_all = bool(keep_all)   # debugging: no arena reuse, so block_output() works
        # conv-pair fusion (stem + stride-2 conv, residual blocks): default on, off with keep_all unless asked for
        # (then the tensor between a fused pair is never written and block_output() of it is meaningless)
        self.fuse = (not self.keep_all) if fuse is None else bool(fuse)
        # kernel-selection options of this network's plans (include/yolov3_hip.h: y3_options), e.g.
        # {"auto_mask": 0}; None = the library's defaults at the time a plan is compiled
        self.options = dict(options) if options else None
        self.device = device
        self.header = None
        self.training = False
        self.dtype = DTYPE_ALIASES[str(dtype).replace("torch.", "")]

        # absolute route indices + cache set, as the reference computes them (darknet.py:334-349)
        self.blocks_to_cache = set()
        for i, blk in enumerate(self.blocks):
            if blk["type"] == "route":
                blk["layers"] = [j if j >= 0 else i + j for j in blk["layers"]]
                self.blocks_to_cache.update(blk["layers"])
            elif blk["type"] == "shortcut":
                self.blocks_to_cache.add(i - 1)
                self.blocks_to_cache.add(i + blk["from"])
            elif blk["type"] in ("scale_channels", "sam") and isinstance(blk.get("from"), int):
                self.blocks_to_cache.add(i - 1)          # (a missing `from` is check_blocks' to refuse, below)
                self.blocks_to_cache.add(i + blk["from"])
        check_blocks(self.blocks)       # what the kernels cannot compute is refused here, not run with other semantics
        self._out_channels, self._convs = conv_layout(self.blocks, self.net_info)
        for c in self._convs:           # groups= against the channel counts the layout has just worked out
            check_grouped_conv(self.blocks, c["block_idx"], c["cin"])
        if self.blocks and self.blocks[0]["type"] != "convolutional":
            raise ValueError("the first block must be [convolutional] (it reads the network input)")
        self.modules_ = [BlockInfo(i, b) for i, b in enumerate(self.blocks)]
        self._params = None          # host copies, list of dicts per conv
        self._dev_weights = {}       # (slot, path) -> dict of device tensors
        self._plans = {}
        self._zero = None

    @property
    def pool(self):
        """Max-pool semantics of this network, "reference" or "darknet": set by the constructor only, so that the cached
        plans of one object never mix modes."""
        return self._pool

    @property
    def scores(self):
        """Class scoring of this network, "reference" or "darknet": set by the constructor only, like ``pool``."""
        return self._scores

    @property
    def multi_label(self):
        """Whether the detection entry points report every class of a box that passes the threshold (set by the
        constructor only)."""
        return self._multi_label

    def label_heads(self, plan=None):
        """The detection heads' float32 conv outputs of ``plan`` (default: the plan of the last forward) as a ctypes array of
        ``y3_head_view`` for ``y3_expand_labels`` / ``Detector.run(labels=...)``.  They live in the plan's arena and are
        overwritten by its next forward.  Needs ``multi_label=True``: other plans reuse (or never write) those tensors."""
        if not self._multi_label:
            raise RuntimeError("construct Darknet(..., multi_label=True) to keep the detection heads' outputs")
        return (plan if plan is not None else self._last_plan).heads

    @property
    def nms_hint(self):
        """``(nms_kind, beta_nms)`` as the last [yolo] block of the cfg states them, or None when it has neither key
        (``beta_nms`` alone gives kind "iou", Darknet's default; ``nms_kind`` alone gives beta 0.6).  A hint only: no cfg key
        switches Darknet's suppression on -- pass it on, ``inference(net, f, nms_kind=net.nms_hint[0],
        beta_nms=net.nms_hint[1])``.  A kind this package does not compute (``cornersnms``) is reported as written, and
        using it raises the ValueError any unknown kind does."""
        heads = [b for b in self.blocks if b["type"] == "yolo"]
        if not heads or not ("nms_kind" in heads[-1] or "beta_nms" in heads[-1]):
            return None
        kind = heads[-1].get("nms_kind", "iou")
        kind = "iou" if kind == "default" else kind     # Darknet's name for plain IoU in a cfg
        return str(kind), float(heads[-1].get("beta_nms", 0.6))

    # ------------------------------------------------------------------ nn.Module-like surface
    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("inference-only implementation (BatchNorm uses running statistics)")
        return self.eval()

    def _move(self, device):
        """Device weights and compiled plans hold addresses on the old device: drop them when the device changes
        (they are rebuilt lazily by the next forward)."""
        if str(device) != str(self.device):
            self.__dict__.pop("_pipelines", None)
            self._dev_weights = {}
            for plan in self._plans.values():
                plan.destroy()
            self._plans = {}
            self._zero = None
        self.device = device
        return self

    def cuda(self, device=None):
        if device is None:
            return self._move("cuda")
        if isinstance(device, int):
            return self._move("cuda:%d" % device)
        return self._move(str(device))

    def to(self, device):
        return self.cuda(device) if str(device).startswith("cuda") else self._set_cpu()

    def cpu(self):
        return self._set_cpu()

    def _set_cpu(self):
        return self._move("cpu")

    def __call__(self, x):
        return self.forward(x)

    # ------------------------------------------------------------------ weights
    def load_weights(self, weights_path):
        """Read a Darknet ``.weights`` file (same stream order as darknet.py:415-476)."""
        self.header, params = read_darknet_weights(weights_path, self.blocks, self.net_info)
        return self.set_params(params)

    def set_params(self, params):
        """Install per-conv parameter dicts (see weights.read_darknet_weights)."""
        if len(params) != len(self._convs):
            raise ValueError("expected {} conv parameter sets, got {}".format(len(self._convs), len(params)))
        self._params = params
        self.__dict__.pop("_f16_range_checked", None)
        self.__dict__.pop("_pipelines", None)      # (their plans hold the old weights' addresses)
        self._dev_weights = {}
        for plan in self._plans.values():
            plan.destroy()
        self._plans = {}
        return self

    def update_bn(self, params):
        """New BN statistics / biases under the plans the network already holds: the folded scale and bias of every conv are
        written into their existing device copies, which the compiled plans read at run time.  The conv weights must be the
        installed ones (they are not uploaded again); use ``set_params`` to change them."""
        if self._params is None or len(params) != len(self._convs):
            raise ValueError("update_bn needs one parameter set per conv of a network that has parameters")
        for old, new in zip(self._params, params):
            if old["weight"].shape != new["weight"].shape or not np.array_equal(old["weight"], new["weight"]):
                raise ValueError("update_bn does not change conv weights: call set_params")
        self._params = params
        for key, entry in self._dev_weights.items():
            if key[1] == "fragment":          # the fragment-order copy of a conv's weights: weights only
                continue
            scale, bias = self._fold_bn(key[0])
            entry["scale"][:scale.size].copy_(torch.from_numpy(scale))
            entry["bias"][:bias.size].copy_(torch.from_numpy(bias))
        return self

    def _fold_bn(self, slot):
        """BN(eval) as y = conv*scale + bias, float32 like torch's CPU batch_norm
        (alpha = gamma / sqrt(var + eps), beta' = beta - mean * alpha)."""
        p = self._params[slot]
        cout = self._convs[slot]["cout"]
        if "bn_gamma" in p:
            inv_std = np.float32(1.0) / np.sqrt(p["bn_var"].astype(np.float32) + BN_EPS)
            scale = (p["bn_gamma"].astype(np.float32) * inv_std).astype(np.float32)
            bias = (p["bn_beta"].astype(np.float32) - p["bn_mean"].astype(np.float32) * scale).astype(np.float32)
        else:
            scale = np.ones(cout, dtype=np.float32)
            bias = p["bias"].astype(np.float32)
        return scale, bias

    def _device_weights(self, slot, path, dtype, dev):
        """Device copies of one conv's parameters in the layout of kernel family ``path``, weights rounded to the
        storage type ``dtype`` ("float32" / "bf16" / "fp16")."""
        dtype = DTYPE_ALIASES[{True: "bf16", False: "float32"}.get(dtype, dtype)]      # (round 1-4 callers passed a bool: bf16 or not)
        key = (slot, path, dtype, str(dev))
        es, to_bits = DTYPES[dtype][1], DTYPES[dtype][3]
        if key in self._dev_weights:
            return self._dev_weights[key]
        c = self._convs[slot]
        cout, cin, k, groups = c["cout"], c["cin"], c["k"], c.get("groups", 1)
        w = self._params[slot]["weight"].astype(np.float32)
        scale, bias = self._fold_bn(slot)
        cout_pad, k_ld = padded_weight_dims(path, cout, cin, k, es, groups)
        if path in (_hip.PATH_GROUPED, _hip.PATH_DWISE):
            host = grouped_weight_layout(path, w, groups, cout_pad, k_ld)
            dw = torch.from_numpy(to_bits(host).view(np.int16) if to_bits is not None else host).to(dev)
        elif path == _hip.PATH_STEM_MFMA:
            # 16-bit [32][32]: row = output channel, k = ky*9 + kx*3 + c_mem with c_mem the BYTE order of the
            # uint8 BGR frame (c_mem = 2 - c_rgb), zero padded (csrc/conv_small.hip: conv_stem_mfma_kernel)
            host = np.zeros((cout_pad, k_ld), dtype=np.float32)
            wk = w[:, ::-1, :, :].transpose(0, 2, 3, 1).reshape(cout, 27)      # (co, ky, kx, c_mem)
            host[:cout, :27] = wk
            dw = torch.from_numpy(to_bits(host).view(np.int16)).to(dev)
        elif path == _hip.PATH_STEM:
            host = np.zeros((k * k * cin, cout_pad), dtype=np.float32)
            host[:, :cout] = w.transpose(2, 3, 1, 0).reshape(k * k * cin, cout)
            dw = torch.from_numpy(host).to(dev)
        else:
            host = np.zeros((cout_pad, k_ld), dtype=np.float32)
            host[:cout, :k * k * cin] = w.transpose(0, 2, 3, 1).reshape(cout, k * k * cin)
            if to_bits is not None:
                dw = torch.from_numpy(to_bits(host).view(np.int16)).to(dev)
            else:
                dw = torch.from_numpy(host).to(dev)
        sc = np.zeros(cout_pad, dtype=np.float32)
        bi = np.zeros(cout_pad, dtype=np.float32)
        sc[:cout] = scale
        bi[:cout] = bias
        entry = dict(weight=dw, scale=torch.from_numpy(sc).to(dev), bias=torch.from_numpy(bi).to(dev),
                     cout_pad=cout_pad, k_ld=k_ld)
        self._dev_weights[key] = entry
        return entry

    # ------------------------------------------------------------------ plan compilation
    def _torch_device(self):
        if not str(self.device).startswith("cuda"):
            raise RuntimeError(
                "Darknet.forward runs only on an MI355X GPU (device={!r}); call .cuda() -- this build "
                "has no CPU execution path".format(self.device))
        _hip.require_gpu()
        dev = torch.device(self.device)
        return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())

    def _fragment_weights(self, slot, dev, op, nbytes):
        """The conv's weights in MFMA-fragment order (direct-weights strip kernel), ONE copy per (layer, storage type, device)
        next to the other device layouts: every plan of the network shares it (until round 6 each plan made its own with
        hipMalloc, ~40 MB per plan for yolov3) and ``set_params`` invalidates it with them.  Made on torch's current stream."""
        key = (slot, "fragment", self.dtype, str(dev))
        frag = self._dev_weights.get(key)
        if frag is None:
            frag = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
            _hip.check(_hip.lib().y3_conv_make_fragment_weights(ctypes.byref(op), frag.data_ptr(), _hip.stream_ptr()))
            self._dev_weights[key] = frag
            self._made_fragments = True
        return frag

    def _compile(self, batch, height, width, input_mode, options=None):
        # every allocation and launch of plan compilation happens on the NETWORK's device, whichever is current
        with torch.cuda.device(self._torch_device()):
            return self._compile_on_device(batch, height, width, input_mode, options)

    def _compile_on_device(self, batch, height, width, input_mode, options=None):
        if self._params is None:
            raise RuntimeError("call load_weights() / set_params() before forward()")
        dev = self._torch_device()
        options = multi_label_options(options if options is not None else self.options, self._multi_label)
        opt = _hip.options(**options) if options else None
        self._made_fragments = False
        desc = build_plan(self.blocks, self.net_info, batch, height, width, DTYPES[self.dtype][1], reuse=not self.keep_all,
                          fuse=self.fuse, pool=self.pool, keep_heads=self._multi_label)
        cp = _CompiledPlan()
        cp.batch = batch
        cp.rows_total = desc["rows_total"]
        cp.desc = desc
        # The zero page (source of padding taps and tile tails in the conv kernels) must outlive every plan that holds its
        # address: one per device index, and every plan keeps a reference.  (Until round 4 the test below compared
        # ``cuda:0`` with ``cuda``, so EVERY compile made a new page and dropped the old one under the plans compiled before:
        # once the allocator reused those 4 KiB, border pixels of the older plans read garbage.  Found by
        # tests/test_gpu_pipeline.py, which is the first test to check outputs of several plans of one network.)
        if self._zero is None or (self._zero.device.index or 0) != (dev.index if dev.index is not None else torch.cuda.current_device()):
            self._zero = torch.zeros(4096, dtype=torch.uint8, device=dev)
        cp.keep.append(self._zero)
        cp.ops, needs, _ = fill_ops(desc, self.net_info, self._convs, self.dtype, batch, input_mode, self._scores, opt,
                                    _PlanMemory(self, cp, dev))
        cp.n_ops = len(cp.ops)
        _hip.require_capabilities(needs, self.config_fpath)
        if self._multi_label:
            cp.heads = head_views(cp.ops)
        handle = ctypes.c_void_p()
        if self._made_fragments:          # plans run on other streams than the one the copies were made on
            torch.cuda.current_stream().synchronize()
        _hip.check(_hip.lib().y3_plan_create_ex(cp.ops, cp.n_ops, self._zero.data_ptr(),
                                                ctypes.byref(opt) if opt is not None else None, ctypes.byref(handle)))
        cp.handle = handle
        return cp

    def _get_plan(self, batch, height, width, input_mode, slot=0, options=None):
        # `slot` selects an independent arena + output buffers (one per in-flight batch when the caller
        # pipelines batches over several HIP streams); `options` (a dict, see __init__) override the network's
        # plan options for this plan only (yolov3/pipeline.py asks for the throughput tile choice).  Any hashable `slot` names a
        # plan: whole numbers belong to forward_frames' callers (0: inference(), on the caller's stream), pipeline.plan_slot(k)
        # to the pipelines, which run theirs on streams of their own
        okey = tuple(sorted(options.items())) if options else None
        key = (batch, height, width, input_mode, self.dtype, str(self.device), slot, okey)
        cp = self._plans.get(key)
        if cp is None:
            cp = self._compile(batch, height, width, input_mode, options)
            self._plans[key] = cp
        return cp

    def _run(self, x, input_mode, timed=False, fresh=True, slot=0, options=None):
        """Launch the plan on torch's current stream.  ``fresh=False`` returns the plan's own
        output buffers (overwritten by the next call with the same shape) -- used by
        ``inference()`` and the benchmark, which consume them immediately."""
        dev = self._torch_device()
        lib = _hip.lib()
        if input_mode == "u8":
            batch, height, width, ch = x.shape
        else:
            batch, ch, height, width = x.shape
        if ch != self.net_info["channels"]:
            raise ValueError("input has {} channels, cfg says {}".format(ch, self.net_info["channels"]))
        cp = self._get_plan(batch, height, width, input_mode, slot, options)
        with torch.cuda.device(dev):
            if timed:
                # "kernel": events bound to every dispatch (the kernels' own begin -> end); True: events recorded on the
                # stream around every launch (includes dispatch handling) -- include/yolov3_hip.h
                ms = (ctypes.c_float * cp.n_ops)()
                run = lib.y3_plan_run_profiled if timed == "kernel" else lib.y3_plan_run_timed
                _hip.check(run(cp.handle, x.data_ptr(), _hip.stream_ptr(), ms))
                self.last_op_ms = list(ms)
            else:
                _hip.check(lib.y3_plan_run(cp.handle, x.data_ptr(), _hip.stream_ptr()))
        self._last_plan = cp
        if self.dtype == "fp16" and not timed and not self.__dict__.get("_f16_range_checked"):
            # IEEE half storage has no saturation: a stored activation above 65504 becomes inf and NaN downstream.
            # The procedural weights stay below 10 (profiles/r05_f16_overflow_audit.txt); real checkpoints are checked here, on
            # the FIRST forward after new parameters (one synchronising reduction, then never again): scores that are not finite
            # mean the half range was exceeded -- warn and point at bf16, which has float32's range.
            self._f16_range_checked = True
            if not bool(torch.isfinite(cp.prob).all()):     # (box sizes may be inf in any dtype: exp(tw) is unclamped, darknet.py:89-101)
                import warnings
                warnings.warn("dtype='fp16': non-finite outputs -- an activation exceeded the IEEE half range (65504); "
                              "use dtype='bf16' (float32 range) or 'float32' for these weights", RuntimeWarning)
        if fresh:
            return {"bbox_xywh": cp.bbox.clone(), "class_prob": cp.prob.clone(), "class_idx": cp.cls.clone()}
        return {"bbox_xywh": cp.bbox, "class_prob": cp.prob, "class_idx": cp.cls}

    # ------------------------------------------------------------------ forward
    def forward(self, x):
        """x: (B,3,H,W) float32 RGB in [0,1] (torch tensor, any device).  Returns the reference's
        dict of (B,M,4) / (B,M) / (B,M) tensors on the GPU (darknet.py:401-405)."""
        dev = self._torch_device()
        if not isinstance(x, torch.Tensor):
            x = torch.as_tensor(x)
        if x.dim() != 4:
            raise ValueError("expected a (B,C,H,W) tensor, got shape {}".format(tuple(x.shape)))
        x = x.to(device=dev, dtype=torch.float32).contiguous()
        return self._run(x, "f32")

    def forward_frames(self, frames_u8, fresh=True, slot=0, options=None):
        """frames_u8: (B,H,W,3) uint8 BGR (numpy or torch).  Same outputs as ``forward`` on
        ``flip(frames)/255`` transposed to NCHW (inference.py:332-333), preprocessing fused
        into the first conv kernel."""
        dev = self._torch_device()
        if not isinstance(frames_u8, torch.Tensor):
            frames_u8 = torch.from_numpy(np.ascontiguousarray(frames_u8))
        if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
            raise ValueError("expected uint8 (B,H,W,3) frames")
        return self._run(frames_u8.to(dev).contiguous(), "u8", fresh=fresh, slot=slot, options=options)

    def block_output(self, i):
        """(B,C,H,W) float32 copy of block i's output from the last forward.  Needs
        ``keep_all=True`` (otherwise the arena slot may have been reused)."""
        if not self.keep_all:
            raise RuntimeError("construct Darknet(..., keep_all=True) to inspect intermediate tensors")
        cp = self._last_plan
        t = cp.desc["tensor_of"][i]
        if t is None:
            raise ValueError("block {} is fused into its consumer and never materialised".format(i))
        es = 4 if t.f32 else DTYPES[self.dtype][1]
        start = cp.desc["offsets"][t.buf]
        nelem = cp.batch * t.h * t.w * t.ld
        raw = cp.arena[start:start + nelem * es]
        arr = raw.view(torch.float32 if es == 4 else DTYPES[self.dtype][2]).reshape(cp.batch, t.h, t.w, t.ld)
        return arr[:, :, :, t.off:t.off + t.c].permute(0, 3, 1, 2).float().contiguous()

    def plan_report(self):
        """Per-op (kernel name, flops, bytes, block) of the last executed plan (for bench/profiling); YOLO ops also carry
        ``scores``, the class scoring they compute ("reference" or "darknet"; a new_coords head reads "darknet" always)."""
        cp = self._last_plan
        lib = _hip.lib()
        report = [dict(kernel=lib.y3_plan_op_kernel(cp.handle, i).decode(),
                       flops=lib.y3_plan_op_flops(cp.handle, i), bytes=lib.y3_plan_op_bytes(cp.handle, i),
                       block=int(cp.ops[i].block_idx)) for i in range(cp.n_ops)]
        for i, entry in enumerate(report):
            if cp.ops[i].kind == _hip.OP_YOLO:
                dark = cp.ops[i].flags & (_hip.F_SCORES_DARKNET | _hip.F_NEW_COORDS)
                entry["scores"] = "darknet" if dark else "reference"
        return report
