"""Helpers the GPU tests of the detection tail share: forward outputs on the device, ``y3_detect`` through ctypes with buffers
of its own, a ``Detector`` run, and the comparisons -- exact, against another run or against the oracle's audited frames."""
import ctypes

import numpy as np
import torch

from yolov3 import _hip
from yolov3.inference import Detector

F = np.float32


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def out(box, prob, cls):
    return {"bbox_xywh": torch.from_numpy(box).cuda(), "class_prob": torch.from_numpy(prob).cuda(),
            "class_idx": torch.from_numpy(cls).cuda()}


def run_detector(box, prob, cls, orig_hw, prob_thresh, thresh, letterbox=None, **kw):
    batch, rows = prob.shape
    det = Detector(batch, rows, dev())
    det.run(out(box, prob, cls), np.asarray(orig_hw, np.int32), float(F(prob_thresh)), thresh, letterbox=letterbox, **kw)
    return det.fetch(return_rows=True)


def direct_detect(box, prob, cls, orig_hw, prob_thresh, thresh):
    """``y3_detect`` through ctypes with buffers of its own: per frame (tlbr, prob, cls, row)."""
    lib = _hip.lib()
    batch, rows = prob.shape
    d = dev()
    o = out(box, prob, cls)
    hw = torch.from_numpy(np.ascontiguousarray(orig_hw, dtype=np.int32)).to(d)
    nbytes = lib.y3_detect_workspace_bytes(batch, rows)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=d)
    count = torch.zeros(batch, dtype=torch.int32, device=d)
    tlbr = torch.empty((batch, rows, 4), dtype=torch.int64, device=d)
    dprob = torch.empty((batch, rows), dtype=torch.float32, device=d)
    dcls = torch.empty((batch, rows), dtype=torch.int64, device=d)
    drow = torch.empty((batch, rows), dtype=torch.int32, device=d)
    _hip.check(lib.y3_detect(o["bbox_xywh"].data_ptr(), o["class_prob"].data_ptr(), o["class_idx"].data_ptr(), batch, rows,
                             hw.data_ptr(), ctypes.c_float(float(F(prob_thresh))), ctypes.c_double(thresh), ws.data_ptr(), nbytes,
                             count.data_ptr(), tlbr.data_ptr(), dprob.data_ptr(), dcls.data_ptr(), drow.data_ptr(),
                             _hip.stream_ptr()))
    torch.cuda.synchronize()
    n = count.cpu().numpy()
    return [(tlbr[f, :n[f]].cpu().numpy(), dprob[f, :n[f]].cpu().numpy(), dcls[f, :n[f]].cpu().numpy(),
             drow[f, :n[f]].cpu().numpy().astype(np.int64))
            for f in range(batch)]


def same(a, b):
    assert len(a) == len(b)
    for fa, fb in zip(a, b):
        assert len(fa) == len(fb)
        for x, y in zip(fa, fb):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and np.array_equal(x, y)


def assert_canonical_order(prob, cls, rows):
    """The output order the header of detect.hip states: class ascending, score descending, then higher row first.  Scores
    compare as numbers; "then" applies to scores of one bit pattern (-0.0 and +0.0 are equal numbers and may come either way)."""
    prob, cls, rows = np.asarray(prob, F), np.asarray(cls, np.int64), np.asarray(rows, np.int64)
    assert not np.isnan(prob).any()
    same_cls = cls[1:] == cls[:-1]
    assert (cls[1:] >= cls[:-1]).all(), "classes do not ascend"
    assert (prob[1:] <= prob[:-1])[same_cls].all(), "scores of a class do not descend"
    tie = same_cls & (prob[1:].view(np.uint32) == prob[:-1].view(np.uint32))
    assert (rows[1:] < rows[:-1])[tie].all(), "tied scores: the higher row does not come first"


def assert_equals_oracle(got, want):
    """One frame of ``direct_detect`` against one audited frame of the oracle's ``postprocess``: the same rows, and the
    oracle's box, score (bit for bit) and class at every one of them.  No row is exempt.  Also the canonical order."""
    tlbr, prob, cls, rows = got
    w_tlbr, w_prob, w_cls, w_rows = want[:4]
    assert tlbr.dtype == np.int64 and prob.dtype == np.float32 and cls.dtype == np.int64
    assert len(set(rows.tolist())) == len(rows), "a row is reported twice"
    a, b = np.argsort(rows, kind="stable"), np.argsort(w_rows, kind="stable")
    assert np.array_equal(rows[a], w_rows[b]), "kept rows differ: %d only here, %d only in the oracle" % (
        len(set(rows.tolist()) - set(w_rows.tolist())), len(set(w_rows.tolist()) - set(rows.tolist())))
    assert np.array_equal(tlbr[a], w_tlbr[b])
    assert np.array_equal(prob[a].view(np.uint32), np.asarray(w_prob, F)[b].view(np.uint32))
    assert np.array_equal(cls[a], w_cls[b])
    assert_canonical_order(prob, cls, rows)
