"""A one-op Y3_OP_YOLO plan through ``y3_op_run`` for the GPU tests of the decode: the logits sit in a buffer whose pixel stride
is wider than the head and NaN outside it, and the outputs are pre-filled (NaN boxes and scores, class -7) so that a row the
decode does not write, or a value it takes from the padding, shows."""
import ctypes

import numpy as np
import torch

from yolov3 import _hip

ANCHORS = ((10.0, 14.0), (23.0, 27.0), (37.0, 58.0))
CLS_PREFILL = -7


def prefill(batch, rows):
    """the outputs as they are before the launch (host tensors): bbox (B, rows, 4) NaN, prob (B, rows) NaN, cls (B, rows) -7"""
    return (torch.full((batch, rows, 4), float("nan"), dtype=torch.float32), torch.full((batch, rows), float("nan"), dtype=torch.float32),
            torch.full((batch, rows), CLS_PREFILL, dtype=torch.int64))


def yolo_op(t, dtype, flags, anchors=ANCHORS, row_offset=0, rows_total=None, scale_x_y=None):
    """t (B, h, w, A, n_attr) float32 -> (rc, bbox, prob, cls) of a one-op Y3_OP_YOLO plan; dtype Y3_F32: the sequential form,
    Y3_BF16: four lanes per box (the logits are float32 either way).  The head's rows start at ``row_offset`` of outputs that
    hold ``rows_total`` rows a frame (default: the head's own), all of which are returned; ``scale_x_y`` None leaves the op's
    field at zero, which means 1."""
    b, h, w, a, n = t.shape
    ld = (a * n + 3) // 4 * 4 + 4
    x = torch.full((b, h, w, ld), float("nan"), dtype=torch.float32)
    x[..., :a * n] = torch.from_numpy(np.array(t, np.float32).reshape(b, h, w, a * n))
    x = x.cuda()
    rows = a * h * w
    rows_total = row_offset + rows if rows_total is None else rows_total
    assert row_offset >= 0 and row_offset + rows <= rows_total and len(anchors) >= a
    bbox, prob, cls = (v.cuda() for v in prefill(b, rows_total))
    zero = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    op = _hip.Y3Op()
    op.kind, op.dtype, op.flags, op.batch = _hip.OP_YOLO, dtype, flags, b
    op.in_h, op.in_w, op.in_c, op.in_ld = h, w, a * n, ld
    op.n_anchor, op.n_attr = a, n
    for k, (aw, ah) in enumerate(anchors[:a]):
        op.anchor_w[k], op.anchor_h[k] = aw, ah
    op.row_offset, op.rows_total = row_offset, rows_total
    op.net_w, op.net_h = 32.0 * w, 32.0 * h
    if scale_x_y is not None:
        op.scale_x_y = scale_x_y
    op.d_in, op.d_bbox, op.d_prob, op.d_cls = x.data_ptr(), bbox.data_ptr(), prob.data_ptr(), cls.data_ptr()
    rc = _hip.lib().y3_op_run(ctypes.byref(op), None, zero.data_ptr(), _hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, bbox.cpu().numpy(), prob.cpu().numpy(), cls.cpu().numpy()
