"""The summation order of ``avgpool_<dtype>`` (include/yolov3_hip.h: Y3_OP_AVGPOOL), restated in numpy float32 -- TEST
INFRASTRUCTURE, independent of the package.

A frame's P = H * W values of one channel, pixel p = y * W + x, are summed in float32 in one order that depends on P only:

    32 partial sums start at +0.0f; partial r adds pixels r, r + 32, r + 64, ... in increasing order;
    then s[r] += s[r + 16] for r < 16, and the same with 8, 4, 2, 1.  S = s[0].

The pool is ``S / float32(P)``, the correctly rounded float32 division, then one rounding to the storage type."""
import numpy as np

LANES = 32


def ordered_sum(x):
    """x: float32 (P, ...) -> float32 (...): the sum over the first axis in the kernel's order"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = np.zeros((LANES,) + x.shape[1:], dtype=np.float32)
    for p0 in range(0, x.shape[0], LANES):          # row k of every partial, in increasing k
        row = x[p0:p0 + LANES]
        s[:row.shape[0]] += row
    half = LANES // 2
    while half >= 1:
        s[:half] += s[half:2 * half]
        half //= 2
    return s[0]


def avgpool(x):
    """x: float32 (B, H, W, C) -> float32 (B, C), not yet rounded to storage"""
    b, h, w, c = x.shape
    flat = np.ascontiguousarray(x, dtype=np.float32).reshape(b, h * w, c).transpose(1, 0, 2)
    with np.errstate(all="ignore"):
        return (ordered_sum(flat) / np.float32(h * w)).astype(np.float32)


# ---- the faults the tests must catch (tests/test_attention_host.py holds each against the rule) -----------------------------

def wrong_sixteen_lane_sum(x):
    """a 16-lane tree in place of the 32-lane one"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = np.zeros((16,) + x.shape[1:], dtype=np.float32)
    for p0 in range(0, x.shape[0], 16):
        row = x[p0:p0 + 16]
        s[:row.shape[0]] += row
    for half in (8, 4, 2, 1):
        s[:half] += s[half:2 * half]
    return s[0]


def wrong_sequential_sum(x):
    """pixels added one after the other"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    s = np.zeros(x.shape[1:], dtype=np.float32)
    for row in x:
        s += row
    return s
