"""Restatement of a grouped [convolutional] block, independent of the package: Darknet's ``groups=G`` splits the input channels
and the filters into G equal parts and convolves part g of the filters with part g of the input (src/convolutional_layer.c:
one GEMM per group on ``weights + j * nweights / groups`` and the group's im2col).  Here: slice input channels and parameters per
group, run the unchanged ``oracle.darknet_oracle.conv_block`` (the reference's conv -> BN -> LeakyReLU) on each slice, and
concatenate.  tests/test_grouped_host.py holds it equal to ``torch.nn.functional.conv2d(..., groups=G)`` in float64.

Activations the oracle's conv_block does not know (mish, logistic) are applied here, to its linear result.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import darknet_oracle as orc

PER_CHANNEL = ("bn_gamma", "bn_beta", "bn_mean", "bn_var", "bias")


def group_params(p, g, groups):
    """parameters of group ``g`` of ``groups``: its filters (rows of ``weight``, which is (Cout, Cin / groups, k, k)) and
    their per-channel tensors"""
    n = p["weight"].shape[0] // groups
    out = {"weight": np.ascontiguousarray(p["weight"][g * n:(g + 1) * n])}
    for key in PER_CHANNEL:
        if key in p:
            out[key] = np.ascontiguousarray(p[key][g * n:(g + 1) * n])
    return out


def activate(y, activation):
    """the activations of a Darknet conv block on its linear result (float32, torch's own functions)"""
    if activation == "leaky":
        return F.leaky_relu(y, orc.LEAKY_SLOPE)
    if activation == "mish":
        return y * torch.tanh(F.softplus(y))
    if activation == "logistic":
        return torch.sigmoid(y)
    assert activation == "linear", activation
    return y


def grouped_conv_block(x, p, stride, pad, activation, groups, round_weights=None, accumulate="f32"):
    """x (B, Cin, H, W) float32 -> (B, Cout, Ho, Wo) float32, not rounded.  ``p`` as weights.read_darknet_weights returns it,
    ``weight`` of shape (Cout, Cin / groups, k, k).  ``round_weights`` / ``accumulate`` as in the oracle's conv_block."""
    cin = x.shape[1]
    assert cin % groups == 0 and p["weight"].shape[0] % groups == 0 and p["weight"].shape[1] == cin // groups
    cg = cin // groups
    leaky = activation == "leaky"
    parts = [orc.conv_block(x[:, g * cg:(g + 1) * cg].contiguous(), group_params(p, g, groups), stride, pad, leaky,
                            round_weights=round_weights, accumulate=accumulate) for g in range(groups)]
    y = torch.cat(parts, dim=1)
    return y if leaky else activate(y, activation)


def conv2d_f64(x, p, stride, pad, activation, groups):
    """the same block through ``torch.nn.functional.conv2d(..., groups=groups)`` in float64 (batch norm folded the textbook way)"""
    w = torch.from_numpy(np.ascontiguousarray(p["weight"])).double()
    y = F.conv2d(x.double(), w, None, stride=stride, padding=pad, groups=groups)
    if "bn_gamma" in p:
        g, b, m, v = (torch.from_numpy(np.ascontiguousarray(p[k])).double().reshape(1, -1, 1, 1)
                      for k in ("bn_gamma", "bn_beta", "bn_mean", "bn_var"))
        y = (y - m) / torch.sqrt(v + float(orc.BN_EPS)) * g + b
    else:
        y = y + torch.from_numpy(np.ascontiguousarray(p["bias"])).double().reshape(1, -1, 1, 1)
    return activate(y, activation)
