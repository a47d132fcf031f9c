"""numpy float64 restatement of the depth read-out's definition: F.interpolate's trilinear
coordinate rule per axis, the softmax over depth, the expectation over the levels and the largest probability.
"""
import numpy as np


def axis(I, O, align_corners):
    """(i0, i1, t) for every output index of an axis with input extent I and output extent O."""
    o = np.arange(O, dtype=np.float64)
    if align_corners:
        src = o * ((I - 1) / (O - 1)) if O > 1 else np.zeros(O)
    else:
        src = np.maximum(0.0, (o + 0.5) * I / O - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), I - 1)
    i1 = np.minimum(i0 + 1, I - 1)
    return i0, i1, src - i0


def lerp_axis(v, ax, O, align_corners):
    i0, i1, t = axis(v.shape[ax], O, align_corners)
    shape = [1] * v.ndim
    shape[ax] = O
    t = t.reshape(shape)
    return (1.0 - t) * np.take(v, i0, axis=ax) + t * np.take(v, i1, axis=ax)


def upsample(cost, out, align_corners):
    """cost [N, D, H, W] -> [N, D_out, H_out, W_out], trilinear."""
    v = np.asarray(cost, dtype=np.float64)
    for ax, O in zip((1, 2, 3), out):
        v = lerp_axis(v, ax, O, align_corners)
    return v


def readout(cost, levels, out, align_corners):
    """depth [N, H_out, W_out] and the largest probability per pixel."""
    u = upsample(cost, out, align_corners)
    e = np.exp(u - u.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return (p * np.asarray(levels, dtype=np.float64).reshape(1, -1, 1, 1)).sum(axis=1), p.max(axis=1)
