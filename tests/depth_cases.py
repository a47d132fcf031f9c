"""The case table of the depth read-out (snvc_amd.depth) and of the pseudo-LiDAR projection, shared by
tests/golden/make_golden_depth.py (which writes tests/golden/depth_ref.npz), tests/test_depth_host.py and
tests/test_gpu_depth.py.  Inputs come from the cases' seeds, so the golden file holds results only.
"""
import collections

import numpy as np

Case = collections.namedtuple("Case", "name cost out align scale grad hip")

# cost [N, D, H, W] -> (D_out, H_out, W_out); `scale` multiplies standard-normal logits; `grad`: the gradient is recorded;
# `hip`: the route depth_readout takes.
CASES = [
    Case("a", (2, 12, 5, 7), (12, 20, 28), False, 8.0, True, True),          # no depth interpolation, x4 spatial, batch 2
    Case("b", (1, 12, 5, 7), (48, 19, 27), True, 1.0, True, True),           # depth x4, non-integer spatial ratios
    Case("c", (1, 48, 6, 9), (192, 24, 36), False, 20.0, True, True),        # the DSGN form
    Case("d", (1, 80, 3, 4), (320, 12, 16), False, 1.0, False, True),        # above 256 planes
    Case("e_h1", (1, 12, 1, 7), (12, 4, 28), False, 1.0, True, True),        # a unit extent, clamped neighbours
    Case("e_w1", (1, 12, 5, 1), (12, 20, 4), False, 1.0, True, True),
    Case("f_shrink", (1, 12, 4, 17), (12, 3, 67), False, 1.0, False, False),  # shrinks in H: the torch route
    Case("f_wide", (1, 12, 4, 17), (12, 16, 67), False, 1.0, False, True),   # width off every tile multiple
    Case("g", (2, 12, 5, 7), (12, 20, 28), False, 1e4, False, True),         # huge logits: finite, confidence in (0, 1]
    Case("h", (1, 12, 5, 7), (12, 5, 7), False, 1.0, False, True),           # size=None: equals disparity_regression(softmax)
]
BY_NAME = {c.name: c for c in CASES}
COMPARED = [c for c in CASES if c.name != "g"]        # g is held to finiteness only; its error is no yardstick
QUANTITIES = ("depth", "conf", "grad")
LOSS_CASE = "a"                                        # DepthLoss over the read-out is recorded for this case

Z_NEAR, Z_FAR = 2.0, 59.6


def levels(c):
    return np.linspace(Z_NEAR, Z_FAR, c.out[0]).astype(np.float32)


def inputs(c):
    """cost float32 [N, D, H, W], upstream gradient float32 [N, H_out, W_out]."""
    r = np.random.default_rng(1000 + CASES.index(c))
    cost = (c.scale * r.standard_normal(c.cost)).astype(np.float32)
    gy = r.standard_normal((c.cost[0], c.out[1], c.out[2])).astype(np.float32)
    return cost, gy


def loss_target(c):
    """A sparse ground-truth depth map for DepthLoss: a fifth of the pixels are -1 (no return), some lie beyond 60 m."""
    r = np.random.default_rng(2000 + CASES.index(c))
    gt = r.uniform(1.0, 70.0, (c.cost[0], c.out[1], c.out[2])).astype(np.float32)
    gt[r.uniform(size=gt.shape) < 0.2] = -1.0
    return gt


# ---------------------------------------------------------------------------------------------------- points
PointCase = collections.namedtuple("PointCase", "name shape per_sample origin stride")

POINT_CASES = [
    PointCase("single", (2, 7, 9), False, (0.0, 0.0), (1.0, 1.0)),            # H * W below one block
    PointCase("batch", (2, 7, 9), True, (1.5, 2.5), (4.0, 4.0)),
    PointCase("blocks", (2, 40, 130), True, (0.0, 0.0), (1.0, 1.0)),          # several blocks, no multiple of the block
    PointCase("strided", (1, 40, 130), False, (2.0, 1.0), (3.0, 2.0)),
]
POINTS_BY_NAME = {c.name: c for c in POINT_CASES}


def point_inputs(c):
    """depth float32 [N, H, W] (a few NaN and inf among them), P float32 [3, 4] or [N, 3, 4], conf float32 [N, H, W]."""
    r = np.random.default_rng(3000 + POINT_CASES.index(c))
    n = c.shape[0]
    depth = r.uniform(1.0, 80.0, c.shape).astype(np.float32)
    flat = depth.reshape(-1)
    flat[r.choice(flat.size, 3, replace=False)] = [np.nan, np.inf, -np.inf]
    base = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    P = np.stack([base * (1.0 + 0.01 * k) for k in range(n)]).astype(np.float32) if c.per_sample else base.astype(np.float32)
    conf = r.uniform(0.0, 1.0, c.shape).astype(np.float32)
    return depth, P, conf


def pixel_grid(c):
    """u [W] and v [H] in float32: origin + index * stride, one rounding per operation."""
    _, h, w = c.shape
    u = np.float32(c.origin[0]) + np.arange(w, dtype=np.float32) * np.float32(c.stride[0])
    v = np.float32(c.origin[1]) + np.arange(h, dtype=np.float32) * np.float32(c.stride[1])
    return u.astype(np.float32), v.astype(np.float32)
