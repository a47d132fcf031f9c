"""Full-resolution depth read-out of a cost volume and the pseudo-LiDAR points made from it.

``GlobalStack`` ends at a one-channel cost volume [N, D, H/4, W/4].  DSGN's depth head, whose backbone this package mirrors,
turns it into a depth map by ``F.interpolate(cost, [D_out, H_img, W_img], mode='trilinear')``, a softmax over depth and the
expectation over the depth levels; the reference's ``snvc/utils/torch_utils.py:5-19`` (``project_image_to_rect``) turns a depth
map into rectified-camera points.  Here:

  ``depth_readout``     the three steps in one launch (``csrc/depth_head.hip``): the up-sampled volume is never stored.
                        Differentiable with respect to ``cost``: the forward keeps two small maps, the backward is one
                        deterministic launch.
  ``depth_to_points``   ``project_image_to_rect`` over a depth map, bit-equal to the reference's float32 result, with the
                        validity mask or an order-preserving compaction that stays on the device.
  ``DepthReadout``      the read-out as a module holding the depth levels.

Inputs the kernels do not serve (an output smaller than the input in H or W, dtypes other than float32, depth levels that need
a gradient) take the torch composition on the GPU; ``DEPTH_HIP[0] = False`` forces that route (the same-process baseline of
tools/bench_depth.py).  Every decision is counted in ``submodule._ROUTES`` as "depth_readout_hip" or "depth_readout_torch".  CPU
tensors raise, as elsewhere in the package.
"""
import math

import torch
from torch import nn
from torch.nn import functional as F

from . import _depth
from ._lib import check
from .ops import _gpu, _stream
from .ops import _ptr as _p
from .models.submodule import _ROUTES

__all__ = ["depth_readout", "depth_to_points", "DepthReadout", "DEPTH_HIP"]

DEPTH_HIP = [True]      # False: depth_readout takes the torch composition


# ---------------------------------------------------------------------------------------------------- the read-out
def _readout_torch(cost, levels, size, align_corners):
    """The composition the kernel replaces; materialises [N, D_out, H_out, W_out]."""
    up = F.interpolate(cost[:, None], size=(levels.numel(), size[0], size[1]), mode="trilinear", align_corners=align_corners)[:, 0]
    prob = F.softmax(up, 1)
    depth = torch.sum(prob * levels.to(dtype=prob.dtype).reshape(1, -1, 1, 1), 1)
    return depth, prob.detach().amax(1)


def _forward_hip(cost, levels, size, align_corners, conf, keep):
    n, d, h, w = cost.shape
    maps = lambda on: torch.empty((n, size[0], size[1]), dtype=torch.float32, device=cost.device) if on else None  # noqa: E731
    depth, c, m, z = maps(True), maps(conf), maps(keep), maps(keep)
    with torch.cuda.device(cost.device):
        check(_depth.lib().snvc_depth_readout_forward(_p(cost), _p(levels), _p(depth), _p(c), _p(m), _p(z), n, d, h, w, levels.numel(),
                                                      size[0], size[1], int(bool(align_corners)), _stream(cost)),
              "snvc_depth_readout_forward")
    return depth, c, m, z


class _Readout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, levels, size, align_corners):
        cost = cost.contiguous()
        depth, conf, m, z = _forward_hip(cost, levels, size, align_corners, True, True)
        ctx.save_for_backward(cost, levels, depth, m, z)
        ctx.align_corners = align_corners
        ctx.mark_non_differentiable(conf)
        return depth, conf

    @staticmethod
    def backward(ctx, gy, _gconf):
        cost, levels, depth, m, z = ctx.saved_tensors
        gy = gy.to(torch.float32).contiguous()
        n, d, h, w = cost.shape
        dcost = torch.empty_like(cost)
        with torch.cuda.device(cost.device):
            check(_depth.lib().snvc_depth_readout_backward(_p(cost), _p(levels), _p(depth), _p(m), _p(z), _p(gy), _p(dcost), n, d, h, w,
                                                           levels.numel(), depth.shape[1], depth.shape[2], int(bool(ctx.align_corners)),
                                                           _stream(cost)),
                  "snvc_depth_readout_backward")
        return dcost, None, None, None


def depth_readout(cost, levels, size=None, align_corners=False, confidence=False):
    """``sum_d softmax_d(U)[d] * levels[d]`` with ``U = F.interpolate(cost[:, None], (len(levels), *size), mode='trilinear',
    align_corners=align_corners)``: float32 ``cost`` [N, D, H, W] and ``levels`` [D_out] on the GPU -> depth [N, H_out, W_out].
    ``size`` = (H_out, W_out), None keeps the spatial extents.  With ``confidence=True`` also the largest probability per pixel
    (not differentiable).  Differentiable with respect to ``cost``; composes with ``loss3d.DepthLoss`` for training:
    ``DepthLoss()({'depth': depth_readout(cost, levels, gt.shape[-2:])}, {'gt_depth': gt})``."""
    _gpu(cost, "cost")
    if cost.dim() != 4:
        raise ValueError(f"cost must be [N, D, H, W], got {tuple(cost.shape)}")
    levels = torch.as_tensor(levels).to(cost.device)
    if levels.dim() != 1:
        raise ValueError(f"levels must be [D_out], got {tuple(levels.shape)}")
    n, d, h, w = cost.shape
    size = (h, w) if size is None else (int(size[0]), int(size[1]))
    if n == 0 or size[0] == 0 or size[1] == 0:                # nothing to compute: no launch
        out = cost.new_zeros((n, size[0], size[1])) + cost.sum() * 0
        return (out, out.detach().clone()) if confidence else out
    if d == 0 or h == 0 or w == 0 or levels.numel() == 0:
        raise ValueError("depth_readout: an output from an empty cost volume or from no depth levels")
    hip = (DEPTH_HIP[0] and cost.dtype == torch.float32 and size[0] >= h and size[1] >= w
           and levels.is_floating_point() and not levels.requires_grad)
    _ROUTES["depth_readout_hip" if hip else "depth_readout_torch"] += 1
    if not hip:
        depth, conf = _readout_torch(cost, levels, size, align_corners)
    else:
        levels = levels.detach().to(torch.float32).contiguous()
        if cost.requires_grad and torch.is_grad_enabled():
            depth, conf = _Readout.apply(cost, levels, size, bool(align_corners))
        else:
            depth, conf, _, _ = _forward_hip(cost.detach().contiguous(), levels, size, align_corners, confidence, False)
    return (depth, conf) if confidence else depth


class DepthReadout(nn.Module):
    """``depth_readout`` with the depth levels held as a (non-persistent) buffer.  The chain from the global stack to the
    local model's inputs::

        cost = GlobalStack(...).forward_pair(left, right, ...)          # [N, D, H/4, W/4]
        depth, conf = DepthReadout(levels)(cost, size=image.shape[-2:], confidence=True)
        points, counts = depth_to_points(depth, P, conf=conf, min_conf=0.1, z_range=(2.0, 59.6), compact=True)
        # -> TargetGenerator / roiaware_pool3d / points_in_boxes_gpu, which take such points
    """

    def __init__(self, levels, align_corners=False):
        super().__init__()
        self.register_buffer("levels", torch.as_tensor(levels, dtype=torch.float32).reshape(-1).clone(), persistent=False)
        self.align_corners = bool(align_corners)

    def forward(self, cost, size=None, confidence=False):
        return depth_readout(cost, self.levels, size=size, align_corners=self.align_corners, confidence=confidence)


# ---------------------------------------------------------------------------------------------------- points
def depth_to_points(depth, P, conf=None, min_conf=0.0, z_range=(0.0, math.inf), origin=(0.0, 0.0), stride=(1.0, 1.0), compact=False):
    """The reference's ``project_image_to_rect`` (snvc/utils/torch_utils.py:5-19) over a depth map [N, H, W]: pixel (i, j) has
    u = origin[0] + j * stride[0], v = origin[1] + i * stride[1], x = ((u - c_u) * z) / f_u + b_x, y = ((v - c_v) * z) / f_v +
    b_y, in float32 and in that order, bit-equal to the reference.  ``P`` is [3, 4] or [N, 3, 4].  A point is valid when z is
    finite, z_range[0] <= z < z_range[1] and, with ``conf`` [N, H, W], conf >= min_conf.

    compact=False -> (points [N, H, W, 3], valid bool [N, H, W]); invalid rows are zero.
    compact=True  -> (points [N, H * W, 3], counts int32 [N]); sample n's first counts[n] rows are its valid points in
                     row-major pixel order, the rest is zero.  Both stay on the device: nothing waits for it."""
    _gpu(depth, "depth")
    if depth.dim() != 3:
        raise ValueError(f"depth must be [N, H, W], got {tuple(depth.shape)}")
    n, h, w = depth.shape
    dev = depth.device
    z = depth.detach().to(torch.float32).contiguous()
    P = torch.as_tensor(P).detach().to(device=dev, dtype=torch.float32).contiguous()
    if tuple(P.shape) not in ((3, 4), (n, 3, 4)):
        raise ValueError(f"P must be [3, 4] or [{n}, 3, 4], got {tuple(P.shape)}")
    if conf is not None:
        if tuple(conf.shape) != (n, h, w):
            raise ValueError(f"conf must be {[n, h, w]}, got {list(conf.shape)}")
        conf = conf.detach().to(device=dev, dtype=torch.float32).contiguous()
    scalars = (float(min_conf), float(z_range[0]), float(z_range[1]), float(origin[0]), float(origin[1]), float(stride[0]),
               float(stride[1]))
    L = _depth.lib()
    with torch.cuda.device(dev):
        if not compact:
            points = torch.empty((n, h, w, 3), dtype=torch.float32, device=dev)
            valid = torch.empty((n, h, w), dtype=torch.bool, device=dev)
            if points.numel():
                check(L.snvc_depth_to_points(_p(z), _p(P), int(P.dim() == 3), _p(conf), *scalars, _p(points), _p(valid), n, h, w,
                                             _stream(z)), "snvc_depth_to_points")
            return points, valid
        points = torch.empty((n, h * w, 3), dtype=torch.float32, device=dev)
        counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        if points.numel():
            ws = torch.empty((L.snvc_depth_points_workspace_bytes(n, h * w) // 4,), dtype=torch.int32, device=dev)
            check(L.snvc_depth_to_points_compact(_p(z), _p(P), int(P.dim() == 3), _p(conf), *scalars, _p(ws), _p(points), _p(counts),
                                                 n, h, w, _stream(z)), "snvc_depth_to_points_compact")
        return points, counts
