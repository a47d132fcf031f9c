"""The training losses of the reference's ``snvc/models/loss3d.py`` behind the same names, constructor arguments, call
signatures and dictionary keys (``snvc_amd.install_as_snvc()`` serves this module as ``snvc.models.loss3d``).

On the HIP route (GPU, float32 prediction) a loss is one streaming kernel plus a one-workgroup finalisation
(``csrc/loss.hip``, ``include/snvc_loss.h``) and its gradient one more kernel; nothing waits for the device.  Every loss
returns a 0-d float32 tensor that autograd differentiates with respect to the prediction(s).  Inputs that route does not
serve (CPU tensors, float64, targets or weights that need a gradient themselves, unusual ``target_weight`` shapes) take a
torch route with the reference's arithmetic.

Deviations from the reference, all deliberate:
  * an empty mask gives a 0-d zero tensor whose gradient is zeros where the reference returns the Python float ``0.``;
  * the two asserts that need a count (``VoxelMSELossWeighted``: a part without a positive target;
    ``sigmoid_focal_loss_multi_target``: a target outside {0, 1}) are checked on the device and raise ``LossInputError`` at
    the next call of that loss or at ``check()`` on the HIP route, at once on the torch route;
  * ``CoordinateLoss`` does not modify the caller's ``gt`` tensor;
  * ``depth_regression_loss`` is an addition;
  * ``RPN3DLoss``, ``disentangled_loss``, ``map2corners``, ``compute_IoU_loss_corner``, ``approximated_3d_iou_pt``,
    ``BboxLoss`` for ``head_reg_type == 'vector3d'`` and ``CoordinateLoss(enable_IoU=True)`` raise ``NotImplementedError``:
    upstream they call functions that exist nowhere in the reference, or belong to the global detector that is not there.
"""
import contextlib
import threading

import torch
from torch import nn
from torch.nn import functional as F

from .. import _loss
from .._loss import LossInputError

__all__ = [
    "sigmoid_focal_loss_multi_target", "smooth_l1_loss", "map2corners", "disentangled_loss", "RPN3DLoss", "W_loss", "calc_disp_loss",
    "DepthLoss", "VoxelMSELoss", "OccupancyLoss", "OffsetLoss", "compute_area_4pts", "compute_IoU_loss_corner", "ShapeLoss",
    "approximated_3d_iou_pt", "BboxLoss", "CoordinateLoss", "VoxelMSELossWeighted", "depth_regression_loss", "check", "LossInputError",
    "INF", "CFG_NAMES", "SELECT_IND1", "SELECT_IND2",
]

INF = 100000000
CFG_NAMES = ([f"CV_{axis}_{end}" for end in ("MIN", "MAX") for axis in "XYZ"] + [f"{axis}_{end}" for end in ("MIN", "MAX") for axis in "XYZ"]
             + [f"VOXEL_{axis}_SIZE" for axis in "XYZ"])
SELECT_IND1 = [1, 3, 7, 5]
SELECT_IND2 = [2, 4, 8, 6]


def check():
    """Wait for the device-side input checks of the losses called so far; raises ``LossInputError`` if one failed."""
    _loss.check_flags()


# ------------------------------------------------------------------------------ routing
_route = threading.local()


@contextlib.contextmanager
def _torch_route():
    """Within the block every loss called from this thread takes the torch route (how the tests compare the two routes on the
    same tensors).  Private: not part of what ``snvc.models.loss3d`` offers."""
    prev = getattr(_route, "torch_only", False)
    _route.torch_only = True
    try:
        yield
    finally:
        _route.torch_only = prev


def _on_hip(pred, *constants):
    """The HIP route serves a float32 GPU prediction whose other operands need no gradient."""
    if getattr(_route, "torch_only", False) or not (torch.is_tensor(pred) and pred.is_cuda and pred.dtype == torch.float32):
        return False
    return not any(torch.is_tensor(t) and t.requires_grad for t in constants)


def _f32(t, device):
    """``t`` as a contiguous float32 tensor on ``device`` (no copy if it already is one)."""
    return t.detach().to(device=device, dtype=torch.float32).contiguous()


def _zero_of(pred):
    """A 0-d float32 zero that is differentiable with respect to ``pred`` (gradient: zeros)."""
    return (pred.reshape(-1)[:0].sum() * 0.0).to(torch.float32)


def _unbuilt(name, why):
    raise NotImplementedError(f"snvc_amd.models.loss3d.{name} is not built: {why}")


_MISSING_UPSTREAM = ("the reference calls {0}, which is defined nowhere in the reference (its import is commented out, "
                     "snvc/models/loss3d.py:9-12)")
_NO_DETECTOR = "it belongs to the global detector (RPN3D head, Box3DList targets), which the reference release does not contain"


# ------------------------------------------------------------------------------ focal / smooth-L1 functions
def _focal_terms(p, t, gamma, alpha):
    term_pos = (1 - p) ** gamma * torch.log(p + 1e-7)
    term_neg = p ** gamma * torch.log(1 - p + 1e-7)
    return -(t == 1).to(p.dtype) * term_pos * alpha - (t == 0).to(p.dtype) * term_neg * (1 - alpha)


def sigmoid_focal_loss_multi_target(logits, targets, weights=None, gamma=2., alpha=0.25):
    """Sum over all elements of the focal loss of ``sigmoid(logits)`` against 0 / 1 ``targets``, times ``weights``."""
    if logits.shape != targets.shape:
        raise RuntimeError(f"logits {tuple(logits.shape)} and targets {tuple(targets.shape)} must share one shape")
    same_shape_w = weights is None or (torch.is_tensor(weights) and weights.shape == logits.shape and weights.is_floating_point())
    if _on_hip(logits, targets, weights) and same_shape_w:
        flag = _loss.flag_of(logits.device)
        flag.look(wait=False)
        dev = logits.device
        t = targets.to(dev)
        if t.dtype == torch.bool:
            t = t.view(torch.uint8)
        tflag = _loss.TARGET_FLAGS.get(t.dtype, 0)          # int32 / int64 / bool / uint8 labels are read as they are
        t = t.contiguous() if tflag else _f32(t, dev)
        w = None if weights is None else _f32(weights, dev)
        return _loss.elementwise(_loss.SIGMOID_FOCAL, logits.contiguous(), t, w, p0=alpha, p1=gamma, flags=tflag, post_flag=True)
    if not bool(torch.all((targets == 1) | (targets == 0))):
        raise LossInputError(_loss.FLAG_TEXT[_loss.FLAG_BAD_TARGET])
    loss = _focal_terms(torch.sigmoid(logits), targets, gamma, alpha)
    return loss.sum() if weights is None else (loss * weights).sum()


def smooth_l1_loss(input, target, weight, beta=1. / 9):
    """Smooth-L1 with a ``beta`` knee: the mean over dim 1, weighted per row and normalised by the weights' sum."""
    if (_on_hip(input, target, weight) and input.dim() == 2 and input.shape == target.shape and torch.is_tensor(weight)
            and weight.numel() == input.size(0) and input.numel() > 0):
        dev = input.device
        return _loss.elementwise(_loss.SMOOTH_L1_ROWS, input.contiguous(), _f32(target, dev), None, _f32(weight, dev).reshape(-1),
                                 group=input.size(1), p0=beta)
    n = torch.abs(input - target)
    loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return (loss.mean(dim=1) * weight).sum() / weight.sum()


def map2corners(pred):
    _unbuilt("map2corners", _MISSING_UPSTREAM.format("compute_corners_sc"))


def disentangled_loss(pred, target, weight):
    _unbuilt("disentangled_loss", _MISSING_UPSTREAM.format("compute_corners_sc (through map2corners)"))


class RPN3DLoss(object):
    def __init__(self, cfg=None, *args, **kwargs):
        _unbuilt("RPN3DLoss", _NO_DETECTOR)


# ------------------------------------------------------------------------------ depth / disparity
def W_loss(prob, target, off, mask, depth_levels, reduction='mean', p=1):
    """Wasserstein-style depth loss: per masked pixel, sum over depth levels of ``prob * |level + off - target| ** p``.
    ``prob`` and ``off`` are [B,D,H,W] and are read in that layout."""
    if (_on_hip(prob, target, depth_levels) and p == 1 and reduction in ('mean', 'none') and torch.is_tensor(off) and off.is_cuda
            and off.dtype == torch.float32 and mask.dtype == torch.bool):
        dev = prob.device
        m8 = mask.to(dev).contiguous().view(torch.uint8)
        out = _loss.wdist(prob.contiguous(), off.contiguous(), _f32(target, dev), m8, _f32(depth_levels, dev), per_pixel=reduction == 'none')
        return out if reduction == 'mean' else out[mask]          # 'none': one value per masked pixel (the shape needs the count)
    off_l = off.permute(0, 2, 3, 1)
    prob_l = prob.permute(0, 2, 3, 1)
    depth = depth_levels[None, None, None, :] + off_l
    tgt = target.unsqueeze(3)
    diff = depth[mask] - tgt[mask]
    out = torch.abs(diff) if p == 1 else diff ** p
    loss = torch.sum(prob_l[mask] * out, 1)
    if reduction == 'none':
        return loss
    if reduction == 'mean':
        return loss.mean()


_DISP_WEIGHTS = (0.5, 0.7, 1.0)


def calc_disp_loss(outputs, mask, gt_disp, loss_type='sl1'):
    """Depth / disparity loss of the global model.  ``'sl1'``: masked smooth-L1 mean of each of up to three predictions
    (``outputs['depth_preds']``), weighted 0.5 / 0.7 / 1.0 with the last prediction at 1.0; ``'W1'``: ``W_loss``."""
    if loss_type == 'sl1':
        preds = [torch.squeeze(o, 1) for o in outputs['depth_preds']]
        total = 0.
        for i, o in enumerate(preds):
            w = _DISP_WEIGHTS[3 - len(preds) + i]
            if _on_hip(o, gt_disp) and mask.dtype == torch.bool and o.shape == gt_disp.shape == mask.shape:
                m8 = mask.to(o.device).contiguous().view(torch.uint8)
                term = _loss.elementwise(_loss.SMOOTH_L1_MASKED, o.contiguous(), _f32(gt_disp, o.device), m8, p0=1.0,
                                         flags=_loss.EMPTY_IS_NAN)
            else:
                term = F.smooth_l1_loss(o[mask], gt_disp[mask], reduction='mean')
            total = total + w * term
        return total
    if loss_type == 'W1':
        return W_loss(outputs['prob'], gt_disp, outputs['offset'], mask, outputs['depth_levels'], reduction='mean', p=1)
    raise NotImplementedError(f"calc_disp_loss: loss_type {loss_type!r}")


class DepthLoss(nn.Module):
    """Smooth-L1 mean of ``outputs['depth']`` [N,H,W] against ``meta_data['gt_depth']`` where the target is neither -1 nor
    60 m or beyond."""

    def forward(self, outputs, meta_data=None):
        pred = outputs['depth']
        gt = meta_data['gt_depth'].to(pred.device)
        if _on_hip(pred, gt) and pred.shape == gt.shape:
            return _loss.elementwise(_loss.SMOOTH_L1_MASKED, pred.contiguous(), _f32(gt, pred.device), p0=1.0)
        mask = ((gt != -1) & (gt < 60.)).detach()
        if mask.sum() > 0:
            return F.smooth_l1_loss(pred[mask], gt[mask], reduction='mean')
        return _zero_of(pred)


def depth_regression_loss(cost, depth_levels, gt_depth):
    """``DepthLoss()({'depth': disparityregression(softmax(cost, 1), depth_levels)}, {'gt_depth': gt_depth})`` for a cost
    volume [N,D,H,W].  Not a name of the reference: an addition.  On the HIP route one forward kernel (softmax over D, the
    expectation, the mask, smooth-L1 and the reduction) and one backward kernel writing the gradient of ``cost``; neither the
    probability volume nor the depth map is stored."""
    gt = gt_depth.to(cost.device)
    if _on_hip(cost, depth_levels, gt) and cost.dim() == 4:
        return _loss.depth_regression_loss(cost.contiguous(), _f32(depth_levels, cost.device), _f32(gt, cost.device))
    prob = F.softmax(cost, 1)
    depth = torch.sum(prob * depth_levels.to(cost.device).reshape(1, -1, 1, 1), 1)
    return DepthLoss()({'depth': depth}, {'gt_depth': gt})


# ------------------------------------------------------------------------------ heat maps
def _row_weights(target_weight, parts, batch, device):
    """``target_weight[idx]`` (a scalar or [N,1] per part) as one float32 weight per (sample, part) row, or None if the shape
    is not one the kernel serves."""
    if not torch.is_tensor(target_weight) or target_weight.dim() == 0 or target_weight.requires_grad or target_weight.size(0) != parts:
        return None
    shape = tuple(target_weight.shape[1:])
    if shape in ((), (1,), (1, 1)):
        per_part = target_weight.reshape(parts, 1).expand(parts, batch)
    elif shape == (batch, 1):
        per_part = target_weight.reshape(parts, batch)
    else:
        return None
    return _f32(per_part.t(), device).reshape(-1)


def _mse_torch(pred_heatmaps, targets, target_weight, use_target_weight, split_sign):
    """The reference's per-part loop (the torch route of both heat-map losses)."""
    criterion = nn.MSELoss(reduction='mean')
    batch, parts = pred_heatmaps.size(0), pred_heatmaps.size(1)
    preds = pred_heatmaps.reshape((batch, parts, -1)).split(1, 1)
    gts = targets.reshape((batch, parts, -1)).split(1, 1)
    loss = 0
    for idx in range(parts):
        p, g = preds[idx].squeeze(), gts[idx].squeeze()
        if use_target_weight:
            term = criterion(p.mul(target_weight[idx]), g.mul(target_weight[idx]))
            loss = loss + (0.5 * term if split_sign else term)
        elif split_sign:
            positive, rest = g > 0, g <= 0
            if not bool(positive.sum() > 0):
                raise LossInputError(_loss.FLAG_TEXT[_loss.FLAG_NO_POSITIVE])
            loss = loss + 0.5 * (criterion(p[positive], g[positive]) + criterion(p[rest], g[rest]))
        else:
            loss = loss + criterion(p, g)
    return loss / parts


class VoxelMSELoss(nn.Module):
    """Mean over parts of the mean squared error of ``outputs['ncf']`` [N,K,...] against ``targets``, each part optionally
    scaled by ``target_weight[part]``."""

    def __init__(self, use_target_weight=False):
        super(VoxelMSELoss, self).__init__()
        self.criterion = nn.MSELoss(reduction='mean')
        self.use_target_weight = use_target_weight

    def forward(self, outputs, targets, target_weight=None, meta_data=None):
        pred = outputs['ncf']
        targets = targets.to(pred.device)
        if _on_hip(pred, targets) and pred.dim() >= 2 and pred.numel() == targets.numel() and pred.numel() > 0:
            batch, parts = pred.size(0), pred.size(1)
            rows = batch * parts
            if not self.use_target_weight:
                return _loss.elementwise(_loss.MSE_ROWS, pred.contiguous(), _f32(targets, pred.device))
            roww = _row_weights(target_weight, parts, batch, pred.device)
            if roww is not None and rows <= _loss.MAX_ROWS:
                return _loss.elementwise(_loss.MSE_ROWS, pred.contiguous(), _f32(targets, pred.device), None, roww, rows=rows)
        return _mse_torch(pred, targets, target_weight, self.use_target_weight, split_sign=False)


class VoxelMSELossWeighted(nn.Module):
    """Per part half the sum of the mean squared errors over the positive and over the non-positive targets (or, with
    ``use_target_weight``, half the weighted mean squared error), averaged over parts.  Every part needs a positive target."""

    def __init__(self, use_target_weight=False):
        super(VoxelMSELossWeighted, self).__init__()
        self.criterion = nn.MSELoss(reduction='mean')
        self.use_target_weight = use_target_weight

    def forward(self, outputs, targets, target_weight=None, meta_data=None):
        pred = outputs['ncf']
        if torch.is_tensor(targets) and targets.device != pred.device:
            targets = targets.to(pred.device)
        if _on_hip(pred, targets) and pred.dim() >= 2 and pred.numel() == targets.numel() and pred.numel() > 0:
            batch, parts = pred.size(0), pred.size(1)
            rows = batch * parts
            if self.use_target_weight:
                roww = _row_weights(target_weight, parts, batch, pred.device)
                if roww is not None and rows <= _loss.MAX_ROWS:
                    return 0.5 * _loss.elementwise(_loss.MSE_ROWS, pred.contiguous(), _f32(targets, pred.device), None, roww, rows=rows)
            elif rows <= _loss.MAX_ROWS:
                _loss.flag_of(pred.device).look(wait=False)
                return _loss.elementwise(_loss.MSE_POSNEG, pred.contiguous(), _f32(targets, pred.device), rows=rows, group=parts,
                                         post_flag=True)
        return _mse_torch(pred, targets, target_weight, self.use_target_weight, split_sign=True)


# ------------------------------------------------------------------------------ occupancy / offset
class OccupancyLoss(nn.Module):
    """Focal loss of the occupancy probabilities ``outputs['occupancy']`` against targets in {-1, 0, 1}; -1 is ignored and
    the mean is over the rest."""

    def __init__(self, use_target_weight=False, gamma=2., alpha=0.25):
        super(OccupancyLoss, self).__init__()
        self.criterion = nn.BCELoss(reduction='mean')
        self.use_target_weight = use_target_weight
        self.gamma = gamma
        self.alpha = alpha

    def forward(self, outputs, targets, target_weight=None, meta_data=None):
        pred = outputs['occupancy']
        gt = targets.to(pred.device)
        if _on_hip(pred, gt) and pred.shape == gt.shape:
            return _loss.elementwise(_loss.OCCUPANCY, pred.contiguous(), _f32(gt, pred.device), p0=self.alpha, p1=self.gamma)
        loss = _focal_terms(pred, gt, self.gamma, self.alpha)
        mask = gt != -1
        if mask.sum() > 0:
            return loss[mask].mean()
        return _zero_of(pred)


class OffsetLoss(nn.Module):
    """L1 mean of ``outputs['offset']`` [N, 3 * parts, H, W, L] against ``meta_data['offset']`` [N, 3, parts, H, W, L] over
    the voxels whose ``meta_data['occupancy']`` [N, H, W, L] is 1."""

    def forward(self, outputs, meta_data):
        pred = outputs['offset']
        gt = meta_data['offset'].to(pred.device)
        occ = meta_data['occupancy']
        parts, h, w, l = gt.shape[2], gt.shape[3], gt.shape[4], gt.shape[5]
        if (_on_hip(pred, gt, occ) and pred.numel() == gt.numel() and pred.numel() > 0 and gt.shape[1] == 3
                and tuple(occ.shape) == (pred.size(0), h, w, l) and pred.size(0) * 3 * parts <= _loss.MAX_ROWS):
            return _loss.elementwise(_loss.OFFSET, pred.contiguous(), _f32(gt, pred.device), _f32(occ, pred.device),
                                     rows=pred.size(0) * 3 * parts, group=3 * parts)
        occupancy = occ.to(pred.device)[:, None, None]
        pred6 = pred.reshape(len(pred), 3, parts, h, w, l)
        loss = F.l1_loss(pred6, gt, reduction='none')
        mask = (occupancy == 1).repeat(1, 3, parts, 1, 1, 1)
        if mask.sum() > 0:
            return loss[mask].mean()
        return _zero_of(pred)


# ------------------------------------------------------------------------------ small heads (a few dozen numbers: torch)
def compute_area_4pts(pts, method='cross-product'):
    """Area of the quadrilaterals ``pts`` [1,N,4,2]: the product of two adjacent edge lengths (``'edge-product'``), or half
    the sum of the cross products at two opposite corners (``'cross-product'``, exact for a convex quadrilateral)."""
    if method == 'edge-product':
        e1 = pts[:, :, 1, :] - pts[:, :, 0, :]
        e2 = pts[:, :, 3, :] - pts[:, :, 0, :]
        return torch.sqrt((e1 ** 2).sum(dim=-1)) * torch.sqrt((e2 ** 2).sum(dim=-1))
    if method == 'cross-product':
        def cross_z(u, v):
            return torch.abs(u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0])
        at0 = cross_z(pts[:, :, 1, :] - pts[:, :, 0, :], pts[:, :, 3, :] - pts[:, :, 0, :])
        at2 = cross_z(pts[:, :, 1, :] - pts[:, :, 2, :], pts[:, :, 3, :] - pts[:, :, 2, :])
        return (at0 + at2) * 0.5
    return None


def compute_IoU_loss_corner(pred, gt):
    """Not built under this name; ``snvc_amd.models.iou_loss.compute_IoU_loss_corner`` computes it."""
    _unbuilt("compute_IoU_loss_corner", _MISSING_UPSTREAM.format("oriented_box_intersection_2d and enclosing_box"))


def approximated_3d_iou_pt(pred, gt, bev_indices):
    """Not built under this name; ``snvc_amd.models.iou_loss.approximated_3d_iou_pt`` computes it."""
    _unbuilt("approximated_3d_iou_pt", _MISSING_UPSTREAM.format("cal_diou"))


class ShapeLoss(nn.Module):
    """L1 mean of ``outputs['shape']`` against ``data_dict['shape'] / scaling``."""

    def __init__(self, scaling=1e4):
        super(ShapeLoss, self).__init__()
        self.scaling = scaling

    def forward(self, outputs, data_dict):
        pred = outputs['shape']
        gt = data_dict['shape'].to(pred.device)
        return F.l1_loss(pred, gt / self.scaling)


class BboxLoss(nn.Module):
    """L1 mean of ``outputs['bbox']`` against ``data_dict['gt_box_local']``, returned as ``{'l1': loss}``.  The '3D' loss of
    ``head_reg_type == 'vector3d'`` is not built under this name; ``snvc_amd.models.iou_loss.Bbox3DLoss`` computes it."""

    def __init__(self, cfg):
        super(BboxLoss, self).__init__()
        if cfg.head_reg_type == 'vector3d':
            _unbuilt("BboxLoss with head_reg_type 'vector3d' ('3D')", _MISSING_UPSTREAM.format("cal_diou (through approximated_3d_iou_pt)"))
        self.bbox_type = '2D'

    def forward(self, outputs, data_dict):
        pred = outputs['bbox']
        gt = data_dict['gt_box_local'].to(pred.device)
        return {'l1': F.l1_loss(pred, gt)}


class CoordinateLoss(nn.Module):
    """L1 mean of the predicted bird's-eye-view corner coordinates ``outputs['coordinates']`` [N,9,2] against the x and z
    columns of ``meta_data['gt_corners_local']`` [N,9,3], the latter normalised to the crop's range with ``normalize_gt``.
    ``enable_IoU=True`` is not built under this name; ``snvc_amd.models.iou_loss.CoordinateIoULoss`` computes it."""

    def __init__(self, cfg, enable_IoU=False, IoU_type='corner', normalize_gt=False):
        super(CoordinateLoss, self).__init__()
        if enable_IoU:
            _unbuilt("CoordinateLoss(enable_IoU=True)", _MISSING_UPSTREAM.format("cal_diou / oriented_box_intersection_2d / enclosing_box"))
        self.enable_IoU = enable_IoU
        self.IoU_type = IoU_type
        self.xmin = cfg.x_range[0]
        self.xrange = cfg.x_range[1] - cfg.x_range[0]
        self.zmin = cfg.z_range[0]
        self.zrange = cfg.z_range[1] - cfg.z_range[0]
        self.normalize_gt = normalize_gt
        self.weight_l1 = 1.

    def forward(self, outputs, meta_data):
        pred = outputs['coordinates'][None]
        corners = meta_data['gt_corners_local'].to(pred.device)
        x, z = corners[None, :, :, 0], corners[None, :, :, 2]
        if self.normalize_gt:
            x = (x - self.xmin) / self.xrange
            z = (z - self.zmin) / self.zrange
        return self.weight_l1 * F.l1_loss(pred, torch.stack([x, z], dim=-1))
