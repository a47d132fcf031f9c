"""The IoU losses that ``snvc_amd.models.loss3d`` leaves unbuilt, over ``snvc_amd.thirdparty.oriented_iou_loss`` (DESIGN.md
"Oriented IoU").  An addition: ``loss3d``'s own names keep raising, and nothing here is served under a ``snvc.*`` name.

  reference (snvc/models/loss3d.py)                    here
  ---------------------------------------------------- ----------------------------------------------
  compute_IoU_loss_corner            :573-601          compute_IoU_loss_corner(pred, gt)
  approximated_3d_iou_pt             :614-636          approximated_3d_iou_pt(pred, gt, bev_indices)
  CoordinateLoss(enable_IoU=True)    :760-799          CoordinateIoULoss(cfg, IoU_type, normalize_gt)
  BboxLoss, head_reg_type 'vector3d' :656-680          Bbox3DLoss(cfg)

On a float32 GPU prediction the pairwise part of each is one HIP launch forward and one backward; the rest (a sigmoid, an L1
mean, the height overlap: a few dozen numbers) is torch.  Other inputs take the torch route of ``oriented_iou_loss``.

Deviation from the reference, deliberate: no function here modifies the caller's tensors.  The reference adds the proposal's
size into ``outputs['bbox']`` and ``gt_box_local`` in place, rescales ``outputs['bbox']`` in place and normalises ``gt`` in
place; here each works on values of its own.
"""
import math

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from .. import _oiou
from ..thirdparty import oriented_iou_loss as oiou
from .loss3d import SELECT_IND1, SELECT_IND2

__all__ = ["compute_IoU_loss_corner", "approximated_3d_iou_pt", "CoordinateIoULoss", "Bbox3DLoss"]


def compute_IoU_loss_corner(pred, gt):
    """DIoU loss of noisy box corners, which may deviate slightly from a rectangle.  ``pred``, ``gt``: [1,N,9,2] part
    coordinates (part 0 is the centre).  The predicted corners are the means of the part pairs (1,2), (3,4), (7,8), (5,6),
    the ground-truth corners are parts 1, 3, 7, 5.  Returns ``(diou_loss [1,N], iou [1,N])``."""
    gt = gt.to(device=pred.device, dtype=pred.dtype)
    pred_corners = 0.5 * (pred[:, :, SELECT_IND1, :] + pred[:, :, SELECT_IND2, :])
    gt_corners = gt[:, :, SELECT_IND1, :]
    lead = pred.shape[:2]
    out = oiou.pair_outputs(_oiou.QUADS, _oiou.DIOU, _oiou.SMALLEST, pred_corners.reshape(-1, 4, 2), gt_corners.reshape(-1, 4, 2),
                            pred[:, :, 0, :].reshape(-1, 2), gt[:, :, 0, :].reshape(-1, 2))
    return out[:, _oiou.LOSS].reshape(lead), out[:, _oiou.IOU].reshape(lead)


def approximated_3d_iou_pt(pred, gt, bev_indices):
    """3D overlap approximated as bird's-eye-view overlap times height overlap.  ``pred``, ``gt``: [N,7] ``centre x / y / z,
    H, W, L, alpha``; ``bev_indices``: the five columns that form the BEV box ``x, y, w, h, alpha``.  Returns the IoU [N]."""
    gt = gt.to(device=pred.device, dtype=pred.dtype)
    _, _, overlap_bev = oiou.cal_diou(pred[None][:, :, bev_indices], gt[None][:, :, bev_indices], return_overlap=True)
    top = torch.min(pred[:, 1] + pred[:, 3] / 2, gt[:, 1] + gt[:, 3] / 2)
    bottom = torch.max(pred[:, 1] - pred[:, 3] / 2, gt[:, 1] - gt[:, 3] / 2)
    overlaps_3d = overlap_bev[0] * torch.clamp(top - bottom, min=0)
    vol_pred = pred[:, 3] * pred[:, 4] * pred[:, 5]
    vol_gt = gt[:, 3] * gt[:, 4] * gt[:, 5]
    return overlaps_3d / torch.clamp(vol_pred + vol_gt - overlaps_3d, min=1e-6)


class CoordinateIoULoss(nn.Module):
    """What ``CoordinateLoss(cfg, enable_IoU=True, ...)`` computes: 0.1 times the L1 mean of ``outputs['coordinates']`` [N,9,2]
    against the x and z columns of ``meta_data['gt_corners_local']`` [N,9,3], plus the mean DIoU loss -- of the corners
    (``IoU_type='corner'``) or of the box decoded from ``outputs['bbox']`` [N,5] against ``meta_data['gt_box_local']`` [N,5]
    (``'bbox'``)."""

    def __init__(self, cfg, IoU_type='corner', normalize_gt=False):
        super(CoordinateIoULoss, self).__init__()
        if IoU_type not in ('corner', 'bbox'):
            raise ValueError(f"IoU_type must be 'corner' or 'bbox', got {IoU_type!r}")
        self.enable_IoU = True
        self.IoU_type = IoU_type
        self.xmin = cfg.x_range[0]
        self.xrange = cfg.x_range[1] - cfg.x_range[0]
        self.zmin = cfg.z_range[0]
        self.zrange = cfg.z_range[1] - cfg.z_range[0]
        self.normalize_gt = normalize_gt
        self.weight_l1 = 0.1

    def decode_bbox(self, raw):
        """``outputs['bbox']`` [N,5] -> ``x, y, w, h, alpha``: centre in +-range, size in (0, range), angle in (0, 2 pi)."""
        s = torch.sigmoid(raw)
        return torch.stack([(s[:, 0] * 2 - 1) * self.xrange, (s[:, 1] * 2 - 1) * self.zrange, s[:, 2] * self.xrange,
                            s[:, 3] * self.zrange, s[:, 4] * (math.pi * 2)], dim=1)

    def forward(self, outputs, meta_data):
        pred = outputs['coordinates'][None]
        corners = meta_data['gt_corners_local'].to(device=pred.device, dtype=pred.dtype)
        x, z = corners[None, :, :, 0], corners[None, :, :, 2]
        if self.normalize_gt:
            x = (x - self.xmin) / self.xrange
            z = (z - self.zmin) / self.zrange
        gt = torch.stack([x, z], dim=-1)
        loss = self.weight_l1 * F.l1_loss(pred, gt)
        if self.IoU_type == 'bbox':
            gt_bbox = meta_data['gt_box_local'].to(device=pred.device, dtype=pred.dtype)
            iou_loss, _ = oiou.cal_diou(self.decode_bbox(outputs['bbox'])[None], gt_bbox[None])
        else:
            iou_loss, _ = compute_IoU_loss_corner(pred, gt)
        return loss + iou_loss.mean()


class Bbox3DLoss(nn.Module):
    """``BboxLoss``'s '3D' branch (``head_reg_type == 'vector3d'``) without the regression mask: ``outputs['bbox'][:, :7]`` and
    ``data_dict['gt_box_local']`` [N,7] are ``x, y, z, dH, dW, dL, alpha``, the sizes relative to the proposals
    ``data_dict['samples']`` ([N,>=3] ``h, w, l, ...``: an array, a tensor or a list of rows).  Returns ``{'sl1': half the
    smooth-L1 mean (beta 0.2), 'IoU3D': mean of 1 - approximated 3D IoU}``."""

    def __init__(self, cfg=None):
        super(Bbox3DLoss, self).__init__()
        self.bbox_type = '3D'
        self.beta = 0.2
        self.indices = [0, 2, 5, 4, 6]
        self.use_reg_mask = False

    def forward(self, outputs, data_dict):
        if self.use_reg_mask:
            raise NotImplementedError("Bbox3DLoss with use_reg_mask is not built: selecting the boxes by their IoU with the proposals "
                                      "needs their count on the host, a synchronisation in every step")
        pred = outputs['bbox'][:, :7]
        gt = data_dict['gt_box_local'].to(device=pred.device, dtype=pred.dtype)
        samples = data_dict['samples']
        if not torch.is_tensor(samples):
            samples = torch.from_numpy(np.vstack(samples) if isinstance(samples, list) else np.asarray(samples))
        size = torch.zeros_like(pred)
        size[:, 3:6] = samples[:, :3].to(device=pred.device, dtype=pred.dtype)
        pred, gt = pred + size, gt + size
        iou3d = approximated_3d_iou_pt(pred, gt, self.indices)
        return {'sl1': F.smooth_l1_loss(pred, gt, beta=self.beta) * 0.5, 'IoU3D': (1 - iou3d).mean()}
