"""One refinement pass, from a decoded stereo pair and box proposals to refined boxes, as one object: the chain of
INTEGRATION.md "The input chain without cv2" (``RoICropper -> GridProjector -> VernierScale -> decode.refine_boxes``) with every
stage on the device and device tensors handed from one to the next.
"""
import numpy as np
import torch

from . import decode
from .geometry import GridProjector, RoICropper


class Refiner:
    """``model`` is a ``VernierScale`` on a GPU, in eval mode; ``roi_cfg`` is what ``RoICropper`` reads (``resolution``,
    ``aspect_ratio``, ``grid_range``, ``img_mean``, ``img_std``); ``grid_cfg`` (default ``model.cfg``) is what ``GridProjector``
    and ``decode.grid_bev_flat`` read (``x_range``, ``y_range``, ``z_range``, ``grid_resolution``); ``filter_3d`` is None or a
    ``decode.Filter``.  Nothing is stored on the model."""

    def __init__(self, model, roi_cfg, grid_cfg=None, filter_3d=None):
        self.model = model
        self.grid_cfg = model.cfg if grid_cfg is None else grid_cfg
        self.cropper = RoICropper(roi_cfg)
        self.projector = GridProjector(self.grid_cfg)
        self.filter_3d = filter_3d
        self.device = next(model.parameters()).device
        self.grid = torch.from_numpy(decode.grid_bev_flat(self.grid_cfg)).to(self.device)

    def refine(self, samples, left_img, right_img, P_left, P_right, frame=None, iterations=1, **crop_kw):
        """samples [N,7] (h,w,l,x,y,z,ry), numpy or torch; left_img / right_img, frame and ``crop_kw`` as
        ``RoICropper.generate`` takes them (host images are uploaded once, before the first pass); P_left / P_right [3,4].
        Crop, grid projection, ``model(...)`` under ``no_grad`` and ``decode.refine_boxes`` (with the model's coordinates when
        it returns them), ``iterations`` times: the 'all_parts' boxes of one pass ('one_part' for a one-part model) are the
        next pass's proposals, as the device tensor they are; a rejected instance's row there is its unchanged proposal.
        Returns the last pass's ``refine_boxes`` dict, 'keep_flags' being the AND over the passes.  Between the uploads and the
        returned dict nothing is copied to the host and nothing waits for the device beyond what the producers do themselves."""
        if iterations < 1:
            raise ValueError(f"iterations must be at least 1, got {iterations!r}")

        def on_device(im):
            return (im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))).to(self.device)

        left_img, right_img = ([on_device(im) for im in imgs] if isinstance(imgs, (list, tuple)) else on_device(imgs)
                               for imgs in (left_img, right_img))
        keep = None
        for _ in range(iterations):
            left, right, meta = self.cropper.generate(samples, left_img, right_img, P_left, P_right, self.device, frame=frame, **crop_kw)
            coord_l, coord_r = self.projector.generate(samples, P_left, P_right, meta["trans_l"], meta["trans_r"], self.device)
            with torch.no_grad():
                out = self.model(left, right, coord_l, coord_r)
            result = decode.refine_boxes(self.grid_cfg, out["ncf"], samples, self.grid, self.filter_3d, coordinates=out.get("coordinates"))
            keep = result["keep_flags"] if keep is None else keep & result["keep_flags"]
            samples = result["all_parts"] if result["all_parts"] is not None else result["one_part"]
        result["keep_flags"] = keep
        return result
