"""Device-side producers of the path's coordinates and of its training targets.

Drop-in for the three ``refinementDataset`` methods that turn box proposals into the
``grid_proj_left`` / ``grid_proj_right`` tensors VernierScale consumes
(snvc/dataset/KITTIRefinement_dataset.py:267-282 ``_init_3d_grid``, :828-846 ``_to_cam``,
:848-868 ``_generate_grid_proj``).  The reference computes them with numpy float64 on the host
(786 k points x 2 cameras per instance) and ships 2 x 6.3 MB per instance to the GPU; here they are
generated where they are used, from 31 doubles per instance.

``TargetGenerator`` does the same for what the losses compare against: ``_generate_displacement_field`` (:870-903), the
per-part heat maps, the occupancy grid and the part positions, from the boxes and the frame's point cloud.

``RoICropper`` is the producer in front of both: ``_generate_rois`` (:555-621), the left and right image patches HRNet reads
and the crop transforms ``GridProjector`` takes, from the stereo pair and the boxes, without cv2.
"""
import ctypes

import numpy as np
import torch

from . import _lib, _roicrop, _targets
from ._lib import check


class GridProjector:
    """``cfg`` needs ``x_range``, ``y_range``, ``z_range`` and ``grid_resolution`` = (nh, nw, nl),
    the attributes ``_init_3d_grid`` reads (KITTIRefinement_dataset.py:271-276)."""

    def __init__(self, cfg):
        self.ranges = np.array([cfg.x_range[0], cfg.x_range[1], cfg.y_range[0], cfg.y_range[1],
                                cfg.z_range[0], cfg.z_range[1]], dtype=np.float64)
        self.nh, self.nw, self.nl = (int(v) for v in cfg.grid_resolution)

    @property
    def num_points(self):
        return self.nh * self.nw * self.nl

    def generate(self, samples, P_left, P_right, trans_l, trans_r, device, with_grid_3d=False):
        """samples [N,7] (h,w,l,x,y,z,ry); P_left/P_right [3,4] (calib_left.P / calib_right.P);
        trans_l/trans_r [N,2,3] (meta_roi['trans_l'/'trans_r']).  numpy or torch inputs.
        Returns (coord_l, coord_r[, grid_3d]) like ``_generate_grid_proj``: float32 [N,2,V] on
        ``device`` (and float64 [N,V,3])."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("GridProjector.generate needs a GPU device: Not implemented on the CPU")

        def dev64(a, shape):
            t = torch.as_tensor(np.asarray(a, dtype=np.float64) if not torch.is_tensor(a) else a, dtype=torch.float64)
            t = t.reshape(shape).contiguous()
            return t.to(device)

        n = len(samples)
        s = dev64(samples, (n, 7))
        pl, pr = dev64(P_left, (3, 4)), dev64(P_right, (3, 4))
        tl, tr = dev64(trans_l, (n, 2, 3)), dev64(trans_r, (n, 2, 3))
        v = self.num_points
        out_l = torch.empty((n, 2, v), dtype=torch.float32, device=device)
        out_r = torch.empty_like(out_l)
        g3 = torch.empty((n, v, 3), dtype=torch.float64, device=device) if with_grid_3d else None
        if n:
            p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)  # noqa: E731
            with torch.cuda.device(device):
                check(_lib.lib().snvc_grid_projection(
                    p(s), p(pl), p(pr), p(tl), p(tr), self.ranges.ctypes.data_as(ctypes.c_void_p), self.nh, self.nw,
                    self.nl, p(out_l), p(out_r), p(g3), n,
                    ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "snvc_grid_projection")
        return (out_l, out_r, g3) if with_grid_3d else (out_l, out_r)


class TargetGenerator:
    """Device-side ``refinementDataset._generate_displacement_field`` (KITTIRefinement_dataset.py:870-903).

    ``cfg`` needs what the reference reads from its cfg / ``df_params`` (:88-95): ``grid_resolution`` = (nh, nw, nl),
    ``spacing`` = (dy, dx, dz), ``grid_range`` (``df_params['range']``), ``x_range`` / ``y_range`` / ``z_range``, ``sigma``
    (a positive integer), ``num_parts`` (at most 9) and ``grid_type`` ('2D' or '3D')."""

    def __init__(self, cfg):
        assert cfg.num_parts <= 9, "Only support less than or equal to 9 object parts"
        if isinstance(cfg.num_parts, bool) or int(cfg.num_parts) != cfg.num_parts or cfg.num_parts < 1:
            raise ValueError(f"num_parts must be an integer in 1 .. 9, got {cfg.num_parts!r}")
        if isinstance(cfg.sigma, bool) or not isinstance(cfg.sigma, (int, np.integer)) or cfg.sigma < 1:
            raise ValueError(f"sigma must be a positive integer (the heat-map window is 6 sigma + 1 cells), got {cfg.sigma!r}")
        if cfg.grid_type not in ("2D", "3D"):
            raise ValueError(f"grid_type must be '2D' or '3D', got {cfg.grid_type!r}")
        self.nh, self.nw, self.nl = (int(v) for v in cfg.grid_resolution)
        self.num_parts, self.sigma, self.grid_type = int(cfg.num_parts), int(cfg.sigma), cfg.grid_type
        spacing = np.asarray(cfg.spacing, dtype=np.float64).reshape(3)
        grid_range = np.asarray(cfg.grid_range, dtype=np.float64).reshape(3)
        if min(self.nh, self.nw, self.nl) < 1 or not (spacing > 0).all():
            raise ValueError("grid_resolution and spacing must be positive")
        g = self.grid = _targets.TargetsGrid()
        g.nh, g.nw, g.nl, g.num_parts, g.sigma, g.grid_type = self.nh, self.nw, self.nl, self.num_parts, self.sigma, int(self.grid_type[0])
        g.spacing[:], g.grid_range[:] = spacing.tolist(), grid_range.tolist()
        g.ranges[:] = [float(v) for v in (*cfg.x_range, *cfg.y_range, *cfg.z_range)]

    def field_shape(self, n):
        if self.grid_type == "2D":
            return (n, self.num_parts, self.nl, self.nw)
        return (n, self.num_parts, self.nh, self.nw, self.nl)

    def generate(self, samples, gt_label, points, device, velo_to_rect=None, frame=None, point_offsets=None,
                 with_point_masks=False):
        """samples [N,7] (h,w,l,x,y,z,ry); gt_label [7], or [N,7] for one label per sample; points [P,3] float32 or float64,
        in rectified-camera coordinates, or in Velodyne coordinates with velo_to_rect = (V2C [3,4], R0 [3,3]).  frame [N] and
        point_offsets [F+1] (host integers) give sample n the rows point_offsets[frame[n]] : point_offsets[frame[n] + 1].
        numpy or torch inputs.  Returns (fields, meta) like ``_generate_displacement_field``, on ``device``: fields float32
        [N,parts,nl,nw] ('2D') or [N,parts,nh,nw,nl] ('3D'); meta['occupancy'] float32 [N,nh,nw,nl] in {-1, 0, 1};
        meta['gt_corners_local'] float32 [N,parts,3]; with_point_masks adds the bool [N,Pmax] meta['in_roi'] and
        meta['in_fg'] (row n indexes sample n's rows of ``points``), the reference's pc_in_roi / pc_in_roi_fg lists."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("TargetGenerator.generate needs a GPU device: Not implemented on the CPU")

        def dev64(a, shape):
            t = torch.as_tensor(np.asarray(a, dtype=np.float64) if not torch.is_tensor(a) else a, dtype=torch.float64)
            return t.reshape(shape).contiguous().to(device)

        n = len(samples)
        if n > _targets.MAX_SAMPLES:
            raise RuntimeError(f"TargetGenerator.generate: {n} samples in one call is above the limit of {_targets.MAX_SAMPLES}")
        s = dev64(samples, (n, 7))
        lab = torch.as_tensor(np.asarray(gt_label, dtype=np.float64)) if not torch.is_tensor(gt_label) else gt_label
        if lab.numel() == 7:
            lab = lab.reshape(1, 7).expand(n, 7)
        elif lab.numel() != 7 * n:
            raise ValueError(f"gt_label must be [7] or [{n},7], got {tuple(lab.shape)}")
        lab = dev64(lab, (n, 7))
        pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
        if pts.dim() != 2 or pts.shape[1] != 3 or pts.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"points must be a float32 or float64 [P,3] array, got {pts.dtype} {tuple(pts.shape)}")
        pts = pts.contiguous().to(device)
        total = pts.shape[0]
        slices, pmax = None, total
        if (frame is None) != (point_offsets is None):
            raise ValueError("frame and point_offsets come together or not at all")
        if frame is not None:
            fr = np.asarray(frame.cpu() if torch.is_tensor(frame) else frame, dtype=np.int64).reshape(n)
            off = np.asarray(point_offsets.cpu() if torch.is_tensor(point_offsets) else point_offsets, dtype=np.int64).reshape(-1)
            if off.size < 2 or off[0] < 0 or off[-1] > total or (np.diff(off) < 0).any():
                raise ValueError(f"point_offsets must ascend within 0 .. {total}")
            if n and (fr.min() < 0 or fr.max() > off.size - 2):
                raise ValueError(f"frame must index the {off.size - 1} frames of point_offsets")
            host = np.stack([off[fr], off[fr + 1] - off[fr]], axis=1)
            pmax = int(host[:, 1].max()) if n else 0
            slices = torch.from_numpy(host).contiguous().to(device)
        v2r = None
        if velo_to_rect is not None:
            v2c, r0 = velo_to_rect
            v2r = torch.cat([dev64(v2c, (12,)), dev64(r0, (9,))])

        fields = torch.empty(self.field_shape(n), dtype=torch.float32, device=device)
        corners = torch.empty((n, self.num_parts, 3), dtype=torch.float32, device=device)
        occ = torch.empty((n, self.nh, self.nw, self.nl), dtype=torch.float32, device=device)
        meta = {"occupancy": occ, "gt_corners_local": corners}
        in_roi = in_fg = None
        if with_point_masks:
            in_roi = torch.empty((n, pmax), dtype=torch.bool, device=device)
            in_fg = torch.empty((n, pmax), dtype=torch.bool, device=device)
            meta["in_roi"], meta["in_fg"] = in_roi, in_fg
        if n:
            p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else ctypes.c_void_p(0)  # noqa: E731
            with torch.cuda.device(device):
                L = _targets.lib()
                ws = torch.empty(L.snvc_targets_workspace_bytes(n), dtype=torch.uint8, device=device)
                stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                g = ctypes.byref(self.grid)
                check(L.snvc_targets_fields(g, p(s), p(lab), n, p(ws), p(fields), p(corners), stream), "snvc_targets_fields")
                check(L.snvc_targets_occupancy(g, p(s), p(lab), n, p(pts), int(pts.dtype == torch.float64), total, p(slices), pmax,
                                               p(v2r), p(ws), p(occ), p(in_roi), p(in_fg), stream), "snvc_targets_occupancy")
        return fields, meta


class RoICropper:
    """Device-side ``refinementDataset._generate_rois`` (KITTIRefinement_dataset.py:555-621) with the ``ToTensor`` + ``Normalize``
    that follows it: box -> nine projected key points -> crop centre and size -> 2x3 affine -> bilinear warp of the left and the
    right image -> normalised planar float32.  The arithmetic that stands in for cv2 is specified in DESIGN.md ("RoI crops").

    ``cfg`` needs ``resolution`` = (Wr, Hr), width first as in the reference's ``roi_params``; ``aspect_ratio`` (height / width
    the crop is grown to); ``grid_range`` (``df_params['range']``); ``img_mean`` and ``img_std``, three values each, for pixels
    scaled to 0 .. 1."""

    INTERPOLATIONS = {"fixed5": _roicrop.FIXED5, "exact": _roicrop.EXACT}

    def __init__(self, cfg):
        res = tuple(cfg.resolution)
        if len(res) != 2 or any(isinstance(v, bool) or int(v) != v for v in res):
            raise ValueError(f"resolution must be two integers (width, height), got {cfg.resolution!r}")
        self.out_w, self.out_h = (int(v) for v in res)
        if min(self.out_w, self.out_h) < 1:
            raise ValueError(f"resolution must be positive, got {cfg.resolution!r}")
        if max(self.out_w, self.out_h) > _roicrop.MAX_SIDE:
            raise ValueError(f"resolution must not exceed {_roicrop.MAX_SIDE} a side, got {cfg.resolution!r}")
        self.aspect_ratio = float(cfg.aspect_ratio)
        if not (self.aspect_ratio > 0 and np.isfinite(self.aspect_ratio)):
            raise ValueError(f"aspect_ratio must be positive, got {cfg.aspect_ratio!r}")
        self.grid_range = np.asarray(cfg.grid_range, dtype=np.float64).reshape(3)
        if not ((self.grid_range > 0).all() and np.isfinite(self.grid_range).all()):
            raise ValueError(f"grid_range must be positive, got {cfg.grid_range!r}")
        mean = torch.as_tensor(np.asarray(cfg.img_mean, dtype=np.float64).reshape(3), dtype=torch.float32)
        std = torch.as_tensor(np.asarray(cfg.img_std, dtype=np.float64).reshape(3), dtype=torch.float32)
        if (std == 0).any():
            raise ValueError(f"img_std must not contain 0 (Normalize divides by it), got {cfg.img_std!r}")
        # ToTensor (uint8 -> float32, div 255) and Normalize (sub mean, div std) on all 256 x 3 inputs, with torch's own CPU
        # operations: the kernel only looks the result up, so its bits are torch's
        levels = torch.arange(256, dtype=torch.uint8).to(torch.float32).div(255)
        self.norm_table = levels.reshape(1, 256).repeat(3, 1).sub_(mean.reshape(3, 1)).div_(std.reshape(3, 1)).contiguous()
        self._tables = {}

    def _table_on(self, device):
        if device not in self._tables:
            self._tables[device] = self.norm_table.to(device)
        return self._tables[device]

    @staticmethod
    def _images(imgs, device):
        """uint8 [H,W,3] device tensors (kept alive by the caller until the launch is queued) and their descriptor rows."""
        held, rows = [], []
        for im in imgs:
            t = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError(f"an image must be uint8 [H,W,3], got {t.dtype} {tuple(t.shape)}")
            h, w = int(t.shape[0]), int(t.shape[1])
            if min(h, w) < 1 or max(h, w) > _roicrop.MAX_SIDE:
                raise ValueError(f"image sides must be within 1 .. {_roicrop.MAX_SIDE}, got {h} x {w}")
            t = t.to(device)
            if t.stride(2) != 1 or t.stride(1) != 3 or (h > 1 and t.stride(0) < 3 * w):
                t = t.contiguous()          # rows of packed 3-byte pixels; any row stride from 3 W up is read as it is
            held.append(t)
            rows.append((ctypes.c_void_p(t.data_ptr()).value, h | (w << 32), t.stride(0) if h > 1 else 3 * w))   # for the kernel
        return held, rows

    def generate(self, samples, left_img, right_img, P_left, P_right, device, frame=None, raw=False, interpolation="fixed5",
                 channel_order="rgb"):
        """samples [N,7] (h,w,l,x,y,z,ry); left_img / right_img: uint8 [H,W,3] tensors or arrays, or lists of F of them with
        frame [N] (host integers) naming the one sample n is cropped from (frames may differ in size; host arrays are uploaded
        once per call, device tensors are read where they are, with their row stride); P_left / P_right [3,4]
        (calib_left.P / calib_right.P), or [F,3,4] for one calibration per frame.  numpy or torch inputs.
        interpolation: 'fixed5', the bilinear warp with source coordinates in 1/32 px and integer weights, or 'exact', float64
        coordinates and float32 weights.  channel_order 'bgr' swaps channels 0 and 2 on the read.
        Returns (left_rois, right_rois, meta) like ``_generate_rois`` followed by the normalising transform, on ``device``:
        rois float32 [N,3,Hr,Wr] (raw=True: the warp's uint8, not normalised); meta['trans_l'] / ['trans_r'] float64 [N,2,3],
        meta['kpts_2d_l'] / ['kpts_2d_r'] float64 [N,9,2], meta['kpts_2d_l_local'] / ['kpts_2d_r_local'] float32 [N,9,2]."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("RoICropper.generate needs a GPU device: Not implemented on the CPU")
        if interpolation not in self.INTERPOLATIONS:
            raise ValueError(f"interpolation must be 'fixed5' or 'exact', got {interpolation!r}")
        if channel_order not in ("rgb", "bgr"):
            raise ValueError(f"channel_order must be 'rgb' or 'bgr', got {channel_order!r}")

        def dev64(a, shape):
            t = torch.as_tensor(np.asarray(a, dtype=np.float64) if not torch.is_tensor(a) else a, dtype=torch.float64)
            return t.reshape(shape).contiguous().to(device)

        n = len(samples)
        if n > _roicrop.MAX_SAMPLES:
            raise RuntimeError(f"RoICropper.generate: {n} samples in one call is above the limit of {_roicrop.MAX_SAMPLES}")
        lefts = list(left_img) if isinstance(left_img, (list, tuple)) else [left_img]
        rights = list(right_img) if isinstance(right_img, (list, tuple)) else [right_img]
        nf = len(lefts)
        if nf < 1 or len(rights) != nf:
            raise ValueError(f"left_img and right_img must hold the same number of frames, got {nf} and {len(rights)}")
        if nf > 1 and frame is None:
            raise ValueError("several frames need frame [N], the frame each sample is cropped from")
        fr = None
        if frame is not None:
            host = np.asarray(frame.cpu() if torch.is_tensor(frame) else frame, dtype=np.int64).reshape(n)
            if n and (host.min() < 0 or host.max() > nf - 1):
                raise ValueError(f"frame must index the {nf} frames given, got values in {host.min()} .. {host.max()}")
            fr = torch.from_numpy(host.astype(np.int32)).to(device)

        def proj(P):
            t = dev64(P, (-1, 12))
            if t.shape[0] not in (1, nf):
                raise ValueError(f"a projection must be [3,4] or [{nf},3,4], got {t.shape[0]} matrices")
            return t.expand(nf, 12).contiguous()

        with torch.cuda.device(device):
            s = dev64(samples, (n, 7))
            pl, pr = proj(P_left), proj(P_right)
            held_l, rows_l = self._images(lefts, device)
            held_r, rows_r = self._images(rights, device)
            desc = torch.tensor(rows_l + rows_r, dtype=torch.int64).reshape(2, nf, 3).to(device)
            table = None if raw else self._table_on(device)
            # everything below is queued on the current stream; nothing waits for the device
            rois = [torch.empty((n, 3, self.out_h, self.out_w), dtype=torch.uint8 if raw else torch.float32, device=device)
                    for _ in range(2)]
            trans = [torch.empty((n, 2, 3), dtype=torch.float64, device=device) for _ in range(2)]
            kpts = [torch.empty((n, 9, 2), dtype=torch.float64, device=device) for _ in range(2)]
            local = [torch.empty((n, 9, 2), dtype=torch.float32, device=device) for _ in range(2)]
            if n:
                L = _roicrop.lib()
                cfg = _roicrop.RoICropConfig()
                cfg.out_w, cfg.out_h, cfg.interpolation = self.out_w, self.out_h, self.INTERPOLATIONS[interpolation]
                cfg.swap_rb, cfg.raw, cfg.aspect_ratio = int(channel_order == "bgr"), int(bool(raw)), self.aspect_ratio
                cfg.grid_range[:] = self.grid_range.tolist()
                ws = torch.empty(L.snvc_roicrop_workspace_bytes(n), dtype=torch.uint8, device=device)
                p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)  # noqa: E731
                check(L.snvc_roicrop(ctypes.byref(cfg), p(desc[0]), p(desc[1]), nf, p(fr), p(s), p(pl), p(pr), n, p(table), p(ws),
                                     p(rois[0]), p(rois[1]), p(trans[0]), p(trans[1]), p(kpts[0]), p(kpts[1]), p(local[0]), p(local[1]),
                                     ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)), "snvc_roicrop")
            del held_l, held_r      # the allocator hands their memory out again in stream order, after the warp
        meta = {"trans_l": trans[0], "trans_r": trans[1], "kpts_2d_l": kpts[0], "kpts_2d_r": kpts[1],
                "kpts_2d_l_local": local[0], "kpts_2d_r_local": local[1]}
        return rois[0], rois[1], meta
