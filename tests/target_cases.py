"""Inputs of the training-target tests (snvc_amd.geometry.TargetGenerator), shared by tests/golden/make_golden_targets.py
(the generator, which needs the reference) and the tests (which need only tests/golden/targets_ref.npz).

Nothing is stored but results: boxes are written out below and point clouds are re-drawn from ``numpy.random.default_rng``
with fixed seeds.  The geometry is the calibration-free one of ``golden_cases.grid_proj_case``.  The generator asserts for
every small case that no tested point lies within 1e-7 m of a plane it is tested against and that no floored index
coordinate lies within 1e-7 of an integer, so a float64 implementation with another summation order takes the same
decisions.
"""
import os
import types

import numpy as np

GOLDEN_NPZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "targets_ref.npz")

X_RANGE, Y_RANGE, Z_RANGE = (-1.6, 1.6), (-0.8, 0.8), (-2.4, 2.4)
EXTENT = (Y_RANGE[1] - Y_RANGE[0], X_RANGE[1] - X_RANGE[0], Z_RANGE[1] - Z_RANGE[0])     # (h, w, l)

LABEL_A = np.array([1.50, 1.60, 3.95, 2.35, 1.62, 14.6, -1.45])
LABEL_B = np.array([1.47, 1.66, 4.21, -3.10, 1.71, 21.3, 0.37])


def make_cfg(grid, sigma, parts, grid_type, spacing=None, grid_range=None):
    """The attributes TargetGenerator (and the reference's dataset) reads.  By default the spacing is the step of the
    sampling grid and grid_range its extent, so every index of a point inside the RoI box lies in 0 .. extent - 1."""
    if spacing is None:
        spacing = tuple(EXTENT[a] / (grid[a] - 1) for a in range(3))
    return types.SimpleNamespace(grid_resolution=tuple(grid), spacing=tuple(spacing), grid_range=list(grid_range or EXTENT),
                                 x_range=X_RANGE, y_range=Y_RANGE, z_range=Z_RANGE, sigma=sigma, num_parts=parts, grid_type=grid_type)


def _near(label, d_xyz, d_ry, d_dim=(0.02, 0.03, -0.07)):
    s = label.copy()
    s[:3] += d_dim
    s[3:6] += d_xyz
    s[6] += d_ry
    return s


def _cloud(label, count, seed, half=3.0, dtype=np.float64):
    """`count` points spread evenly over a cube of 2 * half metres around the label's centre."""
    r = np.random.default_rng(seed)
    centre = label[3:6] - np.array([0.0, 0.5 * label[0], 0.0])
    return (centre + r.uniform(-half, half, (count, 3))).astype(dtype)


# sample 0: label close by, every part on the grid and the centre's window whole (a car's corners sit within 3 sigma of the
# border of a 16-cell axis, so their windows are clipped even here); 1: label offset, several windows clipped by the border and
# some off the grid; 2: label several metres away, every window (and the box) misses the grid
SAMPLES_A = np.stack([_near(LABEL_A, (-0.25, 0.03, -0.40), -0.07),
                      _near(LABEL_A, (0.70, -0.25, 0.90), 0.11),
                      _near(LABEL_A, (5.20, 0.10, -6.70), 0.40)])
SAMPLES_B = np.stack([_near(LABEL_B, (0.31, -0.05, 0.22), 0.05)])


def _local_to_cam(sample, grid_range, local):
    """Camera coordinates of a point given in the RoI box's frame (x: width, y: height, z: length)."""
    ry = sample[6]
    rot = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    basis = rot @ np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]]).T
    centre = np.array([sample[3], sample[4] - 0.5 * grid_range[0], sample[5]])
    return centre + np.asarray(local) @ basis.T


VELO_V2C = np.array([[7.533745e-03, -9.999714e-01, -6.166020e-04, -4.069766e-03],
                     [1.480249e-02, 7.280733e-04, -9.998902e-01, -7.631618e-02],
                     [9.998621e-01, 7.523790e-03, 1.480755e-02, -2.717806e-01]])
VELO_R0 = np.array([[9.999239e-01, 9.837760e-03, -7.445048e-03],
                    [-9.869795e-03, 9.999421e-01, -4.278459e-03],
                    [7.402527e-03, 4.351614e-03, 9.999631e-01]])


def case(name):
    """dict(cfg, samples [N,7], label [7] or [N,7], points [P,3], and for some: frame, point_offsets, velo_to_rect)."""
    if name in ("small2d", "small3d"):
        return dict(cfg=make_cfg((16, 32, 48), 2, 9, name[-2:].upper()), samples=SAMPLES_A, label=LABEL_A,
                    points=_cloud(LABEL_A, 20000, 11))
    if name in ("odd2d", "odd3d"):
        return dict(cfg=make_cfg((5, 7, 11), 1, 1, name[-2:].upper()), samples=SAMPLES_A[:2], label=LABEL_A,
                    points=_cloud(LABEL_A, 3000, 12, dtype=np.float32))
    if name == "quirks":
        # spacing 0.1 and an RoI box 10 % larger than resolution x spacing: along the width, local -0.80 gives index -1
        # (numpy counts it from the end) and local +0.87 gives index 16, the extent (clamped to the last cell)
        grid, spacing = (8, 16, 24), (0.1, 0.1, 0.1)
        grid_range = [0.88, 1.76, 2.64]
        sample = np.array([1.52, 1.63, 3.88, 2.10, 1.65, 14.2, -1.52])
        label = np.array([2.00, 3.60, 4.40, 2.12, 1.93, 14.25, -1.50])
        hand = np.stack([_local_to_cam(sample, grid_range, (-0.80, 0.013, 0.021)),
                         _local_to_cam(sample, grid_range, (0.87, -0.017, -0.033)),
                         _local_to_cam(sample, grid_range, (0.012, -0.42, 0.044)),
                         _local_to_cam(sample, grid_range, (-0.023, 0.031, 1.31))])
        return dict(cfg=make_cfg(grid, 2, 9, "3D", spacing, grid_range), samples=sample[None], label=label,
                    points=np.concatenate([hand, _cloud(sample, 2000, 13, half=1.5)]), hand_points=4)
    if name == "frames":
        # two frames in one call, one label per sample; the golden is made one frame at a time
        pa, pb = _cloud(LABEL_A, 8000, 14), _cloud(LABEL_B, 5000, 15)
        return dict(cfg=make_cfg((16, 32, 48), 2, 9, "2D"), samples=np.concatenate([SAMPLES_A[:2], SAMPLES_B]),
                    label=np.stack([LABEL_A, LABEL_A, LABEL_B]), points=np.concatenate([pa, pb]),
                    frame=np.array([0, 0, 1]), point_offsets=np.array([0, 8000, 13000]))
    if name == "velo":
        # float32 Velodyne points: rectified points around the label taken back through the calibration
        rect = _cloud(LABEL_A, 6000, 16, half=2.5)
        ref = rect @ np.linalg.inv(VELO_R0).T
        velo = (ref - VELO_V2C[:, 3]) @ np.linalg.inv(VELO_V2C[:, :3]).T
        return dict(cfg=make_cfg((8, 16, 24), 2, 4, "3D"), samples=SAMPLES_A[:2], label=LABEL_A, points=velo.astype(np.float32),
                    velo_to_rect=(VELO_V2C, VELO_R0))
    if name == "full":
        return dict(cfg=make_cfg((32, 128, 192), 2, 9, "3D"), samples=SAMPLES_A[:2], label=LABEL_A,
                    points=_cloud(LABEL_A, 120000, 17))
    raise KeyError(name)


SMALL = ("small2d", "small3d", "odd2d", "odd3d", "quirks", "frames", "velo")     # stored in full
FULL = "full"                                                                    # stored as counts, sums and subsamples
FULL_STRIDE = (3, 5, 7)                                                          # of the (nh, nw, nl) axes


def field_shape(cfg, n):
    nh, nw, nl = cfg.grid_resolution
    return (n, cfg.num_parts, nl, nw) if cfg.grid_type == "2D" else (n, cfg.num_parts, nh, nw, nl)


def expected_arrays(name):
    """name -> (shape, dtype) of every array the golden file holds for the case."""
    c = case(name)
    cfg, n = c["cfg"], len(c["samples"])
    nh, nw, nl = cfg.grid_resolution
    if name == FULL:
        sub = tuple(-(-e // s) for e, s in zip((nh, nw, nl), FULL_STRIDE))
        return {"occ_counts": ((n, 3), np.int64), "occ_sub": ((n,) + sub, np.int8), "field_sums": ((n, cfg.num_parts), np.float64),
                "field_sub": ((n, cfg.num_parts) + sub, np.float32), "corners": ((n, cfg.num_parts, 3), np.float32)}
    pmax = len(c["points"]) if "frame" not in c else int(np.diff(c["point_offsets"]).max())
    bits = -(-pmax // 8)
    return {"fields": (field_shape(cfg, n), np.float32), "occupancy": ((n, nh, nw, nl), np.int8),
            "corners": ((n, cfg.num_parts, 3), np.float32), "in_roi": ((n, bits), np.uint8), "in_fg": ((n, bits), np.uint8)}


def load_golden():
    return np.load(GOLDEN_NPZ)
