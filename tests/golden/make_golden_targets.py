"""Writes tests/golden/targets_ref.npz: what the reference's own data loader computes for the cases of tests/target_cases.py.

    python tests/golden/make_golden_targets.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Needs the reference checkout (numpy on the CPU); the tests need only the file.  The reference's methods are called unbound on
a SimpleNamespace that carries cfg / df_params: refinementDataset._generate_displacement_field's loop body
(_construct_neural_confidence_field and _get_point_cloud per sample, KITTIRefinement_dataset.py:888-902), with the grid
points of _to_cam and, for the Velodyne case, Calibration.project_velo_to_rect.  Reading the point cloud from a file
(:885) is the only step left out.

The file holds results only.  Per small case: fields (float32), occupancy (int8), corners (float32), and the two membership
lists as bit-packed flags over the sample's points (the script checks that the flagged rows ARE the lists the reference
returned).  The full-size case: occupancy value counts, float64 sums of each heat map, and strided subsamples.

For every small case the script asserts the decision margins the tests rely on: every tested point (cloud or grid) is at
least 1e-7 m from every plane it is tested against, and every index coordinate that gets floored (part centres,
foreground points) is at least 1e-7 from an integer.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
# modules the reference imports at module scope but never touches on the code paths used here
for _m in ("cv2", "torchvision", "torchvision.transforms", "imageio", "numba", "mayavi", "mayavi.mlab"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.path.insert(0, REF)

import snvc.dataset.KITTIRefinement_dataset as ref_ds  # noqa: E402
import snvc.dataset.kitti_util as ref_ku  # noqa: E402
from snvc.utils.bounding_box import construct_mesh_cuboid  # noqa: E402

# Mesh.in_mesh still uses the alias numpy removed; set only now: matplotlib's import (pulled in above) breaks if it exists earlier
np.bool = np.bool_

import target_cases as TC  # noqa: E402

MARGIN = 1e-7
D = ref_ds.refinementDataset
METHODS = ("_construct_box_3d", "_get_cam_cord", "_get_basis", "_draw_heatmaps_3d", "_draw_heatmaps_2d",
           "_construct_neural_confidence_field", "_get_point_cloud", "_to_cam")


def dataset(cfg):
    d = types.SimpleNamespace(cfg=cfg)
    d.df_params = {"spacing": np.array(cfg.spacing), "grid_resolution": np.array(cfg.grid_resolution), "range": cfg.grid_range,
                   "sigma": cfg.sigma, "x_range": cfg.x_range, "y_range": cfg.y_range, "z_range": cfg.z_range}
    for name in METHODS:
        setattr(d, name, (lambda f: (lambda *a, **k: f(d, *a, **k)))(getattr(D, name)))
    D._init_3d_grid(d)
    return d


def plane_margin(mesh, pts):
    q = np.hstack([pts, np.ones((len(pts), 1))])
    return float(np.min(np.abs(q @ mesh.planes.T) / np.linalg.norm(mesh.planes[:, :3], axis=1)))


def index_margin(d, local):
    """Distance to the nearest integer of the coordinates that _construct_neural_confidence_field / _get_point_cloud floor."""
    spa, re = d.df_params["spacing"], d.df_params["grid_resolution"]
    if not len(local):
        return 1.0
    x, y, z = local[:, 0], local[:, 1], local[:, 2]
    ny, nx, nz = 0.5 * (re - 1)
    c = np.stack([(y + ny * spa[0]) / spa[0], (x + nx * spa[1]) / spa[1], (z + nz * spa[2]) / spa[2]])
    return float(np.min(np.abs(c - np.round(c))))


def run_frame(d, samples, label, pc, check_margins):
    """The loop of _generate_displacement_field over one frame's samples.  Returns fields, occupancy, corners and the two
    flag arrays [N, len(pc)]."""
    pts_3d = d.grid_3d.copy().reshape(3, -1)
    fields, occ, corners, f_roi, f_fg = [], [], [], [], []
    for sample in samples:
        ret = d._construct_neural_confidence_field(sample, label, d.df_params)
        grid_cam = d._to_cam(pts_3d, sample).T                  # what _generate_grid_proj hands over as grid_3d[idx]
        pc_in_roi, pc_in_roi_fg, occupancy = d._get_point_cloud(pc, sample, label, grid_cam)
        fields.append(ret[0])
        corners.append(ret[2])
        occ.append(occupancy)
        # the lists as flags, and the margins, from the reference's own meshes
        roi_3d = sample.copy()
        roi_3d[:3] = d.df_params["range"]
        kpts = d._get_cam_cord(roi_3d).T
        mesh, mesh_gt = construct_mesh_cuboid(kpts), construct_mesh_cuboid(d._get_cam_cord(label).T)
        roi = mesh.in_mesh(pc)
        fg = np.logical_and(roi, mesh_gt.in_mesh(pc))
        assert np.array_equal(pc[roi], pc_in_roi) and np.array_equal(pc[fg], pc_in_roi_fg)
        f_roi.append(roi)
        f_fg.append(fg)
        if check_margins:
            m = min(plane_margin(mesh, pc), plane_margin(mesh_gt, pc), plane_margin(mesh_gt, grid_cam))
            assert m >= MARGIN, f"a tested point is {m:.3g} m from a plane"
            basis = d._get_basis(sample)
            parts = (d._get_cam_cord(label).T[:d.cfg.num_parts] - d._get_cam_cord(sample).T[[0]]) @ basis
            m = min(index_margin(d, parts), index_margin(d, (pc[fg] - kpts[0].reshape(1, 3)) @ basis))
            assert m >= MARGIN, f"a floored index coordinate is {m:.3g} from an integer"
    return (np.concatenate(fields).astype(np.float32), np.concatenate(occ).astype(np.float32),
            np.concatenate(corners).astype(np.float32), np.stack(f_roi), np.stack(f_fg))


def run_case(name, check_margins=True):
    c = TC.case(name)
    d = dataset(c["cfg"])
    pc = c["points"]
    if "velo_to_rect" in c:
        calib = ref_ku.Calibration(np.eye(3, 4), *c["velo_to_rect"])
        pc = calib.project_velo_to_rect(pc)
    if "frame" not in c:
        return c, run_frame(d, c["samples"], c["label"], pc, check_margins)
    # several frames: one reference run per frame (one label serves a frame's samples), flags padded to the longest frame
    off, frame = c["point_offsets"], c["frame"]
    pmax = int(np.diff(off).max())
    outs = []
    for i, sample in enumerate(c["samples"]):
        o = run_frame(d, sample[None], c["label"][i], pc[off[frame[i]]:off[frame[i] + 1]], check_margins)
        pad = lambda f: np.pad(f, ((0, 0), (0, pmax - f.shape[1])))  # noqa: E731
        outs.append(o[:3] + (pad(o[3]), pad(o[4])))
    return c, tuple(np.concatenate([o[k] for o in outs]) for k in range(5))


def main():
    out = {}
    for name in TC.SMALL:
        c, (fields, occ, corners, roi, fg) = run_case(name)
        assert set(np.unique(occ)) <= {-1.0, 0.0, 1.0}
        out[f"{name}/fields"] = fields
        out[f"{name}/occupancy"] = occ.astype(np.int8)
        out[f"{name}/corners"] = corners
        out[f"{name}/in_roi"] = np.packbits(roi, axis=1)
        out[f"{name}/in_fg"] = np.packbits(fg, axis=1)
        flat = fields.reshape(fields.shape[0], fields.shape[1], -1)
        full_window = (6 * c["cfg"].sigma + 1) ** (2 if c["cfg"].grid_type == "2D" else 3)
        nonzero = (flat != 0).sum(axis=2)
        print(f"{name:8s} occupancy -1/0/1: {[(occ == v).sum(axis=(1, 2, 3)).tolist() for v in (-1, 0, 1)]}  roi {roi.sum(axis=1).tolist()} "
              f"fg {fg.sum(axis=1).tolist()}  window cells per part (full {full_window}): {nonzero.tolist()}")
        if name.startswith("small"):
            # what the three samples are there for
            assert nonzero[0, 0] == full_window and (nonzero[0] > 0).all(), "sample 0: every part on the grid, the centre's window whole"
            assert ((nonzero[1] > 0) & (nonzero[1] < full_window)).sum() >= 3, "sample 1: several windows clipped"
            assert (nonzero[2] == 0).any(), "sample 2: a channel of zeros"
        if name == "quirks":
            d = dataset(c["cfg"])
            sample, re = c["samples"][0], np.array(c["cfg"].grid_resolution)
            roi_3d = sample.copy()
            roi_3d[:3] = c["cfg"].grid_range
            local = (c["points"][:c["hand_points"]] - d._get_cam_cord(roi_3d).T[0]) @ d._get_basis(sample)
            idx = np.floor((local[:, [1, 0, 2]] + 0.5 * (re - 1) * np.array(c["cfg"].spacing)) / np.array(c["cfg"].spacing))
            assert fg[0, :c["hand_points"]].all(), "the hand-placed points are foreground"
            assert idx[0, 1] == -1 and idx[1, 1] == re[1] and idx[2, 0] == -1 and idx[3, 2] == re[2], idx
            assert occ[0, int(idx[0, 0]), re[1] - 1, int(idx[0, 2])] == 1, "index -1 lands in the last cell"
            assert occ[0, int(idx[1, 0]), re[1] - 1, int(idx[1, 2])] == 1, "an index at the extent is clamped to the last cell"
    c, (fields, occ, corners, roi, fg) = run_case(TC.FULL, check_margins=False)
    sy, sx, sz = TC.FULL_STRIDE
    out["full/occ_counts"] = np.stack([(occ == v).sum(axis=(1, 2, 3)) for v in (-1, 0, 1)], axis=1).astype(np.int64)
    out["full/occ_sub"] = occ[:, ::sy, ::sx, ::sz].astype(np.int8)
    out["full/field_sums"] = fields.astype(np.float64).sum(axis=(2, 3, 4))
    out["full/field_sub"] = fields[:, :, ::sy, ::sx, ::sz]
    out["full/corners"] = corners
    print("full     occupancy -1/0/1:", out["full/occ_counts"].tolist())
    for name in TC.SMALL + (TC.FULL,):
        for key, (shape, dtype) in TC.expected_arrays(name).items():
            a = out[f"{name}/{key}"]
            assert a.shape == shape and a.dtype == dtype, (name, key, a.shape, a.dtype)
    np.savez_compressed(TC.GOLDEN_NPZ, **out)
    size = os.path.getsize(TC.GOLDEN_NPZ)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz") and f != "targets_ref.npz")
    print(TC.GOLDEN_NPZ, size, "bytes")
    assert size <= largest and size < 1 << 20, (size, largest)


if __name__ == "__main__":
    main()
