"""Writes tests/golden/roi_crop_ref.npz: the crop geometry the reference's own data loader computes for the cases of
tests/roi_crop_cases.py.

    python tests/golden/make_golden_roi_crop.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Needs the reference checkout (numpy on the CPU); the tests need only the file.  refinementDataset._generate_rois is called
unbound on a SimpleNamespace that carries roi_params / df_params, once per frame and side pair, with a stub ``cv2`` module:
  getAffineTransform   a float64 linear solve of our own (numpy.linalg.solve of the 3 x 3 system [x y 1] -> x', y'), fed with
                       the float32 point triples the reference builds;
  imread / cvtColor    hand back the case's arrays;     warpAffine   returns zeros.
So the stub pins the geometry only (kpts_2d, trans, kpts_2d_local), not the warp: no cv2 build is at hand.

The file holds results only: per case kpts_l / kpts_r [N,9,2] float64, trans_l / trans_r [N,2,3] float64 and local_l / local_r
[N,9,2] float32.  The script also prints the largest gap between the closed form of tests/roi_crop_ref.py and the stub's
solve; tests/test_roi_crop_host.py allows 16 times the figure recorded here (SOLVE_GAP) and never more than 1e-9.
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

IMAGES = {}


def _solve(src, dst):
    assert src.dtype == np.float32 and dst.dtype == np.float32 and src.shape == dst.shape == (3, 2)
    A = np.hstack([src.astype(np.float64), np.ones((3, 1))])
    return np.linalg.solve(A, dst.astype(np.float64)).T


cv2 = sys.modules["cv2"]
cv2.getAffineTransform = _solve
cv2.imread = lambda path, flags: IMAGES[path]
cv2.cvtColor = lambda img, code: img
cv2.warpAffine = lambda img, trans, size, flags: np.zeros((size[1], size[0], 3), dtype=np.uint8)
cv2.COLOR_BGR2RGB, cv2.INTER_LINEAR = 4, 1
sys.path.insert(0, REF)

import snvc.dataset.KITTIRefinement_dataset as ref_ds  # noqa: E402
import snvc.dataset.kitti_util as ref_ku  # noqa: E402

import roi_crop_cases as C  # noqa: E402
import roi_crop_ref as R  # noqa: E402

D = ref_ds.refinementDataset
METHODS = ("_construct_box_3d", "_get_cam_cord", "_crop_instance")


def dataset(cfg):
    d = types.SimpleNamespace(roi_params={"resolution": cfg.resolution, "aspect_ratio": cfg.aspect_ratio},
                              df_params={"range": cfg.grid_range})
    for name in METHODS:
        setattr(d, name, (lambda f: (lambda *a, **k: f(d, *a, **k)))(getattr(D, name)))
    return d


def run_case(name):
    c = C.case(name)
    d = dataset(c["cfg"])
    n = len(c["samples"])
    out = {k: [None] * n for k in ("kpts_l", "kpts_r", "trans_l", "trans_r", "local_l", "local_r")}
    for f in range(len(c["left"])):
        rows = [i for i in range(n) if C.frame_of(c, i) == f]
        IMAGES["left"], IMAGES["right"] = c["left"][f], c["right"][f]
        calib = [ref_ku.Calibration(P[f], np.eye(3, 4), np.eye(3)) for P in (c["P_left"], c["P_right"])]
        _, _, meta = D._generate_rois(d, c["samples"][rows], "left", "right", calib[0], calib[1])
        for j, i in enumerate(rows):
            for side in "lr":
                out[f"kpts_{side}"][i] = meta[f"kpts_2d_{side}"][j]
                out[f"trans_{side}"][i] = meta[f"trans_{side}"][j]
                out[f"local_{side}"][i] = meta[f"kpts_2d_{side}_local"][j]
    return c, {k: np.stack(v) for k, v in out.items()}


def main():
    out, gap, kgap = {}, 0.0, 0.0
    for name in C.NAMES:
        c, arrays = run_case(name)
        for key, a in arrays.items():
            assert a.dtype == (np.float32 if key.startswith("local") else np.float64), (key, a.dtype)
            out[f"{name}/{key}"] = a
        for i, s in enumerate(c["samples"]):
            f = C.frame_of(c, i)
            for side, P in (("l", c["P_left"]), ("r", c["P_right"])):
                kpts, trans, _ = R.geometry(s, P[f], c["cfg"].grid_range, c["cfg"].aspect_ratio, c["cfg"].resolution)
                gap = max(gap, float(np.abs(trans - arrays[f"trans_{side}"][i]).max()))
                kgap = max(kgap, float(np.abs(kpts - arrays[f"kpts_{side}"][i]).max()))
    print(f"largest |closed form - float64 solve| over the entries of trans, all cases: {gap:.3e}   (SOLVE_GAP)")
    print(f"largest |restated key point - reference key point|: {kgap:.3e}")
    np.savez_compressed(C.GOLDEN_NPZ, **out)
    size = os.path.getsize(C.GOLDEN_NPZ)
    print(C.GOLDEN_NPZ, size, "bytes")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
