"""Golden vectors of the HRNet backbone by IMPORTING THE REFERENCE (needs the reference checkout; CPU only):
    python tests/golden/make_golden_hrnet.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Builds the reference's own snvc.models.hrnet modules (and one reference VernierScale around a small HRNet), seeds their
weights with benchlib.common.seeded_state and their inputs from numpy.random.default_rng seeds (benchlib/hrnet.py), and
stores only what the tests cannot regenerate: ordered state-dict keys and shapes, and outputs (tests/golden/hrnet_ref.npz).

    keys/<w32|w48>, shapes/<w32|w48>      ordered state-dict keys; shapes padded with -1 to four dimensions
    small/<name>                          eval output of each benchlib.hrnet.SMALL config on its seeded 2 x C x 64 x 64 input
    w32/out                               eval output [1, 32, 64, 64] of HRNet-w32 on a seeded 1 x 3 x 256 x 256 input
    e2e/<ncf|occupancy|coordinates>       a reference VernierScale (BEV_type3, small HRNet, grid 16 x 16 x 24) from RoI images
    e2e/<left|right>_feat                 its backbone's outputs (to tell the backbone's error from the trunk's)

No rescaling of the seeded weights was needed: every stored output is asserted finite and not all zero.
"""
import copy
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")
for _m in ("cv2", "torchvision", "torchvision.transforms", "imageio", "numba", "mayavi", "mayavi.mlab"):
    sys.modules.setdefault(_m, types.ModuleType(_m))
sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
sys.path.insert(0, REF)

import snvc.models.hrnet as ref_hrnet  # noqa: E402
import snvc.models.vernier as ref_vernier  # noqa: E402

from benchlib import hrnet as B  # noqa: E402
from benchlib.common import seeded_state  # noqa: E402
import golden_cases as GC  # noqa: E402

torch.set_num_threads(8)


def solid(name, t):
    a = t.detach().numpy()
    assert np.isfinite(a).all() and np.abs(a).max() > 0, name
    print(f"{name:28s} {tuple(a.shape)}  max |v| {np.abs(a).max():.4g}")
    return a


def model(cfg, seed):
    m = ref_hrnet.get_model(copy.deepcopy(cfg), False)
    m.load_state_dict(seeded_state(m, seed), strict=True)
    return m.eval()


def e2e_cfg():
    grid = (16, 16, 24)
    cfg = types.SimpleNamespace(vernier_type="BEV_type3", backbone="hrfeat", gn=False, grid_resolution=list(grid),
                                resolution=GC.RESOLUTION, x_range=(-1.0, 1.0), z_range=(-1.0, 1.0), num_parts=9)
    cfg.hrfeat = B.E2E_HRNET
    cfg.n_sample_h, cfg.n_sample_w, cfg.n_sample_l = grid
    return cfg


out = {}
with torch.no_grad():
    for nm, cfg in (("w32", B.W32), ("w48", B.W48)):
        sd = ref_hrnet.get_model(copy.deepcopy(cfg), False).state_dict()
        out[f"keys/{nm}"] = np.array(list(sd))
        out[f"shapes/{nm}"] = np.array([list(v.shape) + [-1] * (4 - v.dim()) for v in sd.values()], np.int32)
    for nm, (cfg, wseed, xseed) in B.SMALL.items():
        n, h, w = B.SMALL_INPUT
        out[f"small/{nm}"] = solid(f"small/{nm}", model(cfg, wseed)(B.image((n, B.in_channels(cfg), h, w), xseed)))
    out["w32/out"] = solid("w32/out", model(B.W32, B.W32_SEEDS[0])(B.image((1, 3, 256, 256), B.W32_SEEDS[1])))

    cfg = e2e_cfg()
    ref = ref_vernier.VernierScale(cfg)
    ref.load_state_dict(seeded_state(ref, B.E2E_SEEDS[0]), strict=True)
    ref.eval()
    imgs, gpl, gpr = B.e2e_inputs(cfg, B.E2E_SEEDS[1])
    res = ref(imgs[0], imgs[1], gpl.clone(), gpr.clone())
    out["e2e/left_feat"] = solid("e2e/left_feat", ref.feat_net(imgs[0]))         # what the 3D trunk starts from
    out["e2e/right_feat"] = solid("e2e/right_feat", ref.feat_net(imgs[1]))
    for k in ("ncf", "occupancy", "coordinates"):
        out[f"e2e/{k}"] = solid(f"e2e/{k}", res[k])
path = os.path.join(HERE, "hrnet_ref.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes")
