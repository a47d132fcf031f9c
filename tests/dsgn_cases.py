"""Configurations of the DSGN image backbone shared by tests/golden/make_golden_dsgn.py and the DSGN tests.

GOLDEN: name -> (cfg fields, (N, 3, H, W) of the seeded input, weight seed, input seed).  The branch configurations need
feature maps of at least 64 x 64 (the 64 x 64 pooling window), i.e. images of at least 256 x 256.
"""
import types

import numpy as np
import torch

BACKBONES = ("reslike-det", "reslike-det-small", "reslike-det-small-fixfirst", "reslike50-det-small-fixfirst", "reslike50-det-tiny")

GOLDEN = {
    "small_bn": (dict(backbone="reslike-det-small", GN=False, align_corners=False), (1, 3, 256, 256), 11, 12),
    # GroupNorm of branch1's 64 x 64 pool needs two pooled values per group: features of at least 64 x 128
    "small_gn": (dict(backbone="reslike-det-small", GN=True, align_corners=False), (1, 3, 256, 512), 21, 22),
    "tiny_nobranch": (dict(backbone="reslike50-det-tiny", GN=False, branch=False), (1, 3, 64, 96), 31, 32),
    # rpnconv only (no lastconv): RPN_CONVDIM 16 takes GroupNorm's 16-group form and keeps the fixture small
    "rpn_ac": (dict(backbone="reslike50-det-small-fixfirst", GN=False, align_corners=True, RPN3D_ENABLE=True, cat_img_feature=True,
                    RPN_ONEMORE_CONV=True, RPN_ONEMORE_DIM=64, RPN_CONVDIM=16, PlaneSweepVolume=False), (1, 3, 256, 256), 41, 42),
}

# the golden files: one per group, each below the 1 MiB limit of a committed file
FILES = {"dsgn_ref.npz": ("small_bn", "tiny_nobranch", "rpn_ac"), "dsgn_ref_gn.npz": ("small_gn",)}
STORED_CHANNELS = {"small_gn": 16}      # output_feature channels kept in the fixture (the first ones), where not all


def cfg(**fields):
    base = dict(RPN3D_ENABLE=False, GN=False, backbone="reslike-det-small", align_corners=False)
    base.update(fields)
    return types.SimpleNamespace(**base)


def image(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))
