"""HRNet backbone configurations shared by tests/golden/make_golden_hrnet.py, the HRNet tests and tools/bench_hrnet.py.

The released model's backbone is HRNet-w32 (widths 32/64/128/256, stage modules 1/1/4/3, four blocks per branch) with
the "default" head on 256x256 RoI crops; w48 widens it to 48/96/192/384.  The SMALL configurations keep every structural
case (bottleneck and basic stages, one to four branches, fusion factors 2 to 8) at a size that runs on the CPU in
seconds, with widths that are not multiples of 32.  Inputs are drawn from ``numpy.random.default_rng`` seeds and weights
from ``benchlib.common.seeded_state``; nothing but outputs is stored.
"""
import types

import numpy as np
import torch


def _stage(modules, branches, block, blocks, channels):
    return types.SimpleNamespace(num_modules=modules, num_branches=branches, block=block, num_blocks=list(blocks),
                                 num_channels=list(channels), fuse_method="SUM")


def make_cfg(widths, blocks=4, modules=(1, 1, 4, 3), stem_block="bottleneck", stem_width=64, name="hrnet-w32",
             head_type="default", add_xy=False):
    """A cfg.hrfeat-style namespace: ``widths`` = the four branch widths of stages 2-4."""
    w = list(widths)
    extra = types.SimpleNamespace(
        stage1=_stage(modules[0], 1, stem_block, [blocks], [stem_width]),
        stage2=_stage(modules[1], 2, "basic", [blocks] * 2, w[:2]),
        stage3=_stage(modules[2], 3, "basic", [blocks] * 3, w[:3]),
        stage4=_stage(modules[3], 4, "basic", [blocks] * 4, w[:4]))
    return types.SimpleNamespace(name=name, extra=extra, head_type=head_type, add_xy=add_xy, init_weights=False,
                                 pre_trained_path="", output_channel=w[0])


W32 = make_cfg((32, 64, 128, 256))
W48 = make_cfg((48, 96, 192, 384), name="hrnet-w48")

# name: (cfg, weight seed, input seed); inputs 2 x C x 64 x 64
SMALL = {
    "s_basic": (make_cfg((8, 16, 24, 40), blocks=1, modules=(1, 1, 1, 1), stem_width=16), 900, 901),
    "s_two_modules": (make_cfg((12, 20, 28, 36), blocks=2, modules=(1, 2, 2, 2), stem_block="basic", stem_width=24), 910, 911),
    "s_add_xy": (make_cfg((8, 16, 24, 40), blocks=1, modules=(1, 1, 1, 1), stem_width=16, add_xy=True), 920, 921),
}
SMALL_INPUT = (2, 64, 64)          # N, H, W
W32_SEEDS = (930, 931)             # weights, the 1 x 3 x 256 x 256 input
E2E_SEEDS = (940, 941)             # the end-to-end VernierScale case: weights, inputs


def in_channels(cfg):
    return 5 if getattr(cfg, "add_xy", False) else 3


def image(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


# the end-to-end VernierScale case: a small HRNet whose first branch has the trunk's 32 channels
E2E_HRNET = make_cfg((32, 16, 24, 40), blocks=1, modules=(1, 1, 1, 1), stem_width=16)
E2E_BATCH = 2


def e2e_inputs(cfg, seed, n=E2E_BATCH):
    """(left, right) RoI images [n, 3, res, res] and the projected grids [n, 2, nh * nw * nl] in RoI pixels; about 6 % of
    the projections fall outside the crop."""
    rng = np.random.default_rng(seed)
    rh, rw = cfg.resolution
    v = cfg.n_sample_h * cfg.n_sample_w * cfg.n_sample_l
    imgs = [torch.from_numpy(rng.standard_normal((n, 3, rh, rw)).astype(np.float32)) for _ in range(2)]
    gp = [torch.from_numpy(rng.uniform(-0.03 * rw, 1.03 * rw, (n, 2, v)).astype(np.float32)) for _ in range(2)]
    return imgs, gp[0], gp[1]
