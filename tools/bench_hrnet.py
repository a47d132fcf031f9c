#!/usr/bin/env python3
"""HRNet-w32 backbone on one GPU, at the released shape: eval, seeded weights, batch 16 (8 crops x 2 sides) of 3 x 256 x 256.

  backbone   the HIP route (fused_conv2d + the fusion kernel) against the same module's torch route (MIOpen), timed
             alternately in one process after a warm-up; host clock around a device synchronise, median of --runs each.
             Both outputs are compared (max error over the largest magnitude).  FLOPs and bytes come from the shapes.
  e2e        VernierScale.forward from RoI images (HRNet-w32 + the 3D trunk + heads) at grid 32 x 128 x 192 on 8 crops,
             beside the same model's features-in forward (identity backbone, feature maps in): ms per crop, crops/s.

One JSON line.  Kernel times and launch counts: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o hrnet -- python tools/bench_hrnet.py --profile
which runs --runs HIP-route forwards only (no torch route, no e2e).
   python tools/bench_hrnet.py [--runs 20] [--warmup 5] [--no-e2e] [--out FILE]"""
import argparse
import copy
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchlib import hrnet as B  # noqa: E402
from benchlib.common import seeded_state  # noqa: E402
from snvc_amd import _hrnet  # noqa: E402
from snvc_amd.models import hrnet as H  # noqa: E402
from snvc_amd.models import submodule as S  # noqa: E402

DEV = "cuda:0"


def wall_ms(fn, runs):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def shapes_count(m, x):
    """FLOPs and minimal bytes of every convolution (input + output + weight, fp32) from one torch-route pass, and the
    bytes the fusion kernel moves on the HIP route (its terms read once, its output written once)."""
    conv = {"flop": 0, "bytes": 0, "n": 0}

    def hook(mod, inp, out):
        x_ = inp[0]
        conv["flop"] += 2 * out.numel() * mod.in_channels * mod.kernel_size[0] * mod.kernel_size[1]
        conv["bytes"] += 4 * (x_.numel() + out.numel() + mod.weight.numel())
        conv["n"] += 1
    hs = [mod.register_forward_hook(hook) for mod in m.modules() if isinstance(mod, torch.nn.Conv2d)]
    H.HRNET_HIP[0] = False
    with torch.no_grad():
        m(x)
    H.HRNET_HIP[0] = True
    for h in hs:
        h.remove()
    fuse = {"bytes": 0, "n": 0}
    real = _hrnet.fuse_forward

    def counted(terms, factors, relu=True, out=None):
        r = real(terms, factors, relu=relu, out=out)
        fuse["bytes"] += 4 * (sum(t.numel() for t in terms if t is not None) + r.numel())
        fuse["n"] += 1
        return r
    _hrnet.fuse_forward = counted
    try:
        with torch.no_grad():
            m(x)
    finally:
        _hrnet.fuse_forward = real
    return conv, fuse


def backbone(args):
    m = H.get_model(copy.deepcopy(B.W32), False)
    m.load_state_dict(seeded_state(m, B.W32_SEEDS[0]), strict=True)
    m = m.eval().to(DEV)
    x = B.image((16, 3, 256, 256), B.W32_SEEDS[1]).to(DEV)

    def run(hip):
        H.HRNET_HIP[0] = hip
        try:
            with torch.no_grad():
                return m(x)
        finally:
            H.HRNET_HIP[0] = True
    if args.profile:
        for _ in range(args.warmup):
            run(True)
        torch.cuda.synchronize()
        wall = wall_ms(lambda: run(True), args.runs)
        return {"profile_runs": args.runs, "hip_ms_median": statistics.median(wall)}
    for _ in range(args.warmup):
        run(True)
        run(False)
    hip_ts, torch_ts = [], []
    for _ in range(args.runs):
        hip_ts += wall_ms(lambda: run(True), 1)
        torch_ts += wall_ms(lambda: run(False), 1)
    a, b = run(True), run(False)
    err = float((a.double() - b.double()).abs().max() / b.double().abs().max())
    conv, fuse = shapes_count(m, x)
    hip_ms, torch_ms = statistics.median(hip_ts), statistics.median(torch_ts)
    return {"batch": 16, "input": [3, 256, 256], "runs": args.runs,
            "hip_ms": hip_ms, "hip_ms_min": min(hip_ts), "torch_miopen_ms": torch_ms, "torch_miopen_ms_min": min(torch_ts),
            "speedup_vs_miopen": torch_ms / hip_ms, "rel_err_hip_vs_miopen": err, "agree_1e-4": err <= 1e-4,
            "conv_layers": conv["n"], "conv_gflop": conv["flop"] / 1e9, "conv_min_gbytes": conv["bytes"] / 1e9,
            "fusion_launches": fuse["n"], "fusion_gbytes": fuse["bytes"] / 1e9,
            "launches_min": conv["n"] + fuse["n"],
            "hip_tflops": conv["flop"] / (hip_ms * 1e-3) / 1e12, "miopen_tflops": conv["flop"] / (torch_ms * 1e-3) / 1e12}


def e2e(args, crops=8, grid=(32, 128, 192)):
    from benchlib.local import local_model
    from snvc_amd.models.vernier import VernierScale
    r = np.random.default_rng(5)
    v = grid[0] * grid[1] * grid[2]
    proj = [torch.from_numpy(r.uniform(-8, 264, (crops, 2, v)).astype(np.float32)).to(DEV) for _ in range(2)]
    feats_in = local_model(grid, 32, DEV)
    lf, rf = [torch.from_numpy(r.standard_normal((crops, 32, 64, 64)).astype(np.float32)).to(DEV) for _ in range(2)]
    cfg = types.SimpleNamespace(**vars(feats_in.cfg))
    cfg.hrfeat = copy.deepcopy(B.W32)
    m = VernierScale(cfg)
    m.load_state_dict(seeded_state(m), strict=True)
    m = m.eval().to(DEV)
    imgs = [B.image((crops, 3, 256, 256), s).to(DEV) for s in (6, 7)]

    def from_images():
        with torch.no_grad():
            return m(imgs[0], imgs[1], proj[0], proj[1])

    def from_features():
        with torch.no_grad():
            return feats_in(lf, rf, proj[0], proj[1])
    for _ in range(args.warmup):
        from_images()
        from_features()
    ti, tf = [], []
    for _ in range(max(5, args.runs // 2)):
        ti += wall_ms(from_images, 1)
        tf += wall_ms(from_features, 1)
    out = from_images()
    mi, mf = statistics.median(ti), statistics.median(tf)
    return {"crops": crops, "grid": list(grid), "from_images_ms_per_crop": mi / crops, "from_images_crops_per_s": crops / (mi * 1e-3),
            "forward_ms_per_crop": mf / crops, "backbone_share_ms_per_crop": (mi - mf) / crops,
            "outputs_finite": bool(all(torch.isfinite(out[k]).all() for k in ("ncf", "occupancy", "coordinates")))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hrnet needs a GPU"
    res = {"tool": "bench_hrnet", "device": torch.cuda.get_device_name(0), "backbone": backbone(args)}
    if not (args.profile or args.no_e2e):
        res["e2e"] = e2e(args)
    res["routes"] = {k: v for k, v in S._ROUTES.items() if k.startswith("hrnet")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
