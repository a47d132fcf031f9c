#!/usr/bin/env python3
"""DSGN image backbone (feature_extraction, reslike-det-small, eval BatchNorm, seeded weights) on one GPU at the cfg2 image
size: N = 2 (a stereo pair) of 3 x 384 x 1248.

  backbone   the HIP route against the same module's torch route (MIOpen), timed alternately in one process after a
             warm-up; host clock around a device synchronise, median of --runs each.  Both outputs are compared (max error
             over the largest magnitude).  Convolution FLOPs come from the shapes (forward hooks on the torch route).
  e2e        images -> features -> GlobalStack.forward_pair at cfg2 (192 disparity planes), beside the features-in
             forward_pair on bench.make_inputs: ms per pair, pairs/s.

One JSON line.  Kernel times and launch counts: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o dsgn -- python tools/bench_dsgn.py --profile
which runs --runs HIP-route forwards only (no torch route, no e2e).
   python tools/bench_dsgn.py [--runs 20] [--warmup 5] [--no-e2e] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchlib.common import seeded_state  # noqa: E402
from snvc_amd.models import submodule as S  # noqa: E402

DEV = "cuda:0"
CFG = dict(RPN3D_ENABLE=False, GN=False, backbone="reslike-det-small", align_corners=False)


def wall_ms(fn, runs):
    ts = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return ts


def conv_classes(m, x):
    """GFLOP and layer count per convolution class, from the shapes of one torch-route pass."""
    cls = {}

    def hook(mod, inp, out):
        k, d = mod.kernel_size[0], mod.dilation[0]
        if m.lastconv[0][0] is mod:
            name = "lastconv"
        else:
            name = f"{k}x{k}_d{d}_s{mod.stride[0]}_{out.size(2)}x{out.size(3)}"
        c = cls.setdefault(name, {"gflop": 0.0, "layers": 0})
        c["gflop"] += 2 * out.numel() * mod.in_channels * k * mod.kernel_size[1] / 1e9
        c["layers"] += 1
    hs = [mod.register_forward_hook(hook) for mod in m.modules() if isinstance(mod, torch.nn.Conv2d)]
    S.DSGN_HIP[0] = False
    try:
        with torch.no_grad():
            m(x)
    finally:
        S.DSGN_HIP[0] = True
        for h in hs:
            h.remove()
    return cls


def model():
    m = S.feature_extraction(types.SimpleNamespace(**CFG))
    m.load_state_dict(seeded_state(m, 5), strict=True)
    return m.eval().to(DEV)


def images(seed=6):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((2, 3, 384, 1248)).astype(np.float32)).to(DEV)


def backbone(args):
    m, x = model(), images()

    def run(hip):
        S.DSGN_HIP[0] = hip
        try:
            with torch.no_grad():
                return m(x)[0]
        finally:
            S.DSGN_HIP[0] = True
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
    cls = conv_classes(m, x)
    flop = sum(c["gflop"] for c in cls.values()) * 1e9
    hip_ms, torch_ms = statistics.median(hip_ts), statistics.median(torch_ts)
    return {"batch": 2, "input": [3, 384, 1248], "runs": args.runs,
            "hip_ms_per_pair": hip_ms, "hip_ms_min": min(hip_ts), "torch_miopen_ms_per_pair": torch_ms,
            "torch_miopen_ms_min": min(torch_ts), "speedup_vs_miopen": torch_ms / hip_ms,
            "rel_err_hip_vs_miopen": err, "agree_1e-4": err <= 1e-4, "conv_gflop_per_pair": flop / 1e9, "conv_classes": cls,
            "hip_tflops": flop / (hip_ms * 1e-3) / 1e12, "miopen_tflops": flop / (torch_ms * 1e-3) / 1e12}


def e2e(args):
    import bench
    from snvc_amd.models.stereo_volume import GlobalStack
    stack = GlobalStack(bench.C)
    stack.load_state_dict(bench.seeded_state(stack))
    stack = stack.eval().to(DEV)
    left, right, shift = bench.make_inputs(0, DEV)
    m, x = model(), images()

    def from_images():
        with torch.no_grad():
            f = m(x)[0]
            return stack.forward_pair(f[0:1], f[1:2], shift, 1)

    def from_features():
        with torch.no_grad():
            return stack.forward_pair(left, right, shift, 1)
    for _ in range(args.warmup):
        from_images()
        from_features()
    ti, tf = [], []
    for _ in range(max(5, args.runs // 2)):
        ti += wall_ms(from_images, 1)
        tf += wall_ms(from_features, 1)
    out = from_images()
    mi, mf = statistics.median(ti), statistics.median(tf)
    return {"features": list(left.shape), "planes": int(shift.shape[1]), "from_images_ms_per_pair": mi,
            "from_images_pairs_per_s": 1e3 / mi, "from_features_ms_per_pair": mf, "from_features_pairs_per_s": 1e3 / mf,
            "outputs_finite": bool(torch.isfinite(out).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dsgn needs a GPU"
    res = {"tool": "bench_dsgn", "device": torch.cuda.get_device_name(0), "backbone": backbone(args)}
    if not (args.profile or args.no_e2e):
        res["e2e"] = e2e(args)
    res["routes"] = {k: v for k, v in S._ROUTES.items() if k.startswith("dsgn") or k == "conv2d_dilated_direct"}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
