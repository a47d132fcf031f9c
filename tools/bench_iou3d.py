#!/usr/bin/env python3
"""End-to-end times of the rotated-box IoU / NMS family (snvc_amd.extension.iou3d_nms) on one GPU: BEV IoU and 3D IoU
matrices of 1k x 1k and 4k x 4k boxes, rotated and axis-aligned NMS of 1k / 4k / 16k boxes (score sort, both launches
and the 4-byte count read-back, i.e. what a caller of nms_gpu waits for).  Seeded KITTI-like scenes: objects in a
70 m x 80 m field, each proposed several times with jitter.  One JSON line per case.  Kernel times: run it under
    rocprofv3 --kernel-trace --stats -d <dir> -o iou3d -- python tools/bench_iou3d.py --reps 20
   python tools/bench_iou3d.py [--reps 50] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from snvc_amd.extension.iou3d_nms import iou3d_nms_utils as U  # noqa: E402

DIMS = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])


def scene(n, seed, dup=6):
    r = np.random.default_rng(seed)
    k = max(1, n // dup)
    obj = np.concatenate([r.uniform(0, 70, (k, 1)), r.uniform(-40, 40, (k, 1)), r.uniform(-2.5, 0.5, (k, 1)),
                          DIMS[r.choice(3, k, p=[0.7, 0.2, 0.1])], r.uniform(-np.pi, np.pi, (k, 1))], 1)
    pick = obj[r.integers(0, k, n)]
    jit = np.concatenate([r.normal(0, 0.25, (n, 2)), r.normal(0, 0.1, (n, 1)), pick[:, 3:6] * r.normal(0, 0.08, (n, 3)),
                          r.normal(0, 0.15, (n, 1))], 1)
    return torch.from_numpy((pick + jit).astype(np.float32)).cuda(), torch.from_numpy(r.random(n).astype(np.float32)).cuda()


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return float(np.median(ts)), float(np.min(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for n in (1024, 4096):
        b, _ = scene(n, n)
        for name, fn in (("iou_bev", U.boxes_iou_bev), ("iou3d", U.boxes_iou3d_gpu)):
            med, best = timed(lambda: fn(b, b), args.reps)
            rows.append({"case": f"{name} {n}x{n}", "median_us": round(med, 1), "min_us": round(best, 1),
                         "pairs_per_us": round(n * n / med, 1)})
            print(json.dumps(rows[-1]), flush=True)
    for n in (1024, 4096, 16384):
        b, s = scene(n, n + 1)
        for name, fn in (("nms_gpu", U.nms_gpu), ("nms_normal_gpu", U.nms_normal_gpu)):
            med, best = timed(lambda: fn(b, s, 0.1), args.reps)
            kept = fn(b, s, 0.1)[0].numel()
            rows.append({"case": f"{name} {n} @0.1", "median_us": round(med, 1), "min_us": round(best, 1), "kept": kept})
            print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
