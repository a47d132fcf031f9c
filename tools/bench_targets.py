"""Device time of the two training-target calls (include/snvc_targets.h) at the released grid, beside a numpy float64
composition of the same stages on the host CPU of the same box, written here and not routed through the module under test.

    python tools/bench_targets.py [--iters 30] [--warmup 5] [--out profiles/targets/bench_targets.txt]

The parent process only starts one child per case (a fresh process, under its own timeout) and collects their lines; a child
that fails ends the run.  Cases:
  device   grid (32, 128, 192), N = 8, 120 000 points, '3D', 9 parts: per iteration two device events around each C call
           (buffers allocated once), the median over the iterations.  That is the time of the call on the stream: the
           prologue and the streaming launches, host issue included.  "MB written" is what the call must write (every heat-map
           or occupancy element once); the point pass also reads N x P x 12 bytes.
  hbm      the rate benchlib/hbm_rows.py measures on this box (its a2 row, a 1.5 GB streaming read), the yardstick for
           "fraction of the measured HBM rate".
  host     the same targets for ONE sample with numpy float64 on the host, the way the reference's loader computes them
           (six plane tests over the grid points, twelve over the cloud, np.zeros + a window per part), stage by stage.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_DEVICE = 8


def child_device(iters, warmup):
    import ctypes
    import numpy as np
    import torch
    import target_cases as TC
    from snvc_amd import _targets
    from snvc_amd._lib import check
    from snvc_amd.geometry import TargetGenerator
    c = TC.case(TC.FULL)
    gen = TargetGenerator(c["cfg"])
    dev = torch.device("cuda:0")
    r = np.random.default_rng(3)
    samples = np.tile(c["samples"], (N_DEVICE // 2, 1))
    samples[:, 3:6] += r.uniform(-0.2, 0.2, (N_DEVICE, 3))
    s = torch.from_numpy(samples).to(dev)
    lab = torch.from_numpy(np.tile(c["label"], (N_DEVICE, 1))).to(dev)
    pts = torch.from_numpy(c["points"]).to(dev)
    L = _targets.lib()
    fields = torch.empty(gen.field_shape(N_DEVICE), dtype=torch.float32, device=dev)
    corners = torch.empty((N_DEVICE, gen.num_parts, 3), dtype=torch.float32, device=dev)
    occ = torch.empty((N_DEVICE, gen.nh, gen.nw, gen.nl), dtype=torch.float32, device=dev)
    ws = torch.empty(L.snvc_targets_workspace_bytes(N_DEVICE), dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    g = ctypes.byref(gen.grid)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    calls = {
        "fields": lambda: check(L.snvc_targets_fields(g, p(s), p(lab), N_DEVICE, p(ws), p(fields), p(corners), stream)),
        "occupancy": lambda: check(L.snvc_targets_occupancy(g, p(s), p(lab), N_DEVICE, p(pts), 1, len(pts), None, len(pts), None, p(ws),
                                                            p(occ), None, None, stream)),
        "generate": lambda: gen.generate(s, lab, pts, dev),
    }
    out = {"case": "device", "iters": iters, "fields_bytes": fields.numel() * 4, "occupancy_bytes": occ.numel() * 4,
           "points_read_bytes": N_DEVICE * pts.numel() * 8}
    for name, fn in calls.items():
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out[name + "_ms"], out[name + "_min_ms"] = statistics.median(ms), min(ms)
    print("RESULT " + json.dumps(out))


def child_hbm():
    import torch
    from benchlib import hbm_rows
    from benchlib.common import PEAK_HBM_GBS
    row = hbm_rows.cost_volume_backward_row(torch.device("cuda:0"))
    print("RESULT " + json.dumps({"case": "hbm", "gbs": row["achieved"], "peak_gbs": PEAK_HBM_GBS, "what": row["kernel"]}))


def child_host(iters):
    import numpy as np
    import target_cases as TC
    c = TC.case(TC.FULL)
    cfg = c["cfg"]
    nh, nw, nl = cfg.grid_resolution
    re, spa = np.array(cfg.grid_resolution), np.array(cfg.spacing)
    sample, label, pc = c["samples"][0], c["label"], c["points"]

    def rot(ry):
        return np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])

    def corners(box):
        h, w, l = box[:3]
        fixed = np.array([[0.5 * l, l, l, l, l, 0, 0, 0, 0], [0.5 * h, 0, h, 0, h, 0, h, 0, h], [0.5 * w, w, w, 0, 0, w, w, 0, 0]])
        fixed = fixed - np.array([[np.float32(l) / 2], [np.float32(h)], [np.float32(w) / 2]])
        return (rot(box[6]) @ fixed + box[3:6].reshape(3, 1)).T

    faces = np.array([[2, 1, 3], [8, 7, 5], [6, 5, 1], [4, 3, 7], [1, 5, 7], [8, 6, 2]])

    def in_box(kpts, q):
        flag = np.ones(len(q), dtype=bool)
        q = np.hstack([q, np.ones((len(q), 1))])
        for a, b, cc in faces:
            normal = np.cross(kpts[b] - kpts[a], kpts[cc] - kpts[b])
            plane = np.append(normal, -kpts[a] @ normal)
            flag = np.logical_and(flag, (q @ plane.reshape(4, 1) < 0)[:, 0])
        return flag

    def index(local):
        x, y, z = np.split(local, 3, axis=1)
        ny, nx, nz = 0.5 * (re - 1)
        return np.floor((y + ny * spa[0]) / spa[0]), np.floor((x + nx * spa[1]) / spa[1]), np.floor((z + nz * spa[2]) / spa[2])

    gx, gy, gz = np.meshgrid(np.linspace(*cfg.x_range, nw), np.linspace(*cfg.y_range, nh), np.linspace(*cfg.z_range, nl), indexing="xy")
    grid = np.concatenate([gx[None], gy[None], gz[None]]).reshape(3, -1)
    basis = rot(sample[6]) @ np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]]).T

    def occupancy():
        grid_cam = (rot(sample[6] + 0.5 * np.pi) @ grid + np.array([[sample[3]], [sample[4] - sample[0] * 0.5], [sample[5]]])).T
        roi = sample.copy()
        roi[:3] = cfg.grid_range
        k_roi, k_gt = corners(roi), corners(label)
        fg = pc[np.logical_and(in_box(k_roi, pc), in_box(k_gt, pc))]
        i, j, k = (np.minimum(v, e - 1).squeeze().astype(np.int32) for v, e in zip(index((fg - k_roi[0]) @ basis), re))
        occ = -np.ones((nh, nw, nl), dtype=np.float32)
        occ[i, j, k] = 1.
        occ[np.logical_not(in_box(k_gt, grid_cam).reshape(nh, nw, nl))] = 0.
        return occ

    def heat_maps():
        t = 3 * cfg.sigma
        x = (np.arange(0, 2 * t + 1, 1, np.float32) - t) ** 2
        gauss = np.exp(-(x.reshape(-1, 1, 1) + x.reshape(1, -1, 1) + x.reshape(1, 1, -1)) / (2 * cfg.sigma ** 2))
        mu = np.concatenate(index((corners(label)[:cfg.num_parts] - corners(sample)[[0]]) @ basis), axis=1).astype(int)
        out = []
        for m in mu:
            f = np.zeros((nh, nw, nl))
            lo, hi = np.maximum(m - t, 0), np.minimum(m + t + 1, re)
            if (hi > lo).all():
                f[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = gauss[lo[0] - m[0] + t:hi[0] - m[0] + t, lo[1] - m[1] + t:hi[1] - m[1] + t,
                                                                 lo[2] - m[2] + t:hi[2] - m[2] + t]
            out.append(f[None])
        return np.concatenate(out).astype(np.float32)

    res = {"case": "host", "iters": iters}
    for name, fn in (("occupancy", occupancy), ("fields", heat_maps)):
        fn()
        ms = []
        for _ in range(iters):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name + "_ms"] = statistics.median(ms)
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "targets", "bench_targets.txt"))
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return {"device": lambda: child_device(args.iters, args.warmup), "hbm": child_hbm,
                "host": lambda: child_host(max(3, args.iters // 6))}[args.child]()
    rows = {}
    for name in ("device", "hbm", "host"):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(args.iters),
                            "--warmup", str(args.warmup)], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit(f"bench_targets: case {name} failed (exit status {r.returncode}); nothing more is started")
        rows[name] = json.loads(line[0][7:])
    d, h, c = rows["device"], rows["hbm"], rows["host"]
    text = [f"training targets at grid (32, 128, 192), '3D', 9 parts, sigma 2, 120 000 float64 points; device: N = {N_DEVICE}, median of "
            f"{d['iters']} event-timed calls after {args.warmup} warm-up (call time on the stream, host issue included; not kernel time)",
            f"measured HBM rate of this box (benchlib/hbm_rows.py, a2 row): {h['gbs']:.0f} GB/s; data-sheet peak {h['peak_gbs']:.0f} GB/s",
            f"{'call':28s} {'ms':>9s} {'min ms':>9s} {'MB written':>11s} {'GB/s':>8s} {'of measured':>12s} {'of peak':>8s}"]
    for name, nbytes in (("fields", d["fields_bytes"]), ("occupancy", d["occupancy_bytes"])):
        gbs = nbytes / (d[name + "_ms"] * 1e-3) / 1e9
        text.append(f"snvc_targets_{name:15s} {d[name + '_ms']:9.4f} {d[name + '_min_ms']:9.4f} {nbytes / 1e6:11.1f} {gbs:8.0f} "
                    f"{gbs / h['gbs']:12.3f} {gbs / h['peak_gbs']:8.3f}")
    text.append(f"{'TargetGenerator.generate':28s} {d['generate_ms']:9.4f} {d['generate_min_ms']:9.4f}   (allocation and both calls; "
                f"the occupancy call also reads {d['points_read_bytes'] / 1e6:.1f} MB of points)")
    per = (d["fields_ms"] + d["occupancy_ms"]) / N_DEVICE
    text.append(f"host numpy float64, ONE sample, median of {c['iters']}: occupancy stage {c['occupancy_ms']:.1f} ms, heat maps {c['fields_ms']:.1f} ms; "
                f"device per sample {per:.4f} ms: {(c['occupancy_ms'] + c['fields_ms']) / per:.0f}x")
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
