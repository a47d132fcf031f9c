"""Device time of RoICropper.generate (include/snvc_roicrop.h) for N = 1, 10 and 64 crops of 256 x 256 from a 375 x 1242 stereo
pair, beside the same crops by torch's F.grid_sample + normalisation on the same GPU and beside the store floor.

    python tools/bench_roicrop.py [--iters 200] [--warmup 20] [--out profiles/roicrop/bench_roicrop.txt]

The parent process only starts one child per case (a fresh process, under its own timeout) and collects their lines; a child
that fails ends the run.  Cases:
  device   per N: two device events around (a) the C call alone, outputs and workspace allocated once and the images already
           on the device, and (b) RoICropper.generate with device-resident inputs (allocation of the outputs, the descriptor
           upload and the call); the median over the iterations.  That is time on the stream, host issue included, not kernel
           time: kernel time is what `rocprofv3 --kernel-trace --stats -- python tools/bench_roicrop.py --child device` lists.
  torch    per N: affine_grid-free F.grid_sample (bilinear, zeros, align_corners=True on a grid built from the same
           transforms, uploaded before the timed window) of the float image, then the normalisation: the composition a user
           would write with torch alone.  The grid construction is outside the timed window, in torch's favour.
  hbm      the write rate of this box: a 1 GiB tensor.zero_(), median of 20; the store floor of N crops is
           N x 2 x 3 x 256 x 256 x 4 bytes over that rate.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 10, 64)
RES = (256, 256)
IMAGE = (375, 1242)


def inputs(n):
    import types
    import numpy as np
    r = np.random.default_rng(7)
    cfg = types.SimpleNamespace(resolution=RES, aspect_ratio=1.0, grid_range=(3.0, 3.0, 6.0), img_mean=(0.485, 0.456, 0.406),
                                img_std=(0.229, 0.224, 0.225))
    P = np.array([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
    Pr = P.copy()
    Pr[0, 3] -= 721.5377 * 0.54
    samples = np.stack([r.uniform(1.4, 1.7, n), r.uniform(1.5, 1.8, n), r.uniform(3.5, 4.5, n), r.uniform(-12, 12, n),
                        r.uniform(1.4, 1.9, n), r.uniform(8, 45, n), r.uniform(-3.1, 3.1, n)], axis=1)
    left, right = (r.integers(0, 256, IMAGE + (3,), dtype=np.uint8) for _ in range(2))
    return cfg, samples, left, right, P, Pr


def timed(fn, iters, warmup):
    import torch
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
    return statistics.median(ms), min(ms)


def child_device(iters, warmup):
    import ctypes
    import torch
    from snvc_amd import _roicrop
    from snvc_amd._lib import check
    from snvc_amd.geometry import RoICropper
    dev = torch.device("cuda:0")
    out = {"case": "device", "iters": iters}
    for n in SIZES:
        cfg, samples, left, right, P, Pr = inputs(n)
        crop = RoICropper(cfg)
        s, pl, pr = (torch.from_numpy(a).to(dev) for a in (samples, P.reshape(1, 12), Pr.reshape(1, 12)))
        dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        L = _roicrop.lib()
        c = _roicrop.RoICropConfig()
        c.out_w, c.out_h, c.aspect_ratio = RES[0], RES[1], cfg.aspect_ratio
        c.grid_range[:] = list(cfg.grid_range)
        desc = torch.tensor([[d.data_ptr(), d.shape[0] | (d.shape[1] << 32), d.stride(0)] for d in (dl, dr)], dtype=torch.int64).to(dev)
        table = crop.norm_table.to(dev)
        rois = [torch.empty((n, 3, RES[1], RES[0]), dtype=torch.float32, device=dev) for _ in range(2)]
        trans = [torch.empty((n, 2, 3), dtype=torch.float64, device=dev) for _ in range(2)]
        kpts = [torch.empty((n, 9, 2), dtype=torch.float64, device=dev) for _ in range(2)]
        local = [torch.empty((n, 9, 2), dtype=torch.float32, device=dev) for _ in range(2)]
        ws = torch.empty(L.snvc_roicrop_workspace_bytes(n), dtype=torch.uint8, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        call = lambda: check(L.snvc_roicrop(ctypes.byref(c), p(desc[0]), p(desc[1]), 1, None, p(s), p(pl), p(pr), n, p(table), p(ws),  # noqa: E731
                                            p(rois[0]), p(rois[1]), p(trans[0]), p(trans[1]), p(kpts[0]), p(kpts[1]), p(local[0]),
                                            p(local[1]), stream))
        out[f"call_{n}"] = timed(call, iters, warmup)
        out[f"generate_{n}"] = timed(lambda: crop.generate(s, dl, dr, pl, pr, dev), iters, warmup)
        got = crop.generate(s, dl, dr, pl, pr, dev)
        assert torch.equal(got[0], rois[0]) and torch.equal(got[1], rois[1])
    print("RESULT " + json.dumps(out))


def child_torch(iters, warmup):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from snvc_amd.geometry import RoICropper
    dev = torch.device("cuda:0")
    out = {"case": "torch", "iters": iters}
    for n in SIZES:
        cfg, samples, left, right, P, Pr = inputs(n)
        crop = RoICropper(cfg)
        dl, dr = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        _, _, meta = crop.generate(samples, dl, dr, P, Pr, dev)
        mean = torch.tensor(cfg.img_mean, device=dev).reshape(1, 3, 1, 1)
        std = torch.tensor(cfg.img_std, device=dev).reshape(1, 3, 1, 1)
        u, v = torch.arange(RES[0], device=dev, dtype=torch.float64), torch.arange(RES[1], device=dev, dtype=torch.float64)
        grids = []
        for t in (meta["trans_l"], meta["trans_r"]):
            xs = (u.reshape(1, 1, -1) - t[:, 0, 2].reshape(-1, 1, 1)) / t[:, 0, 0].reshape(-1, 1, 1)
            ys = (v.reshape(1, -1, 1) - t[:, 1, 2].reshape(-1, 1, 1)) / t[:, 1, 1].reshape(-1, 1, 1)
            gx = (xs / (IMAGE[1] - 1) * 2 - 1).expand(n, RES[1], RES[0])
            gy = (ys / (IMAGE[0] - 1) * 2 - 1).expand(n, RES[1], RES[0])
            grids.append(torch.stack([gx, gy], dim=3).float().contiguous())

        def run():
            res = []
            for img, grid in zip((dl, dr), grids):
                f = img.permute(2, 0, 1).unsqueeze(0).float().div(255)
                res.append((F.grid_sample(f.expand(n, 3, *IMAGE), grid, mode="bilinear", padding_mode="zeros", align_corners=True) - mean) / std)
            return res
        out[f"torch_{n}"] = timed(run, iters, warmup)
        ours = crop.generate(samples, dl, dr, P, Pr, dev, interpolation="exact")[0]
        out[f"maxdiff_{n}"] = float((run()[0] - ours).abs().max())       # in units of std: a float blend against a uint8-rounded one
    print("RESULT " + json.dumps(out))


def child_hbm():
    import torch
    buf = torch.empty(1 << 30, dtype=torch.uint8, device="cuda:0")
    med, best = timed(buf.zero_, 20, 3)
    print("RESULT " + json.dumps({"case": "hbm", "write_gbs": (1 << 30) / (med * 1e-3) / 1e9, "best_gbs": (1 << 30) / (best * 1e-3) / 1e9}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roicrop", "bench_roicrop.txt"))
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return {"device": lambda: child_device(args.iters, args.warmup), "torch": lambda: child_torch(args.iters, args.warmup),
                "hbm": child_hbm}[args.child]()
    rows = {}
    for name in ("device", "torch", "hbm"):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(args.iters),
                            "--warmup", str(args.warmup)], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit(f"bench_roicrop: case {name} failed (exit status {r.returncode}); nothing more is started")
        rows[name] = json.loads(line[0][7:])
    d, t, h = rows["device"], rows["torch"], rows["hbm"]
    text = [f"RoI crops of {RES[0]} x {RES[1]} from a {IMAGE[0]} x {IMAGE[1]} uint8 stereo pair, both sides, normalised float32; median (min) of "
            f"{d['iters']} event-timed calls after {args.warmup} warm-up: time on the stream, host issue included, not kernel time",
            f"measured write rate of this box (1 GiB zero_()): {h['write_gbs']:.0f} GB/s median, {h['best_gbs']:.0f} GB/s best",
            f"{'N':>3s} {'MB stored':>10s} {'store floor us':>15s} {'snvc_roicrop us':>22s} {'generate() us':>22s} {'grid_sample+norm us':>22s} "
            f"{'call / floor':>13s} {'torch / call':>13s}"]
    for n in SIZES:
        nbytes = n * 2 * 3 * RES[0] * RES[1] * 4
        floor = nbytes / (h["write_gbs"] * 1e9) * 1e6
        c, g, tt = d[f"call_{n}"], d[f"generate_{n}"], t[f"torch_{n}"]
        text.append(f"{n:3d} {nbytes / 1e6:10.2f} {floor:15.2f} {c[0] * 1e3:12.1f} ({c[1] * 1e3:7.1f}) {g[0] * 1e3:12.1f} ({g[1] * 1e3:7.1f}) "
                    f"{tt[0] * 1e3:12.1f} ({tt[1] * 1e3:7.1f}) {c[0] * 1e3 / floor:13.1f} {tt[0] / c[0]:13.1f}")
    text.append("largest |grid_sample result - 'exact' crop| per N, in units of the normalised output (one uint8 step is about 0.017): "
                + ", ".join(f"{t[f'maxdiff_{n}']:.4f}" for n in SIZES))
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
