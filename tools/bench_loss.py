"""Forward + backward time of every HIP loss at its working size (tests/loss_cases.py WORK) beside a stock-torch
composition of the same formula on the same GPU, written here and not routed through the module under test.

    python tools/bench_loss.py [--iters 50] [--warmup 10] [--out profiles/loss/bench_loss.txt]

The parent process only starts one child per case (a fresh process, under its own timeout) and collects their lines; a child
that fails ends the run.  In a child: warm-up, then per iteration two device events around forward + backward, the median
over the iterations.  That is the time of the call, which includes the host's time to issue the launches; it is not kernel
time, so no HBM rate is derived from it (that needs a kernel trace).  "MB to move" is what the kernels must read and write
(every operand once per direction, each gradient once), for scale.  The stock-torch baseline keeps the reference's host
waits (`if mask.sum() > 0`, one assert per part in VoxelMSELossWeighted): removing them is part of what is measured.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def torch_formula(kind, o, d, c):
    """The reference's way of computing the loss, in stock torch ops (boolean-mask gathers and all)."""
    import torch
    import torch.nn.functional as F
    if kind == "mse":
        p, g = d["pred"], c["gt"]
        n, k = p.shape[:2]
        p, g = p.reshape(n, k, -1), g.reshape(n, k, -1)
        total = 0
        for i in range(k):
            a, b = p[:, i], g[:, i]
            total = total + (F.mse_loss(a * c["tw"][i], b * c["tw"][i]) if "tw" in c else F.mse_loss(a, b))
        return total / k
    if kind == "msew":
        p, g = d["pred"], c["gt"]
        n, k = p.shape[:2]
        p, g = p.reshape(n, k, -1), g.reshape(n, k, -1)
        total = 0
        for i in range(k):
            a, b = p[:, i], g[:, i]
            pos, rest = b > 0, b <= 0
            assert pos.sum() > 0
            total = total + 0.5 * (F.mse_loss(a[pos], b[pos]) + F.mse_loss(a[rest], b[rest]))
        return total / k
    if kind == "occ":
        p, t = d["pred"], c["gt"]
        loss = -(t == 1).float() * ((1 - p) ** 2. * torch.log(p + 1e-7)) * 0.25 - (t == 0).float() * (p ** 2. * torch.log(1 - p + 1e-7)) * 0.75
        mask = t != -1
        return loss[mask].mean() if mask.sum() > 0 else 0.
    if kind == "offset":
        p, g = d["pred"], c["gt"]
        loss = F.l1_loss(p.reshape(g.shape), g, reduction="none")
        mask = (c["occ"][:, None, None] == 1).repeat(1, 3, g.shape[2], 1, 1, 1)
        return loss[mask].mean() if mask.sum() > 0 else 0.
    if kind == "wloss":
        off, prob = d["off"].permute(0, 2, 3, 1), d["prob"].permute(0, 2, 3, 1)
        depth = c["levels"][None, None, None, :] + off
        m = c["mask"]
        return torch.sum(prob[m] * torch.abs(depth[m] - c["target"].unsqueeze(3)[m]), 1).mean()
    if kind == "depthreg":
        depth = torch.sum(F.softmax(d["cost"], 1) * c["levels"][None, :, None, None], 1)
        gt = c["gt"]
        m = (gt != -1) & (gt < 60.)
        return F.smooth_l1_loss(depth[m], gt[m]) if m.sum() > 0 else 0.
    raise KeyError(kind)


def moved_bytes(x):
    """Forward reads every operand once; backward reads them again and writes one gradient per differentiable operand."""
    read = sum(t.numel() * t.element_size() for t in list(x["diff"].values()) + list(x["const"].values()))
    return 2 * read + sum(t.numel() * t.element_size() for t in x["diff"].values())


def child(name, iters, warmup):
    import torch
    import loss_cases as LC
    from snvc_amd.models import loss3d
    kind, o = LC.CASES[name]
    x = LC.inputs(name, torch.float32, "cuda:0")
    d, c = x["diff"], x["const"]

    def timed(fn):
        def once():
            for t in d.values():
                t.grad = None
            fn().backward()
        for _ in range(warmup):
            once()
        torch.cuda.synchronize()
        ms = []
        for _ in range(iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            once()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), min(ms)

    hip, hip_min = timed(lambda: LC.call(loss3d, name, x))
    ref, ref_min = timed(lambda: torch_formula(kind, o, d, c))
    nbytes = moved_bytes(x)
    print("RESULT " + json.dumps({"case": name, "hip_ms": hip, "hip_min_ms": hip_min, "torch_ms": ref, "torch_min_ms": ref_min, "bytes": nbytes,
                                  "iters": iters}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss", "bench_loss.txt"))
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.iters, args.warmup)
    import loss_cases as LC
    rows = []
    for name in sorted(LC.WORK):
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--iters", str(args.iters),
                            "--warmup", str(args.warmup)], capture_output=True, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            sys.exit(f"bench_loss: case {name} failed (exit status {r.returncode}); nothing more is started")
        rows.append(json.loads(line[0][7:]))
    head = f"{'case':14s} {'HIP call ms':>12s} {'torch call ms':>14s} {'ratio':>7s} {'MB to move':>11s}"
    text = [f"forward + backward call time (host issue included; not kernel time), median of {args.iters} iterations after "
            f"{args.warmup} warm-up, device events; the torch column includes the reference's host waits", head]
    for r in rows:
        text.append(f"{r['case']:14s} {r['hip_ms']:12.4f} {r['torch_ms']:14.4f} {r['torch_ms'] / r['hip_ms']:6.1f}x {r['bytes'] / 1e6:11.1f}")
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
