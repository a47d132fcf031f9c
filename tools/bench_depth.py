"""Time of the depth read-out (snvc_amd.depth) on its HIP route and on the torch composition (``DEPTH_HIP[0] = False``, the
"depth_readout_torch" route), alternated in one process, at two shapes:

  * cfg2's own cost volume, [1,192,96,312] -> (192,384,1248);
  * the DSGN form,          [1, 48,96,312] -> (192,384,1248).

For each: the forward (with the confidence), forward + backward of sum(depth * g), and depth_to_points(compact=True) against
its torch composition (the projection, the mask and ``points[valid]``, which waits for the device as boolean indexing must).

    python tools/bench_depth.py [--rounds 20] [--calls 5] [--warmup 5] [--out profiles/depth_head/bench_depth.txt]

The parent process only starts the child (a fresh process, under its own timeout) and writes its lines.  Each round times
`--calls` consecutive calls of one route between two device events, then the same of the other route, on the same tensors;
reported per call: the median over the rounds, the quartiles and the minimum.  That is time on the stream with the host's issue
included; at these shapes a call is far longer than its launch.  The bytes of a call are the ones the algorithm needs (inputs
read once, outputs written once), computed from the shapes; the rate is those bytes over the median, beside the HBM peak of
8 TB/s.  Before anything is timed the two routes' results are compared.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cfg2 [1,192,96,312] -> (192,384,1248)": ((1, 192, 96, 312), (192, 384, 1248)),
          "DSGN [1,48,96,312] -> (192,384,1248)": ((1, 48, 96, 312), (192, 384, 1248))}
HBM_PEAK = 8.0e12


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median": statistics.median(xs), "q1": q[0], "q3": q[2], "min": min(xs)}


def needed_bytes(cost_shape, out):
    n, d, h, w = cost_shape
    vol, px = n * d * h * w * 4, n * out[1] * out[2] * 4
    return {"forward": vol + 2 * px,                          # cost in; depth and confidence out
            "forward + backward": 3 * vol + 8 * px,  # cost in, depth, conf, m, z out; cost, depth, m, z, g in, d cost out
            "depth_to_points(compact)": 2 * px + 3 * px + n * 4,        # depth, confidence in; points, counts out
            "torch materialises": n * out[0] * out[1] * out[2] * 4}


def child(rounds, calls, warmup):
    import torch
    from snvc_amd import depth as D
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    P = torch.tensor([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]], device=dev)

    def on(route, call):
        D.DEPTH_HIP[0] = route == "hip"
        try:
            return call()
        finally:
            D.DEPTH_HIP[0] = True

    def points_torch(depth, conf):
        n, h, w = depth.shape
        u = torch.arange(w, dtype=torch.float32, device=dev)[None, None, :]
        v = torch.arange(h, dtype=torch.float32, device=dev)[None, :, None]
        x = ((u - P[0, 2]) * depth) / P[0, 0] + P[0, 3] / (-P[0, 0])
        y = ((v - P[1, 2]) * depth) / P[1, 1] + P[1, 3] / (-P[1, 1])
        valid = torch.isfinite(depth) & (depth >= 2.0) & (depth < 59.6) & (conf >= 0.1)
        return torch.stack([x, y, depth], -1)[valid]

    result = {}
    for name, (cost_shape, out) in SHAPES.items():
        cost = (4.0 * torch.randn(cost_shape, device=dev)).requires_grad_(True)
        levels = torch.linspace(2.0, 59.6, out[0], device=dev)
        g = torch.randn((cost_shape[0],) + out[1:], device=dev)

        def forward():
            with torch.no_grad():
                return D.depth_readout(cost, levels, size=out[1:], confidence=True)

        def step():
            cost.grad = None
            D.depth_readout(cost, levels, size=out[1:]).backward(g)
            return cost.grad

        depth, conf = forward()
        pts_call = {"hip": lambda: D.depth_to_points(depth, P, conf=conf, min_conf=0.1, z_range=(2.0, 59.6), compact=True),
                    "torch": lambda: points_torch(depth, conf)}
        work = {"forward": {"hip": forward, "torch": forward}, "forward + backward": {"hip": step, "torch": step},
                "depth_to_points(compact)": pts_call}
        result[name] = {"bytes": needed_bytes(cost_shape, out)}
        for what, call in work.items():
            for _ in range(warmup):
                a, b = on("hip", call["hip"]), on("torch", call["torch"])
            if what == "forward":
                diff = float((a[0] - b[0]).abs().max() / b[0].abs().max())
            elif what == "forward + backward":
                diff = float((a - b).abs().max() / b.abs().max())
            else:
                pts, counts = a
                same = int(counts[0]) == b.shape[0] and torch.equal(pts[0, :b.shape[0]], b)
                diff = 0.0 if same else float("nan")
            times = {"hip": [], "torch": []}
            for _ in range(rounds):
                for route in ("hip", "torch"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        on(route, call[route])
                    e1.record()
                    e1.synchronize()
                    times[route].append(e0.elapsed_time(e1) * 1e-3 / calls)
            result[name][what] = {"hip": quartiles(times["hip"]), "torch": quartiles(times["torch"]), "rel_diff": diff}
    print("RESULT " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_head", "bench_depth.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.rounds, args.calls, args.warmup)
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds),
                        "--calls", str(args.calls), "--warmup", str(args.warmup)], capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"bench_depth: the child failed (exit status {r.returncode})")
    d = json.loads(line[0][7:])
    us = lambda q: f"{q['median'] * 1e6:9.1f} us median, quartiles {q['q1'] * 1e6:.1f} .. {q['q3'] * 1e6:.1f}, min {q['min'] * 1e6:.1f}"  # noqa: E731
    text = [f"Depth read-out; per call, {args.calls} consecutive calls between two device events (host issue included), {args.rounds} rounds, "
            f"routes alternated in one process after {args.warmup} warm-up calls each"]
    for name, v in d.items():
        text.append(f"{name}:  (the torch route materialises {v['bytes']['torch materialises'] / 1e6:.0f} MB and passes over it several times)")
        for what in ("forward", "forward + backward", "depth_to_points(compact)"):
            w, need = v[what], v["bytes"][what]
            rate = need / w["hip"]["median"]
            text.append(f"  {what}: needs {need / 1e6:.1f} MB")
            text.append(f"    HIP route   {us(w['hip'])}; {rate / 1e12:.3f} TB/s of needed bytes = {100 * rate / HBM_PEAK:.1f} % of the 8 TB/s HBM peak")
            text.append(f"    torch route {us(w['torch'])}")
            ratio = w["torch"]["median"] / w["hip"]["median"]
            text.append(f"    torch / HIP = {ratio:.2f}" + ("" if ratio > 1 else "  (the HIP route is NOT faster here)")
                        + (f"; largest |HIP - torch| over largest |torch| = {w['rel_diff']:.2g}" if what != "depth_to_points(compact)"
                           else f"; compacted rows equal points[valid]: {w['rel_diff'] == 0.0}"))
    f192, f48 = (d[k]["forward"]["hip"]["median"] for k in SHAPES)
    text.append(f"forward, 192 input planes over 48 input planes (same 192 output planes, same exponentials, four times the LDS reads and "
                f"staged bytes): {f192 / f48:.2f}")
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
