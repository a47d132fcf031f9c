"""Time of ``oriented_iou_loss.cal_diou`` for M = 64 and M = 4096 seeded box pairs, forward alone and forward + backward, by two
routes alternated in one process:

  hip    the HIP route: one launch forward, one backward (include/snvc_oiou.h);
  torch  the same module's torch route on the same GPU tensors (``loss3d._torch_route()``): the vectorised clip and the
         28-line enclosing search as a few hundred small torch launches.

    python tools/bench_oriented_iou.py [--rounds 20] [--calls 20] [--warmup 5] [--out profiles/oriented_iou/bench.txt]

The parent process only starts the child (a fresh process, under its own timeout) and writes its lines; a child that fails
ends the run.  Per round and route, `--calls` consecutive calls run between two device events; reported is the median over the
rounds of the time per call, with quartiles and minimum.  That is time on the stream with the host's issue included, not
kernel time: at these sizes a call is bound by launches, on both routes.  Launches per call are the device-side kernel events
torch's profiler records over ten calls (for forward + backward that includes the few launches of ``(loss * g).sum()`` and its
backward, on both routes).  Before anything is timed the two routes' results are compared.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (64, 4096)


def boxes(m):
    import numpy as np
    r = np.random.default_rng(m)
    b = np.stack([r.uniform(-20, 20, m), r.uniform(-20, 20, m), r.uniform(1.5, 2.5, m), r.uniform(3.5, 5.0, m), r.uniform(-3.1, 3.1, m)], axis=1)
    a = b + np.concatenate([r.normal(0, 0.5, (m, 4)), r.normal(0, 0.3, (m, 1))], axis=1)
    return a.astype(np.float32), b.astype(np.float32)


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median": statistics.median(xs), "q1": q[0], "q3": q[2], "min": min(xs)}


def child(rounds, calls, warmup):
    import contextlib
    import torch
    from snvc_amd.models import loss3d
    from snvc_amd.thirdparty import oriented_iou_loss as O
    dev = torch.device("cuda:0")

    def on(route, call):
        with (loss3d._torch_route() if route == "torch" else contextlib.nullcontext()):
            return call()

    def launches(route, call):
        try:
            from torch.profiler import ProfilerActivity, profile
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(10):
                    on(route, call)
                torch.cuda.synchronize()
            from torch.autograd import DeviceType
            kernels = [e for e in prof.events() if e.device_type == DeviceType.CUDA and "memcpy" not in e.name.lower()
                       and "memset" not in e.name.lower()]
            names = [e.name[e.name.index("oiou"):].split("(")[0] for e in kernels if "oiou" in e.name]
            named = [f"{names.count(n) / 10:g} x {n}" for n in sorted(set(names))]
            return {"per_call": len(kernels) / 10 if kernels else "not measured (no device-side events)", "oiou_kernels": named}
        except Exception as e:      # the figure is "not measured" then, the times stand
            return {"per_call": f"not measured ({type(e).__name__})", "oiou_kernels": []}

    result = {}
    for m in SIZES:
        a_h, b_h = boxes(m)
        a = torch.from_numpy(a_h).to(dev)[None].requires_grad_(True)
        b = torch.from_numpy(b_h).to(dev)[None]
        g = torch.rand(1, m, device=dev)

        def forward():
            with torch.no_grad():
                return O.cal_diou(a, b)[0]

        def both():
            a.grad = None
            loss = O.cal_diou(a, b)[0]
            (loss * g).sum().backward()
            return a.grad

        for name, call in ((f"M = {m}, forward", forward), (f"M = {m}, forward + backward", both)):
            x, y = on("hip", call).clone(), on("torch", call).clone()
            diff = float((x - y).abs().max() / y.abs().max())
            for _ in range(warmup):
                on("hip", call), on("torch", call)
            times = {"hip": [], "torch": []}
            for _ in range(rounds):
                for route in ("hip", "torch"):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(calls):
                        on(route, call)
                    e1.record()
                    e1.synchronize()
                    times[route].append(e0.elapsed_time(e1) * 1e-3 / calls)
            result[name] = {"hip": quartiles(times["hip"]), "torch": quartiles(times["torch"]), "rel_diff": diff,
                            "launches": {r: launches(r, call) for r in ("hip", "torch")}}
    print("RESULT " + json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oriented_iou", "bench.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.rounds, args.calls, args.warmup)
    r = subprocess.run(["timeout", "-k", "10", "400", sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds),
                        "--calls", str(args.calls), "--warmup", str(args.warmup)], capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"bench_oriented_iou: the child failed (exit status {r.returncode})")
    d = json.loads(line[0][7:])
    us = lambda q: f"{q['median'] * 1e6:9.1f} us median, quartiles {q['q1'] * 1e6:.1f} .. {q['q3'] * 1e6:.1f}, min {q['min'] * 1e6:.1f}"  # noqa: E731
    text = [f"cal_diou on seeded box pairs; per call, {args.calls} consecutive calls between two device events (host issue included, not "
            f"kernel time), median of {args.rounds} rounds, routes alternated in one process after {args.warmup} warm-up calls each"]
    for name, v in d.items():
        text.append(f"{name}:")
        for route, label in (("hip", "HIP route  "), ("torch", "torch route")):
            n = v["launches"][route]
            text.append(f"  {label} {us(v[route])}; launches per call {n['per_call']}"
                        + (f" (of them this module's: {', '.join(n['oiou_kernels'])})" if n["oiou_kernels"] else ""))
        ratio = v["torch"]["median"] / v["hip"]["median"]
        text.append(f"  torch / HIP = {ratio:.1f}" + ("" if ratio > 1 else "  (the HIP route is NOT faster here)")
                    + f"; largest |HIP - torch| over largest |torch| = {v['rel_diff']:.2g}")
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
