"""Time of the FC box head (snvc_amd.models.FCmodel) on its HIP route and on the torch route of the same module
(``FC_HIP[0] = False``), alternated in one process:

  * eval calls at N = 64 for get_fc_model() (18 -> 128 -> 5, one block) and for the class defaults (32 -> 1024 -> 64, two blocks);
  * one training step (forward, backward of sum(out * g)) of get_fc_model() at N = 64, p = 0.5.

    python tools/bench_fc.py [--rounds 40] [--calls 50] [--warmup 20] [--out profiles/fc_head/bench_fc.txt]

The parent process only starts the child (a fresh process, under its own timeout) and writes its lines.  Each round times
`--calls` consecutive calls of one route between two device events, then the same of the other route, on the same tensors;
reported per call: the median over the rounds, the quartiles and the minimum.  That is time on the stream with the host's
issue included, not kernel time: for launches of a few microseconds the host side is most of it.  Launches per call are
the device-side kernel events torch's profiler records over ten calls (for the training step that includes drawing the masks
and the functional's own few launches, on both routes).  Before anything is timed the two routes' results are compared.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 64


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median": statistics.median(xs), "q1": q[0], "q3": q[2], "min": min(xs)}


def child(rounds, calls, warmup):
    import torch
    from snvc_amd.models import FCmodel
    dev = torch.device("cuda:0")
    torch.manual_seed(0)

    def randomised(m):
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.normal_(0, 0.5)
                mod.running_var.uniform_(0.5, 2.0)
                mod.weight.data.uniform_(0.5, 1.5)
                mod.bias.data.normal_(0, 0.2)
        return m.to(dev)

    def eval_call(m, x):
        def call():
            with torch.no_grad():
                return m(x)
        return call

    def train_call(m, x, g):
        def call():
            for p in m.parameters():
                p.grad = None
            out = m(x)
            (out * g).sum().backward()
            return out
        return call

    head, big, trained = randomised(FCmodel.get_fc_model()).eval(), randomised(FCmodel.FCModel()).eval(), randomised(FCmodel.get_fc_model()).train()
    x18, x32 = torch.rand(N, 18, device=dev), torch.rand(N, 32, device=dev)
    g = torch.randn(N, 5, device=dev)
    work = {"eval get_fc_model()": eval_call(head, x18), "eval FCModel() defaults": eval_call(big, x32),
            "train step get_fc_model()": train_call(trained, x18.clone().requires_grad_(True), g)}

    def on(route, call):
        FCmodel.FC_HIP[0] = route == "hip"
        try:
            return call()
        finally:
            FCmodel.FC_HIP[0] = True

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
            return len(kernels) / 10 if kernels else "not measured (no device-side events)"
        except Exception as e:      # the figure is "not measured" then, the times stand
            return f"not measured ({type(e).__name__})"

    result = {}
    for name, call in work.items():
        for _ in range(warmup):
            a, b = on("hip", call), on("torch", call)
        diff = float((a - b).abs().max() / b.abs().max()) if not name.startswith("train") else None      # a step draws its own masks
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
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_head", "bench_fc.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.rounds, args.calls, args.warmup)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(args.rounds),
                        "--calls", str(args.calls), "--warmup", str(args.warmup)], capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"bench_fc: the child failed (exit status {r.returncode})")
    d = json.loads(line[0][7:])
    us = lambda q: f"{q['median'] * 1e6:8.1f} us median, quartiles {q['q1'] * 1e6:.1f} .. {q['q3'] * 1e6:.1f}, min {q['min'] * 1e6:.1f}"  # noqa: E731
    text = [f"FC box head, N = {N} rows; per call, {args.calls} consecutive calls between two device events (host issue included, not kernel "
            f"time), {args.rounds} rounds, routes alternated in one process after {args.warmup} warm-up calls each"]
    for name, v in d.items():
        text.append(f"{name}:")
        text.append(f"  HIP route   {us(v['hip'])}; launches per call {v['launches']['hip']}")
        text.append(f"  torch route {us(v['torch'])}; launches per call {v['launches']['torch']}")
        ratio = v["torch"]["median"] / v["hip"]["median"]
        text.append(f"  torch / HIP = {ratio:.2f}" + ("" if ratio > 1 else "  (the HIP route is NOT faster here)")
                    + (f"; largest |HIP - torch| over largest |torch| = {v['rel_diff']:.2g}" if v["rel_diff"] is not None else ""))
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
