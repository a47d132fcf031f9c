"""Time of the box read-out for N = 64 instances of 9 parts with 192 x 128 maps (seeded), by two routes alternated in one process:

  (a) decode.ncf_to_update_2d on the device ncf: argmax_rows + aminmax on the device, three blocking copies, the pose fit in
      numpy on the host;
  (b) decode.refine_boxes followed by one synchronise: one scan of the maps and one fit per instance on the device
      (include/snvc_decode.h), nothing copied back.

    python tools/bench_decode.py [--seconds 1.0] [--warmup 10] [--out profiles/decode/bench_decode.txt]

The parent process only starts the child (a fresh process, under its own timeout) and writes its lines; a child that fails
ends the run.  Each round runs (a) once, then (b) as often as fits into (a)'s time, on the same device tensors, each between two host clock readings that
end in a synchronise ((a) ends in its own copies); rounds are repeated until each route has filled `--seconds`.  Reported: the
median, the quartiles and the minimum per call.  The scan's share of the 6.3 TB/s HBM peak is its N * P * M * 4 bytes over the
device-event time of the C call alone (outputs and workspace allocated once): that is time on the stream for both launches,
host issue included, not kernel time, and the 57 MB of maps may be served from cache on a repeated read.
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

N, PARTS, NL, NW = 64, 9, 192, 128
HBM_PEAK = 6.3e12


def inputs():
    import types
    import numpy as np
    r = np.random.default_rng(5)
    cfg = types.SimpleNamespace(x_range=(-1.6, 1.6), z_range=(-2.4, 2.4))
    ncf = r.uniform(0.0, 1.0, (N, PARTS, NL, NW)).astype(np.float32)
    ncf[::8, 3, 7, 7] = 2.5             # every eighth instance fails the filter
    samples = np.stack([r.uniform(1.4, 1.7, N), r.uniform(1.5, 1.8, N), r.uniform(3.5, 4.5, N), r.uniform(-10, 10, N),
                        r.uniform(1.5, 1.9, N), r.uniform(6, 50, N), r.uniform(-3.0, 3.0, N)], axis=1)
    zs, xs = np.meshgrid(np.linspace(-2.4, 2.4, NL), np.linspace(-1.6, 1.6, NW), indexing="ij")
    grid = np.stack([xs.ravel(), np.zeros(NL * NW), zs.ravel()], axis=1)
    return cfg, ncf, samples, grid


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return {"median": statistics.median(xs), "q1": q[0], "q3": q[2], "min": min(xs), "calls": len(xs)}


def child(seconds, warmup):
    import ctypes
    import numpy as np
    import torch
    from snvc_amd import _decode
    from snvc_amd import decode as D
    from snvc_amd._lib import check
    dev = torch.device("cuda:0")
    cfg, ncf_h, samples, grid = inputs()
    ncf, s_dev, g_dev = (torch.from_numpy(a).to(dev) for a in (ncf_h, samples, grid))
    filt = D.Filter()

    def route_a():
        t0 = time.perf_counter()
        res = D.ncf_to_update_2d(cfg, ncf, samples, grid, filt)
        return time.perf_counter() - t0, 0.0, res

    def route_b():
        t0 = time.perf_counter()
        res = D.refine_boxes(cfg, ncf, s_dev, g_dev, filt)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, res

    for _ in range(warmup):
        est = route_a()[0], route_b()[0]
    per_round = max(1, round(est[0] / est[1]))       # calls of (b) per call of (a), so that both fill their time in the same rounds
    ta, tb, issue = [], [], []
    while (sum(ta) < seconds or sum(tb) < seconds) and len(ta) < 20000:
        ta.append(route_a()[0])
        for _ in range(per_round):
            t, i, _ = route_b()
            tb.append(t)
            issue.append(i)
    a, b = route_a()[2], D.to_update_dict(route_b()[2])
    assert np.array_equal(a["keep_flags"], b["keep_flags"]) and np.array_equal(a["confidence"], b["confidence"])
    diff = float(np.abs(np.asarray(a["pred"]["all_parts"]) - np.asarray(b["pred"]["all_parts"])).max())
    assert diff <= 1e-9, diff

    # the C call alone, between two device events
    L = _decode.lib()
    c = _decode.DecodeConfig()
    c.x_range[:], c.z_range[:], c.min_val, c.max_val, c.source = list(cfg.x_range), list(cfg.z_range), -1.0, 2.0, _decode.GRID
    m = NL * NW
    ws = torch.empty(L.snvc_decode_workspace_bytes(N, PARTS), dtype=torch.uint8, device=dev)
    conf = torch.empty((N, PARTS), dtype=torch.float32, device=dev)
    index = torch.empty((N, PARTS), dtype=torch.int64, device=dev)
    keep = torch.empty((N,), dtype=torch.bool, device=dev)
    one, both = (torch.empty((N, 7), dtype=torch.float64, device=dev) for _ in range(2))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    call = lambda: check(L.snvc_decode_boxes(ctypes.byref(c), p(ncf), p(s_dev), p(g_dev), N, PARTS, m, p(ws), p(conf), p(index),  # noqa: E731
                                             p(keep), p(one), p(both), stream), "snvc_decode_boxes")
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    ev = []
    for _ in range(200):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1) * 1e-3)
    print("RESULT " + json.dumps({"a": quartiles(ta), "b": quartiles(tb), "b_issue": quartiles(issue), "call": quartiles(ev),
                                  "max_box_diff": diff, "kept": int(a["keep_flags"].sum())}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode", "bench_decode.txt"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args.seconds, args.warmup)
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", "--seconds", str(args.seconds),
                        "--warmup", str(args.warmup)], capture_output=True, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"bench_decode: the child failed (exit status {r.returncode})")
    d = json.loads(line[0][7:])
    us = lambda q: f"{q['median'] * 1e6:9.1f} us median, quartiles {q['q1'] * 1e6:.1f} .. {q['q3'] * 1e6:.1f}, min {q['min'] * 1e6:.1f}, {q['calls']} calls"  # noqa: E731
    nbytes = N * PARTS * NL * NW * 4
    rate = nbytes / d["call"]["median"]
    a, b = d["a"]["median"], d["b"]["median"]
    text = [f"box read-out, N = {N} instances x {PARTS} parts x {NL} x {NW} maps ({nbytes / 1e6:.1f} MB), {d['kept']} kept; host clock per call, each call "
            f"ending in a synchronise, routes alternated in one process after {args.warmup} warm-up rounds, about {args.seconds:g} s each",
            f"(a) ncf_to_update_2d on the device ncf (device scans, three copies, numpy fit): {us(d['a'])}",
            f"(b) refine_boxes + synchronise (scan + fit on the device):                      {us(d['b'])}",
            f"    of which until refine_boxes returns (six allocations, two launches queued): {us(d['b_issue'])}",
            f"(a) / (b) = {a / b:.1f}; per instance (a) {a / N * 1e6:.1f} us, (b) {b / N * 1e6:.2f} us; largest |(a) - (b)| over the boxes {d['max_box_diff']:.3g}",
            f"snvc_decode_boxes alone between two device events (both launches, host issue included, not kernel time): {us(d['call'])}",
            f"the scan's {nbytes / 1e6:.1f} MB over that time: {rate / 1e9:.0f} GB/s = {100 * rate / HBM_PEAK:.1f} % of the 6.3 TB/s HBM peak "
            f"(two launches of a few microseconds each bound this from above at this size; the maps may be read from cache)"]
    if b >= a:
        text.append(f"(b) is NOT faster than (a) here: its {b * 1e6:.1f} us are {d['b_issue']['median'] * 1e6:.1f} us of host issue in refine_boxes (six torch allocations, "
                    f"the ctypes call) plus the wait for two launches, against (a)'s {a * 1e6:.1f} us; what (b) buys is that the boxes stay on the device")
    print("\n".join(text))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(text) + "\n")


if __name__ == "__main__":
    main()
