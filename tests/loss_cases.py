"""Case table of the loss tests, seeded inputs, the call of each loss through a loss3d-shaped module, and a float64
restatement of every loss written from its formula (masks as 0/1 factors, sums over everything, one division): no boolean
gather, no per-part loop.  Shared by tests/golden/make_golden_loss.py (which calls the reference through ``call``),
tests/test_loss_host.py and tests/test_gpu_loss.py.

A case is (kind, options).  ``inputs(name, dtype, device)`` builds its tensors from the case's seed (drawn in float64 on the
CPU, rounded to float32 values, then cast), so the golden file stores results only."""
import types

import torch

# name -> (kind, options); "work": a working-size case (GPU tests only, not in the golden file)
SMALL = {
    "mse": ("mse", dict(n=2, k=3, vol=(4, 5, 6), seed=11)),
    "mse_odd": ("mse", dict(n=3, k=2, vol=(3, 5, 7), seed=12)),
    "mse_w_part": ("mse", dict(n=2, k=3, vol=(4, 5, 6), seed=13, tw="part")),
    "mse_w_rows": ("mse", dict(n=2, k=3, vol=(4, 5, 6), seed=14, tw="rows")),
    "msew": ("msew", dict(n=2, k=3, vol=(4, 5, 6), seed=21, pos=0.2)),
    "msew_odd": ("msew", dict(n=3, k=2, vol=(3, 5, 7), seed=22, pos=0.1)),
    "msew_tail": ("msew", dict(n=2, k=2, vol=(4100,), seed=24, pos=0.1)),                   # rows of 4096 + 4 elements
    "msew_w_rows": ("msew", dict(n=2, k=3, vol=(4, 5, 6), seed=23, pos=0.2, tw="rows")),
    "occ": ("occ", dict(n=2, vol=(4, 6, 10), seed=31, ignore=0.3, pos=0.2)),
    "occ_odd": ("occ", dict(n=1, vol=(3, 5, 7), seed=32, ignore=0.5, pos=0.4, gamma=2.0, alpha=0.4)),
    "occ_edge": ("occ", dict(n=2, vol=(4, 6, 10), seed=33, ignore=0.3, pos=0.3, edge=True)),
    "occ_tail": ("occ", dict(n=1, vol=(2, 2, 2049), seed=35, ignore=0.3, pos=0.2)),          # 2 * 4096 + 4 elements: a partial last tile
    "occ_empty": ("occ", dict(n=1, vol=(2, 3, 4), seed=34, ignore=1.0, pos=0.0)),
    "offset": ("offset", dict(n=2, parts=3, vol=(4, 5, 6), seed=41, occ=0.3)),
    "offset_odd": ("offset", dict(n=1, parts=2, vol=(3, 5, 7), seed=42, occ=0.5)),
    "offset_empty": ("offset", dict(n=1, parts=1, vol=(2, 3, 4), seed=43, occ=0.0)),
    "depth": ("depth", dict(n=2, hw=(6, 10), seed=51, invalid=0.3)),
    "depth_odd": ("depth", dict(n=1, hw=(5, 7), seed=52, invalid=0.5)),
    "depth_empty": ("depth", dict(n=1, hw=(3, 4), seed=53, invalid=1.0)),
    "w_mean": ("wloss", dict(b=2, d=5, hw=(4, 6), seed=61, masked=0.6, reduction="mean")),
    "w_mean_odd": ("wloss", dict(b=1, d=11, hw=(3, 7), seed=62, masked=0.5, reduction="mean")),
    "w_none": ("wloss", dict(b=2, d=5, hw=(4, 6), seed=63, masked=0.6, reduction="none")),
    "disp_sl1": ("disp", dict(b=2, hw=(4, 6), seed=71, masked=0.6, preds=3)),
    "disp_sl1_two": ("disp", dict(b=1, hw=(5, 7), seed=72, masked=0.5, preds=2)),
    "disp_w1": ("disp_w1", dict(b=2, d=5, hw=(4, 6), seed=73, masked=0.6)),
    "focal": ("focal", dict(rows=40, cols=12, seed=81, pos=0.1, target="int32")),
    "focal_i64": ("focal", dict(rows=9, cols=12, seed=83, pos=0.2, target="int64")),
    "focal_bool": ("focal", dict(rows=21, cols=5, seed=84, pos=0.2, target="bool")),
    "focal_w": ("focal", dict(rows=13, cols=7, seed=82, pos=0.2, target="float", weights=True)),
    "sl1rows": ("sl1rows", dict(rows=10, cols=24, seed=91, beta=1. / 9)),
    "sl1rows_odd": ("sl1rows", dict(rows=7, cols=7, seed=92, beta=0.5)),
    "depthreg": ("depthreg", dict(b=2, d=12, hw=(4, 6), seed=101, invalid=0.3)),
    "depthreg_few": ("depthreg", dict(b=1, d=5, hw=(3, 7), seed=102, invalid=0.4)),
    "depthreg_deep": ("depthreg", dict(b=1, d=300, hw=(2, 5), seed=103, invalid=0.2)),
    "coord": ("coord", dict(n=5, seed=111, normalize=False)),
    "coord_norm": ("coord", dict(n=5, seed=112, normalize=True)),
    "shape": ("shape", dict(n=4, seed=121)),
    "bbox": ("bbox", dict(n=6, seed=131)),
}

# Working sizes: N = 4 crops of the released local model's 32 x 128 x 192 grid, N x 9 x 128 x 192 heat maps, and the cost
# volume of the benchmark's cfg2 workload (benchlib.common: D, H, W = 192, 96, 312).
WORK = {
    "occ_work": ("occ", dict(n=4, vol=(32, 128, 192), seed=201, ignore=0.3, pos=0.1)),
    "offset_work": ("offset", dict(n=4, parts=1, vol=(32, 128, 192), seed=202, occ=0.1)),
    "mse_work": ("mse", dict(n=4, k=9, vol=(128, 192), seed=203)),
    "mse_w_work": ("mse", dict(n=4, k=9, vol=(128, 192), seed=204, tw="rows")),
    "msew_work": ("msew", dict(n=4, k=9, vol=(128, 192), seed=205, pos=0.05)),
    "w_work": ("wloss", dict(b=1, d=192, hw=(96, 312), seed=206, masked=0.6, reduction="mean")),
    "depthreg_work": ("depthreg", dict(b=1, d=192, hw=(96, 312), seed=207, invalid=0.3)),
}

CASES = dict(SMALL, **WORK)
HIP_KINDS = ("mse", "msew", "occ", "offset", "depth", "wloss", "disp", "disp_w1", "focal", "sl1rows", "depthreg")
COORD_CFG = types.SimpleNamespace(x_range=(-3.0, 5.0), z_range=(-4.0, 6.0), head_reg_type="vector")


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=torch.float64)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def inputs(name, dtype=torch.float64, device="cpu"):
    """{"diff": {name: tensor that wants a gradient}, "const": {name: tensor}} for the case."""
    kind, o = CASES[name]
    g = torch.Generator().manual_seed(o["seed"])
    diff, const = {}, {}
    if kind in ("mse", "msew"):
        shape = (o["n"], o["k"]) + tuple(o["vol"])
        diff["pred"] = _rand(g, *shape)
        gt = _rand(g, *shape)
        if kind == "msew":
            gt = torch.where(_rand(g, *shape) < o["pos"], gt, -gt * (_rand(g, *shape) < 0.5))      # positives, zeros and negatives
            gt.reshape(o["n"], o["k"], -1)[:, :, 0] = 0.5                                            # every part has a positive
        const["gt"] = gt
        if o.get("tw") == "part":
            const["tw"] = 0.5 + _rand(g, o["k"])
        elif o.get("tw") == "rows":
            const["tw"] = (_rand(g, o["k"], o["n"], 1) < 0.8) * (0.5 + _rand(g, o["k"], o["n"], 1))
    elif kind == "occ":
        shape = (o["n"],) + tuple(o["vol"])
        p = 0.02 + 0.96 * _rand(g, *shape)            # no saturated prediction: no gradient carries the 1 / 1e-7 factor
        u = _rand(g, *shape)
        t = torch.where(u < o["ignore"], -1.0, torch.where(u < o["ignore"] + o["pos"] * (1 - o["ignore"]), 1.0, 0.0)).to(torch.float64)
        if o.get("edge"):
            flat = p.reshape(-1)
            flat[0::7] = 0.0                          # exact 0 and exact 1 at ignored and at counted elements of both classes
            flat[3::7] = 1.0
        diff["pred"], const["gt"] = p, t
    elif kind == "offset":
        vol = tuple(o["vol"])
        diff["pred"] = _randn(g, o["n"], 3 * o["parts"], *vol)
        const["gt"] = _randn(g, o["n"], 3, o["parts"], *vol)
        occupied = (_rand(g, o["n"], *vol) < o["occ"]).to(torch.float64)
        const["occ"] = torch.where(_rand(g, o["n"], *vol) < 0.2, -occupied, occupied)      # -1 (unknown) counts as not occupied
    elif kind == "depth":
        shape = (o["n"],) + tuple(o["hw"])
        gt = 2.0 + 56.0 * _rand(g, *shape)
        u = _rand(g, *shape)
        gt = torch.where(u < o["invalid"] / 2, -1.0, torch.where(u < o["invalid"], 60.0 + 20.0 * u, gt)).to(torch.float64)
        diff["pred"] = torch.where(gt > 0, gt, 30.0) + 1.5 * _randn(g, *shape)     # errors on both sides of the smooth-L1 knee
        const["gt"] = gt
    elif kind in ("wloss", "disp_w1"):
        b, d, (h, w) = o["b"], o["d"], o["hw"]
        # |level + off - target| has a kink at 0, where the side (the gradient's sign) is decided by the rounding of level + off.
        # Levels, offsets and targets are multiples of 2^-10 below 64, so that the sum and the difference are exact in float32
        # as in float64 and both precisions stand on the same side of every kink.
        def q(t):
            return torch.round(t * 1024.0) / 1024.0
        diff["prob"] = torch.softmax(_randn(g, b, d, h, w), 1)
        diff["off"] = q(0.2 * _randn(g, b, d, h, w))
        const["levels"] = q(torch.linspace(2.0, 40.0, d, dtype=torch.float64))
        const["target"] = q(2.0 + 38.0 * _rand(g, b, h, w))
        const["mask"] = _rand(g, b, h, w) < o["masked"]
    elif kind == "disp":
        shape = (o["b"],) + tuple(o["hw"])
        const["target"] = 2.0 + 38.0 * _rand(g, *shape)
        const["mask"] = _rand(g, *shape) < o["masked"]
        for i in range(o["preds"]):
            diff[f"pred{i}"] = (const["target"] + 1.5 * _randn(g, *shape)).unsqueeze(1)
    elif kind == "focal":
        shape = (o["rows"], o["cols"])
        diff["logits"] = 2.0 * _randn(g, *shape)      # sigmoid within about [0.02, 0.98] but for a few tails
        t = _rand(g, *shape) < o["pos"]
        const["targets"] = {"int32": t.to(torch.int32), "int64": t.to(torch.int64), "bool": t, "float": t.to(torch.float64)}[o["target"]]
        if o.get("weights"):
            const["weights"] = 0.5 + _rand(g, *shape)
    elif kind == "sl1rows":
        diff["input"] = _randn(g, o["rows"], o["cols"])
        const["target"] = diff["input"] + 0.3 * _randn(g, o["rows"], o["cols"])
        const["weight"] = 0.1 + _rand(g, o["rows"])
    elif kind == "depthreg":
        b, d, (h, w) = o["b"], o["d"], o["hw"]
        diff["cost"] = 3.0 * _randn(g, b, d, h, w)
        const["levels"] = torch.linspace(2.0, 59.0, d, dtype=torch.float64)
        gt = 2.0 + 56.0 * _rand(g, b, h, w)
        u = _rand(g, b, h, w)
        const["gt"] = torch.where(u < o["invalid"] / 2, -1.0, torch.where(u < o["invalid"], 60.0 + 20.0 * u, gt)).to(torch.float64)
    elif kind == "coord":
        diff["pred"] = _randn(g, o["n"], 9, 2)
        const["corners"] = 2.0 * _randn(g, o["n"], 9, 3)
    elif kind == "shape":
        diff["pred"] = _randn(g, o["n"], 16)
        const["gt"] = 1e4 * _randn(g, o["n"], 16)
    elif kind == "bbox":
        diff["pred"] = _randn(g, o["n"], 5)
        const["gt"] = _randn(g, o["n"], 5)
    else:
        raise KeyError(kind)

    def cast(t):                  # every value is a float32 number, so that the float32 and float64 runs see the same inputs
        return t.to(device) if t.dtype in (torch.bool, torch.int32, torch.int64) else t.float().to(device=device, dtype=dtype)
    return {"diff": {k: cast(v).requires_grad_(True) for k, v in diff.items()}, "const": {k: cast(v) for k, v in const.items()}}


def call(mod, name, x, depth_regression=None):
    """The case's loss through ``mod`` (this package's loss3d or the reference's): its public classes and functions, called
    the way a training script calls them.  ``depth_regression`` stands in for ``mod.depth_regression_loss`` where ``mod`` has
    none (the reference)."""
    kind, o = CASES[name]
    d, c = x["diff"], x["const"]
    if kind == "mse":
        return mod.VoxelMSELoss(use_target_weight="tw" in o)({"ncf": d["pred"]}, c["gt"], c.get("tw"))
    if kind == "msew":
        return mod.VoxelMSELossWeighted(use_target_weight="tw" in o)({"ncf": d["pred"]}, c["gt"], c.get("tw"))
    if kind == "occ":
        return mod.OccupancyLoss(gamma=o.get("gamma", 2.), alpha=o.get("alpha", 0.25))({"occupancy": d["pred"]}, c["gt"])
    if kind == "offset":
        return mod.OffsetLoss()({"offset": d["pred"]}, {"offset": c["gt"], "occupancy": c["occ"]})
    if kind == "depth":
        return mod.DepthLoss()({"depth": d["pred"]}, {"gt_depth": c["gt"]})
    if kind == "wloss":
        return mod.W_loss(d["prob"], c["target"], d["off"], c["mask"], c["levels"], reduction=o["reduction"], p=1)
    if kind == "disp":
        return mod.calc_disp_loss({"depth_preds": [d[f"pred{i}"] for i in range(o["preds"])]}, c["mask"], c["target"], "sl1")
    if kind == "disp_w1":
        return mod.calc_disp_loss({"prob": d["prob"], "offset": d["off"], "depth_levels": c["levels"]}, c["mask"], c["target"], "W1")
    if kind == "focal":
        return mod.sigmoid_focal_loss_multi_target(d["logits"], c["targets"], c.get("weights"))
    if kind == "sl1rows":
        return mod.smooth_l1_loss(d["input"], c["target"], c["weight"], beta=o["beta"])
    if kind == "depthreg":
        return (depth_regression or mod.depth_regression_loss)(d["cost"], c["levels"], c["gt"])
    if kind == "coord":
        return mod.CoordinateLoss(COORD_CFG, normalize_gt=o["normalize"])({"coordinates": d["pred"]}, {"gt_corners_local": c["corners"]})
    if kind == "shape":
        return mod.ShapeLoss()({"shape": d["pred"]}, {"shape": c["gt"]})
    if kind == "bbox":
        return mod.BboxLoss(COORD_CFG)({"bbox": d["pred"]}, {"gt_box_local": c["gt"]})["l1"]
    raise KeyError(kind)


# ------------------------------------------------------------------------------ the restatement
def _mean_over(values, counted):
    """sum(values where counted) / count, 0 where nothing is counted (a zero that still depends on ``values``)."""
    counted = counted.to(values.dtype)
    total, count = (values * counted).sum(), counted.sum()
    return total / count if float(count) > 0 else total * 0.0


def _focal(p, t, gamma, alpha):
    pos = -alpha * (1 - p) ** gamma * torch.log(p + 1e-7)
    neg = -(1 - alpha) * p ** gamma * torch.log((1 - p) + 1e-7)
    return (t == 1).to(p.dtype) * pos + (t == 0).to(p.dtype) * neg


def _huber(diff, beta):
    n = diff.abs()
    return torch.where(n < beta, n * n / (2 * beta), n - beta / 2)


def restate(name, x):
    """The case's loss from its formula, in the dtype of ``x`` (float64 in the tests)."""
    kind, o = CASES[name]
    d, c = x["diff"], x["const"]
    if kind in ("mse", "msew"):
        p, g = d["pred"], c["gt"]
        n, k = p.shape[:2]
        p, g = p.reshape(n, k, -1), g.reshape(n, k, -1)
        if "tw" in o:
            w = c["tw"].reshape(k, -1, 1).expand(k, n, 1).transpose(0, 1)           # [n, k, 1]
            return (0.5 if kind == "msew" else 1.0) * ((w * (p - g)) ** 2).mean()
        if kind == "mse":
            return ((p - g) ** 2).mean()
        sq = (p - g) ** 2
        pos, rest = (g > 0).to(p.dtype), (g <= 0).to(p.dtype)
        per_part = 0.5 * ((sq * pos).sum((0, 2)) / pos.sum((0, 2)) + (sq * rest).sum((0, 2)) / rest.sum((0, 2)))
        return per_part.mean()
    if kind == "occ":
        return _mean_over(_focal(d["pred"], c["gt"], o.get("gamma", 2.), o.get("alpha", 0.25)), c["gt"] != -1)
    if kind == "offset":
        p = d["pred"]
        n = p.size(0)
        diff = (p.reshape(n, 3, o["parts"], *o["vol"]) - c["gt"]).abs()
        counted = (c["occ"] == 1)[:, None, None].expand_as(diff)
        return _mean_over(diff, counted)
    if kind == "depth":
        return _mean_over(_huber(d["pred"] - c["gt"], 1.0), (c["gt"] != -1) & (c["gt"] < 60.))
    if kind in ("wloss", "disp_w1"):
        dist = (c["levels"].reshape(1, -1, 1, 1) + d["off"] - c["target"].unsqueeze(1)).abs()
        per_pixel = (d["prob"] * dist).sum(1)
        if o.get("reduction") == "none":
            return per_pixel[c["mask"]]
        m = c["mask"].to(per_pixel.dtype)
        return (per_pixel * m).sum() / m.sum()
    if kind == "disp":
        m = c["mask"].to(c["target"].dtype)
        weights = (0.5, 0.7, 1.0)[3 - o["preds"]:]
        return sum(w * (_huber(d[f"pred{i}"].squeeze(1) - c["target"], 1.0) * m).sum() / m.sum() for i, w in enumerate(weights))
    if kind == "focal":
        t = c["targets"].to(d["logits"].dtype)
        l = _focal(torch.sigmoid(d["logits"]), t, 2., 0.25)
        return (l * c["weights"]).sum() if "weights" in c else l.sum()
    if kind == "sl1rows":
        w = c["weight"]
        return (_huber(d["input"] - c["target"], o["beta"]).mean(1) * w).sum() / w.sum()
    if kind == "depthreg":
        depth = (torch.softmax(d["cost"], 1) * c["levels"].reshape(1, -1, 1, 1)).sum(1)
        return _mean_over(_huber(depth - c["gt"], 1.0), (c["gt"] != -1) & (c["gt"] < 60.))
    if kind == "coord":
        gt = c["corners"][:, :, [0, 2]]
        if o["normalize"]:
            lo = gt.new_tensor([COORD_CFG.x_range[0], COORD_CFG.z_range[0]])
            span = gt.new_tensor([COORD_CFG.x_range[1] - COORD_CFG.x_range[0], COORD_CFG.z_range[1] - COORD_CFG.z_range[0]])
            gt = (gt - lo) / span
        return (d["pred"] - gt).abs().mean()
    if kind == "shape":
        return (d["pred"] - c["gt"] / 1e4).abs().mean()
    if kind == "bbox":
        return (d["pred"] - c["gt"]).abs().mean()
    raise KeyError(kind)


def loss_and_grads(fn, x):
    """(loss, {name: gradient}) of ``fn(x)``; a vector loss ('none') is differentiated through its sum.  A loss that does not
    depend on the inputs (the reference's Python ``0.`` for an empty mask) has zero gradients."""
    for t in x["diff"].values():
        t.grad = None
    out = fn(x)
    if not torch.is_tensor(out):
        out = torch.zeros((), dtype=next(iter(x["diff"].values())).dtype)
    if out.requires_grad:
        out.sum().backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)).detach() for k, t in x["diff"].items()}
    return out.detach(), grads
