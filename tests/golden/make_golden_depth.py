"""Writes tests/golden/depth_ref.npz: the depth read-out's torch composition on the small cases of tests/depth_cases.py, and
the reference's own project_image_to_rect (snvc/utils/torch_utils.py:5-19) on its point cases.

    python tests/golden/make_golden_depth.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Needs the reference checkout (it imports on the CPU); the tests need only the file.  Inputs come from the cases' seeds, so
the file holds results only:

    depth64/<case>, conf64/<case>   F.interpolate(trilinear) -> softmax over depth -> expectation over the levels, and the
                                    largest probability, in float64
    grad64/<case>                   d cost by float64 autograd of sum(depth * gy), for the gradient cases
    e32/<case>                      [depth, conf, grad]: the largest error of the same composition run in float32 against the
                                    float64 result, relative to the quantity's largest magnitude (grad: 0 where not recorded):
                                    the composition's own float32 error, the yardstick the HIP error is held to
    loss64, lossgrad64, loss_e32    DepthLoss (smooth-L1 mean over the pixels whose target is neither -1 nor 60 m or beyond)
                                    over the read-out of case LOSS_CASE, its gradient with respect to cost, and [loss, grad]
                                    float32 errors as above
    points/<case>                   float32 [N, H, W, 3]: project_image_to_rect of every pixel for float32 inputs
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")
sys.path.insert(0, REF)

from snvc.utils.torch_utils import project_image_to_rect  # noqa: E402

import depth_cases as DC  # noqa: E402


def compose(cost, levels, c):
    up = F.interpolate(cost[:, None], size=c.out, mode="trilinear", align_corners=c.align)[:, 0]
    p = F.softmax(up, 1)
    return (p * levels.reshape(1, -1, 1, 1)).sum(1), p.max(1).values


def depth_loss(depth, gt):
    mask = (gt != -1) & (gt < 60.)
    return F.smooth_l1_loss(depth[mask], gt[mask], reduction="mean")


def run(c, dtype):
    cost, gy = (torch.from_numpy(v).to(dtype) for v in DC.inputs(c))
    levels = torch.from_numpy(DC.levels(c)).to(dtype)
    cost.requires_grad_(True)
    depth, conf = compose(cost, levels, c)
    grad = torch.autograd.grad((depth * gy).sum(), cost)[0] if c.grad else None
    return depth.detach(), conf.detach(), grad


def run_loss(c, dtype):
    cost = torch.from_numpy(DC.inputs(c)[0]).to(dtype).requires_grad_(True)
    levels, gt = torch.from_numpy(DC.levels(c)).to(dtype), torch.from_numpy(DC.loss_target(c)).to(dtype)
    loss = depth_loss(compose(cost, levels, c)[0], gt)
    return loss.detach(), torch.autograd.grad(loss, cost)[0]


def rel(a32, a64):
    top = float(a64.abs().max())
    return float((a32.double() - a64).abs().max()) / top if top > 0 else 0.0


def main():
    out = {}
    for c in DC.CASES:
        d64, c64, g64 = run(c, torch.float64)
        d32, c32, g32 = run(c, torch.float32)
        out[f"depth64/{c.name}"], out[f"conf64/{c.name}"] = d64.numpy(), c64.numpy()
        if c.grad:
            out[f"grad64/{c.name}"] = g64.numpy()
        e = np.array([rel(d32, d64), rel(c32, c64), rel(g32, g64) if c.grad else 0.0])
        out[f"e32/{c.name}"] = e
        print(f"{c.name:9s} depth {float(d64.min()):.4f} .. {float(d64.max()):.4f}  e32 depth {e[0]:.2e} conf {e[1]:.2e} grad {e[2]:.2e}"
              f"  (depth abs {e[0] * float(d64.abs().max()):.2e})")
    c = DC.BY_NAME[DC.LOSS_CASE]
    (l64, lg64), (l32, lg32) = run_loss(c, torch.float64), run_loss(c, torch.float32)
    out["loss64"], out["lossgrad64"] = l64.numpy(), lg64.numpy()
    out["loss_e32"] = np.array([abs(float(l32) - float(l64)) / abs(float(l64)), rel(lg32, lg64)])
    print(f"loss {float(l64):.9g}  e32 loss {out['loss_e32'][0]:.2e} grad {out['loss_e32'][1]:.2e}")
    for c in DC.POINT_CASES:
        depth, P, _ = DC.point_inputs(c)
        u, v = DC.pixel_grid(c)
        n, h, w = c.shape
        pts = np.empty((n, h, w, 3), dtype=np.float32)
        for k in range(n):
            uv_depth = torch.stack([torch.from_numpy(u)[None, :].expand(h, w).reshape(-1), torch.from_numpy(v)[:, None].expand(h, w).reshape(-1),
                                    torch.from_numpy(depth[k]).reshape(-1)])
            assert uv_depth.dtype == torch.float32
            res = project_image_to_rect(uv_depth, torch.from_numpy(P[k] if c.per_sample else P))
            assert res.dtype == torch.float32
            pts[k] = res.t().reshape(h, w, 3).numpy()
        out[f"points/{c.name}"] = pts
    path = os.path.join(ROOT, "tests", "golden", "depth_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
