"""Writes tests/golden/loss3d_ref.npz: what the reference's own snvc/models/loss3d.py computes on the small cases of
tests/loss_cases.py.

    python tests/golden/make_golden_loss.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Needs the reference checkout (it imports on the CPU); the tests need only the file.  Inputs come from the cases' seeds, so
the file holds results only:

    loss64/<case>            the loss in float64 (a vector for reduction='none')
    grad64/<case>/<input>    its gradient in float64, from autograd through the reference's own code
    loss32/<case>            the loss of the reference's float32 run
    e32/<case>               [relative error of loss32, max |grad32 - grad64| / max |grad64| over the inputs]: the
                             reference's own float32-against-float64 error, the yardstick the HIP error is printed beside

For depth_regression_loss, which the reference does not have as one function, the reference's pieces are composed:
F.softmax over D, disparityregression.forward (called unbound: the constructor calls .cuda()) and DepthLoss.
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

import snvc.models.loss3d as ref_loss  # noqa: E402
from snvc.models.submodule import disparityregression  # noqa: E402

import loss_cases as LC  # noqa: E402


def ref_depth_regression(cost, levels, gt):
    depth = disparityregression.forward(None, F.softmax(cost, 1), levels)
    return ref_loss.DepthLoss()({"depth": depth}, {"gt_depth": gt})


def run(name, dtype):
    x = LC.inputs(name, dtype)
    return LC.loss_and_grads(lambda v: LC.call(ref_loss, name, v, depth_regression=ref_depth_regression), x)


def main():
    out = {}
    for name in LC.SMALL:
        l64, g64 = run(name, torch.float64)
        l32, g32 = run(name, torch.float32)
        out[f"loss64/{name}"] = l64.numpy()
        out[f"loss32/{name}"] = l32.numpy()
        for k, g in g64.items():
            out[f"grad64/{name}/{k}"] = g.numpy()
        scale = float(l64.abs().max()) if l64.numel() else 0.0
        e_loss = float((l32.double() - l64).abs().max()) / scale if scale > 0 else 0.0
        e_grad = 0.0
        for k, g in g64.items():
            top = float(g.abs().max())
            if top > 0:
                e_grad = max(e_grad, float((g32[k].double() - g).abs().max()) / top)
        out[f"e32/{name}"] = np.array([e_loss, e_grad])
        print(f"{name:16s} loss {float(l64.sum()):.12g}  e32 loss {e_loss:.2e} grad {e_grad:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "loss3d_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
