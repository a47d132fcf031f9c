"""A kernel's grant of dynamic LDS above 48 KB must grow with the calls: ``snvc_warped_expand_backward`` sizes its LDS by the row
width, so a process whose first large call needs 49 KB and whose next needs 66 KB has to raise the kernel's attribute twice (the
launch helper once remembered only THAT it had been raised).  Each order runs in a fresh process: the grant is per process.

The oracle check is test_warped_expand_backward_vs_oracle's, at its 1e-5, with the C oracle run in float64: its float32 form rounds
the sampling position x = w - shift to float32 before it takes the interpolation weight from it, which at w near 768 / 1024 (half an ulp
of x: 3e-5) is an error of the REFERENCE of 1.1e-5 (W = 768) and 3.0e-5 (W = 1024) of the largest value -- measured: float32 oracle
against float64 oracle 1.10e-5 / 2.97e-5, kernel against float32 oracle 1.10e-5 / 2.97e-5, kernel against float64 oracle 7.2e-8 /
6.1e-8.  (The kernel takes the weight from the shift itself.  At the 40- and 72-wide rows of the existing test the same rounding is
below 2e-6.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import check

pytestmark = pytest.mark.gpu

HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers")
sys.path.insert(0, HELPERS)
import lds_grant_child as child  # noqa: E402


def run_child(order, tmp_path):
    out = str(tmp_path / f"{order}.npz")
    p = subprocess.run([sys.executable, os.path.join(HELPERS, "lds_grant_child.py"), order, out], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, f"child ({order}) failed with status {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


def test_warped_expand_backward_lds_grant_grows_in_either_order(tmp_path):
    from oracle import native as O
    up, down = run_child("up", tmp_path), run_child("down", tmp_path)
    assert sorted(up) == sorted(down) == ["a1024", "a768", "dpl1024", "dpl768"]
    for k in up:
        assert np.array_equal(up[k], down[k]), f"{k} differs between the two orders"
    for W in child.WIDTHS:         # the oracle check of test_warped_expand_backward_vs_oracle
        dy, s = child.inputs(W)
        N, C, D, H = 1, 1, 3, 2
        a = up[f"a{W}"]
        for kd in range(3):
            for kw in range(3):
                g = np.zeros((N, 2 * C, D, H, W), np.float32)
                for e in range(D):
                    d = e - kd + 1
                    if 0 <= d < D:
                        lo, hi = max(0, kw - 1), min(W, W + kw - 1)
                        g[:, C:, e, :, lo:hi] = dy[:, :, d, :, lo - kw + 1:hi - kw + 1]
                _, exp = O.cost_volume_backward(g.astype(np.float64), s.astype(np.float64), 1)
                check(a[:, kd, kw], exp, 1e-5, f"a[{kd}][{kw}] (W = {W})")
        exp = np.stack([dy[:, :, 0], dy[:, :, 1:-1].sum(2), dy[:, :, -1]], axis=2)
        check(up[f"dpl{W}"], exp, 1e-5, f"depth-class sums (W = {W})")
