"""Two calls of ``ops.warped_expand_backward`` in a fresh process (started by tests/test_gpu_lds_grant.py), whose dynamic LDS needs
differ: W = 768 takes 49 456 bytes, just over the 48 KB a kernel gets unasked, W = 1024 takes 65 840, more than the first call
was granted.  argv: the order ("up": 768 then 1024, "down": 1024 then 768) and the .npz file the results go to."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WIDTHS = (768, 1024)


def inputs(W):
    """dy [1,1,3,2,W] and shifts [1,3]: fractional, a zero and a repeated one."""
    r = np.random.default_rng(171 + W)
    dy = r.standard_normal((1, 1, 3, 2, W)).astype(np.float32)
    s = r.uniform(0, 14, (1, 3))
    s[0, 2] = 0.0
    s[0, 1] = np.floor(s[0, 0]) + 0.25
    return dy, s.astype(np.float32)


def main(order, out_path):
    import torch

    from snvc_amd import ops
    dev = torch.device("cuda:0")
    out = {}
    for W in (WIDTHS if order == "up" else WIDTHS[::-1]):
        dy, s = inputs(W)
        a, dpl = ops.warped_expand_backward(torch.from_numpy(dy).to(dev), torch.from_numpy(s).to(dev))
        torch.cuda.synchronize()
        out[f"a{W}"], out[f"dpl{W}"] = a.cpu().numpy(), dpl.cpu().numpy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
