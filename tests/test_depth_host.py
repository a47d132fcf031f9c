"""CPU checks of the depth read-out's host side: the binding against include/snvc_depth.h, the argument checks of every entry
point (made before any device work), the float64 restatement of the coordinate rule (tests/depth_ref.py) against float64
F.interpolate on the case table, the golden file's contents, and that CPU inputs raise.
"""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_cases as DC
import depth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_depth.h")
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "depth_ref.npz"))


def test_header_and_binding_agree():
    """The mirrored constants; names, parameters and the ABI number are held by tests/test_abi_tables_host.py."""
    from snvc_amd import _depth
    text = open(HEADER).read()
    assert int(re.search(r"SNVC_DEPTH_MAX_PLANES = (\d+)", text).group(1)) == _depth.MAX_PLANES >= 512
    assert int(re.search(r"SNVC_DEPTH_POINTS_BLOCK = (\d+)", text).group(1)) == _depth.POINTS_BLOCK


def test_the_c_calls_check_their_arguments_before_any_launch():
    from snvc_amd import _depth
    from snvc_amd._lib import lib
    L = _depth.lib()
    err = lambda: lib().snvc_last_error_string()      # noqa: E731
    one = 16        # a non-null, aligned stand-in: every check below comes before any pointer is read
    big = _depth.MAX_PLANES + 1
    # forward
    assert L.snvc_depth_readout_forward(None, None, None, None, None, None, 0, 12, 5, 7, 12, 20, 28, 0, None) == 0       # N = 0
    assert L.snvc_depth_readout_forward(None, None, None, None, None, None, 2, 12, 5, 7, 12, 0, 28, 0, None) == 0        # no pixels
    assert L.snvc_depth_readout_forward(None, None, None, None, None, None, 2, 12, 5, 7, 12, 20, 28, 0, None) == 1 and b"null pointer" in err()
    assert L.snvc_depth_readout_forward(one, one, one, None, None, None, 2, 12, 5, 7, big, 20, 28, 0, None) == 2 and b"at most 2048" in err()
    assert L.snvc_depth_readout_forward(one, one, one, None, None, None, 2, big, 5, 7, 12, 20, 28, 0, None) == 2
    assert L.snvc_depth_readout_forward(one, one, one, None, None, None, 2, 12, 5, 7, 12, 4, 28, 0, None) == 2 and b"up-sampling" in err()
    assert L.snvc_depth_readout_forward(one, one, one, None, None, None, 2, 12, 5, 7, 12, -1, 28, 0, None) == 1 and b"negative" in err()
    assert L.snvc_depth_readout_forward(one, one, one, None, None, None, 2, 0, 5, 7, 12, 20, 28, 0, None) == 1
    assert L.snvc_depth_readout_forward(one, one, one, None, None, None, 2, 12, 5, 7, 0, 20, 28, 0, None) == 1
    assert L.snvc_depth_readout_forward(one, one, one + 2, None, None, None, 2, 12, 5, 7, 12, 20, 28, 0, None) == 1 and b"aligned" in err()
    # backward
    assert L.snvc_depth_readout_backward(*([None] * 7), 0, 12, 5, 7, 12, 20, 28, 0, None) == 0
    assert L.snvc_depth_readout_backward(*([None] * 7), 2, 12, 5, 7, 12, 20, 28, 0, None) == 1 and b"null pointer" in err()
    assert L.snvc_depth_readout_backward(*([one] * 6), None, 2, 12, 5, 7, 12, 20, 28, 0, None) == 1
    assert L.snvc_depth_readout_backward(*([one] * 7), 2, 12, 5, 7, big, 20, 28, 0, None) == 2
    assert L.snvc_depth_readout_backward(*([one] * 7), 2, 12, 5, 7, 12, 20, 6, 0, None) == 2
    assert L.snvc_depth_readout_backward(*([one] * 7), 2, 12, -5, 7, 12, 20, 28, 0, None) == 1
    # points
    f = [0.0, 0.0, 1e9, 0.0, 0.0, 1.0, 1.0]
    assert L.snvc_depth_to_points(None, None, 0, None, *f, None, None, 0, 7, 9, None) == 0
    assert L.snvc_depth_to_points(None, None, 0, None, *f, None, None, 2, 7, 9, None) == 1 and b"null pointer" in err()
    assert L.snvc_depth_to_points(one, one, 0, None, *f, one, None, 2, 7, 9, None) == 1
    assert L.snvc_depth_to_points(one, one, 0, None, *f, one, one, 2, -7, 9, None) == 1
    assert L.snvc_depth_to_points(one, one, 0, None, *f, one, one, 2, 1 << 16, 1 << 16, None) == 2
    assert L.snvc_depth_points_workspace_bytes(2, 63) == 8 and L.snvc_depth_points_workspace_bytes(2, 5200) == 2 * 21 * 4
    assert L.snvc_depth_points_workspace_bytes(0, 63) == 0 and L.snvc_depth_points_workspace_bytes(-1, 63) < 0
    assert L.snvc_depth_points_workspace_bytes(1, 1 << 31) < 0
    assert L.snvc_depth_to_points_compact(None, None, 0, None, *f, None, None, None, 0, 7, 9, None) == 0
    assert L.snvc_depth_to_points_compact(None, None, 0, None, *f, None, None, None, 2, 7, 9, None) == 1 and b"null pointer" in err()
    assert L.snvc_depth_to_points_compact(one, one, 0, None, *f, None, one, one, 2, 7, 9, None) == 1         # no workspace
    assert L.snvc_depth_to_points_compact(one, one, 0, None, *f, one, one, one, 2, 7, -9, None) == 1


@pytest.mark.parametrize("c", DC.CASES, ids=[c.name for c in DC.CASES])
def test_restatement_equals_float64_interpolate(c):
    cost, _ = DC.inputs(c)
    want = F.interpolate(torch.from_numpy(cost).double()[:, None], size=c.out, mode="trilinear", align_corners=c.align)[:, 0].numpy()
    got = R.upsample(cost, c.out, c.align)
    assert got.shape == want.shape == (c.cost[0],) + c.out
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    depth, conf = R.readout(cost, DC.levels(c), c.out, c.align)
    # the golden file is torch's float64 run of the same definition
    assert np.abs(depth - GOLD[f"depth64/{c.name}"]).max() <= 1e-9 * DC.Z_FAR
    if c.name != "g":       # with logits of 1e4 a near-tie moves the largest probability by far more than a rounding
        assert np.abs(conf - GOLD[f"conf64/{c.name}"]).max() <= 1e-9


def test_coordinate_rule_at_the_edges():
    i0, i1, t = R.axis(5, 20, False)
    assert i0[0] == 0 and t[0] == 0.0 and i0[-1] == 4 and i1[-1] == 4         # clamped at both ends
    assert (i0[2], i1[2], t[2]) == (0, 1, 0.125)
    i0, i1, t = R.axis(5, 19, True)
    assert (i0[-1], i1[-1]) == (4, 4) and abs(t[-1]) < 1e-12 and i0[0] == 0
    i0, i1, t = R.axis(1, 4, False)
    assert not i0.any() and not i1.any()
    assert R.axis(7, 1, True)[0].tolist() == [0]


def test_golden_file_holds_every_case():
    for c in DC.CASES:
        n, (_, ho, wo) = c.cost[0], c.out
        assert GOLD[f"depth64/{c.name}"].shape == GOLD[f"conf64/{c.name}"].shape == (n, ho, wo)
        assert GOLD[f"depth64/{c.name}"].dtype == np.float64 and GOLD[f"e32/{c.name}"].shape == (3,)
        assert (f"grad64/{c.name}" in GOLD.files) == c.grad
        if c.grad:
            assert GOLD[f"grad64/{c.name}"].shape == c.cost and GOLD[f"e32/{c.name}"][2] > 0
        assert 0 < GOLD[f"e32/{c.name}"][0] < 1e-5
    assert GOLD["lossgrad64"].shape == DC.BY_NAME[DC.LOSS_CASE].cost and GOLD["loss_e32"].shape == (2,)
    for c in DC.POINT_CASES:
        assert GOLD[f"points/{c.name}"].shape == c.shape + (3,) and GOLD[f"points/{c.name}"].dtype == np.float32
    # the table itself: what the issue lists
    assert [c.name for c in DC.CASES] == ["a", "b", "c", "d", "e_h1", "e_w1", "f_shrink", "f_wide", "g", "h"]
    assert DC.BY_NAME["d"].out[0] == 320 and DC.BY_NAME["c"].out == (192, 24, 36) and not DC.BY_NAME["f_shrink"].hip


def test_golden_points_follow_the_stated_order_of_operations():
    for c in DC.POINT_CASES:
        depth, P, _ = DC.point_inputs(c)
        u, v = DC.pixel_grid(c)
        for k in range(c.shape[0]):
            p = P[k] if c.per_sample else P
            z = depth[k]
            with np.errstate(invalid="ignore"):
                x = ((u[None, :] - p[0, 2]) * z) / p[0, 0] + p[0, 3] / (-p[0, 0])
                y = ((v[:, None] - p[1, 2]) * z) / p[1, 1] + p[1, 3] / (-p[1, 1])
            assert x.dtype == np.float32
            ok = np.isfinite(z)
            got = GOLD[f"points/{c.name}"][k]
            assert np.array_equal(got[..., 0][ok], x[ok]) and np.array_equal(got[..., 1][ok], y[ok]) and np.array_equal(got[..., 2][ok], z[ok])


def test_cpu_inputs_raise():
    from snvc_amd import depth
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        depth.depth_readout(torch.zeros(1, 4, 3, 3), torch.ones(4))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        depth.DepthReadout(torch.ones(4))(torch.zeros(1, 4, 3, 3), size=(6, 6))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        depth.depth_to_points(torch.zeros(1, 3, 3), torch.eye(3, 4))
    m = depth.DepthReadout(np.linspace(2.0, 59.6, 8))
    assert m.levels.dtype == torch.float32 and "levels" not in m.state_dict()
