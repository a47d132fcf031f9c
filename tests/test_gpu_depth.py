"""The depth read-out and the pseudo-LiDAR projection on the GPU (snvc_amd.depth, csrc/depth_head.hip) against
tests/golden/depth_ref.npz (written by tests/golden/make_golden_depth.py) on the cases of tests/depth_cases.py.

Tolerance.  The kernel and the torch composition's own float32 run differ from float64 by the order of the interpolation's
and the softmax's sums; the kernel also rescales its running sums when the maximum moves (the online softmax).  The bound of
a quantity (depth, confidence, gradient) is FACTOR = 8 (4 for summation and interpolation order, times 2 for the online
rescaling) times the largest error of the composition's float32 run for that quantity over the compared cases of the table
(`e32` in the golden file), relative to the quantity's own maximum.  Case g (logits of 1e4) is held to finiteness only and is
left out of the maximum: its float32 error is larger and would only widen the bound.  The yardstick comes from the
composition, never from the kernel.  Each test prints its error beside the bound.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import depth_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "depth_ref.npz"))
FACTOR = 8.0
BOUND = dict(zip(DC.QUANTITIES, FACTOR * np.max([GOLD[f"e32/{c.name}"] for c in DC.COMPARED], axis=0)))


def dev():
    return torch.device("cuda:0")


def routes():
    from snvc_amd.models import submodule as S
    return S._ROUTES["depth_readout_hip"], S._ROUTES["depth_readout_torch"]


def within(what, got, want, bound):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else got
    err = float(np.abs(got.astype(np.float64) - want).max() / np.abs(want).max())
    print(f"{what}: error {err:.3g}, bound {bound:.3g}")
    assert got.shape == want.shape and got.dtype == np.float32 and err <= bound, f"{what}: {err:.3g} > {bound:.3g}"


def tensors(c, grad=False):
    cost, gy = (torch.from_numpy(v).to(dev()) for v in DC.inputs(c))
    return cost.requires_grad_(grad), torch.from_numpy(DC.levels(c)).to(dev()), gy


# ---------------------------------------------------------------------------------------------------- the read-out
@pytest.mark.parametrize("c", DC.COMPARED, ids=[c.name for c in DC.COMPARED])
def test_forward_and_confidence_against_float64(c):
    from snvc_amd import depth as D
    cost, levels, _ = tensors(c)
    h0, t0 = routes()
    got, conf = D.depth_readout(cost, levels, size=c.out[1:], align_corners=c.align, confidence=True)
    assert routes() == ((h0 + 1, t0) if c.hip else (h0, t0 + 1))
    within(f"depth {c.name}", got, GOLD[f"depth64/{c.name}"], BOUND["depth"])
    within(f"confidence {c.name}", conf, GOLD[f"conf64/{c.name}"], BOUND["conf"])
    alone = D.depth_readout(cost, levels, size=c.out[1:], align_corners=c.align)
    assert torch.is_tensor(alone) and torch.equal(alone, got) and not conf.requires_grad


GRAD_CASES = [c for c in DC.CASES if c.grad]


@pytest.mark.parametrize("c", GRAD_CASES, ids=[c.name for c in GRAD_CASES])
def test_backward_against_float64_autograd(c):
    from snvc_amd import depth as D
    cost, levels, gy = tensors(c, grad=True)
    h0, t0 = routes()
    got, conf = D.depth_readout(cost, levels, size=c.out[1:], align_corners=c.align, confidence=True)
    assert routes() == (h0 + 1, t0) and got.requires_grad and not conf.requires_grad
    (got * gy).sum().backward()
    within(f"depth {c.name} (autograd forward)", got, GOLD[f"depth64/{c.name}"], BOUND["depth"])
    within(f"confidence {c.name} (autograd forward)", conf, GOLD[f"conf64/{c.name}"], BOUND["conf"])
    within(f"d cost {c.name}", cost.grad, GOLD[f"grad64/{c.name}"], BOUND["grad"])


def test_backward_is_bit_identical_over_two_runs():
    from snvc_amd import depth as D
    c = DC.BY_NAME["c"]
    grads = []
    for _ in range(2):
        cost, levels, gy = tensors(c, grad=True)
        D.depth_readout(cost, levels, size=c.out[1:]).backward(gy)
        grads.append(cost.grad.clone())
    assert torch.equal(grads[0], grads[1])


def test_huge_logits_give_finite_results():
    from snvc_amd import depth as D
    c = DC.BY_NAME["g"]
    cost, levels, gy = tensors(c, grad=True)
    got, conf = D.depth_readout(cost, levels, size=c.out[1:], confidence=True)
    got.backward(gy)
    assert torch.isfinite(got).all() and torch.isfinite(conf).all() and torch.isfinite(cost.grad).all()
    assert float(conf.min()) > 0.0 and float(conf.max()) <= 1.0
    assert float(got.detach().min()) >= DC.Z_NEAR * (1 - 1e-6) and float(got.detach().max()) <= DC.Z_FAR * (1 + 1e-6)


def test_size_none_equals_disparity_regression_of_the_softmax():
    from snvc_amd import depth as D
    from snvc_amd import ops
    c = DC.BY_NAME["h"]
    cost, levels, _ = tensors(c)
    h0, t0 = routes()
    got = D.DepthReadout(DC.levels(c)).to(dev())(cost)
    assert routes() == (h0 + 1, t0) and got.shape == (c.cost[0],) + c.cost[2:]
    want = ops.disparity_regression(F.softmax(cost, 1), levels)
    within("size=None against the golden file", got, GOLD[f"depth64/{c.name}"], BOUND["depth"])
    within("size=None against disparity_regression(softmax)", got, want.double().cpu().numpy(), BOUND["depth"])


def test_empty_batch_returns_an_empty_tensor_without_a_launch():
    from snvc_amd import depth as D
    levels = torch.from_numpy(DC.levels(DC.BY_NAME["a"])).to(dev())
    before = routes()
    got, conf = D.depth_readout(torch.zeros(0, 12, 5, 7, device=dev()), levels, size=(20, 28), confidence=True)
    assert got.shape == conf.shape == (0, 20, 28) and got.dtype == torch.float32 and routes() == before
    assert D.depth_readout(torch.zeros(2, 12, 0, 7, device=dev()), levels).shape == (2, 0, 7)
    cost = torch.zeros(0, 12, 5, 7, device=dev(), requires_grad=True)
    D.depth_readout(cost, levels, size=(20, 28)).sum().backward()
    assert cost.grad.shape == cost.shape


def test_a_transposed_view_gives_its_contiguous_copys_values():
    from snvc_amd import depth as D
    c = DC.BY_NAME["b"]
    cost, levels, gy = tensors(c)
    view = cost.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not view.is_contiguous() and torch.equal(view, cost)
    want = D.depth_readout(cost, levels, size=c.out[1:], align_corners=c.align)
    assert torch.equal(D.depth_readout(view, levels, size=c.out[1:], align_corners=c.align), want)
    a, b = cost.clone().requires_grad_(True), view.clone(memory_format=torch.preserve_format).requires_grad_(True)
    assert not b.is_contiguous()
    D.depth_readout(a, levels, size=c.out[1:], align_corners=c.align).backward(gy)
    D.depth_readout(b, levels, size=c.out[1:], align_corners=c.align).backward(gy)
    assert torch.equal(a.grad, b.grad)


def test_other_dtypes_take_the_torch_route():
    from snvc_amd import depth as D
    c = DC.BY_NAME["a"]
    cost, levels, _ = tensors(c)
    h0, t0 = routes()
    got = D.depth_readout(cost.double(), levels.double(), size=c.out[1:])
    assert routes() == (h0, t0 + 1) and got.dtype == torch.float64
    assert float((got.cpu() - torch.from_numpy(GOLD[f"depth64/{c.name}"])).abs().max()) < 1e-9 * DC.Z_FAR


def test_more_levels_than_the_kernel_takes_is_a_clean_error():
    from snvc_amd import _depth
    from snvc_amd import depth as D
    with pytest.raises(RuntimeError, match="at most 2048"):
        D.depth_readout(torch.zeros(1, 4, 2, 2, device=dev()), torch.ones(_depth.MAX_PLANES + 1, device=dev()), size=(4, 4))


def test_nothing_of_the_upsampled_volumes_size_is_allocated():
    """[1,16,16,32] -> (64,64,128): the up-sampled volume has 2 MiB.  Forward + backward may hold, above the inputs and the
    outputs, less than a quarter of that.  A condition that keeps a materialising implementation out, not a measurement."""
    from snvc_amd import depth as D
    r = np.random.default_rng(7)
    levels = torch.linspace(2.0, 59.6, 64, device=dev())
    gy = torch.from_numpy(r.standard_normal((1, 64, 128)).astype(np.float32)).to(dev())

    def step():
        cost = torch.from_numpy(r.standard_normal((1, 16, 16, 32)).astype(np.float32)).to(dev()).requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = D.depth_readout(cost, levels, size=(64, 128))
        out.backward(gy)
        torch.cuda.synchronize()
        results = out.numel() * 4 + cost.grad.numel() * 4
        return torch.cuda.max_memory_allocated() - base - results

    step()          # loads the library and whatever torch sets up on a first call
    extra = step()
    volume = 64 * 64 * 128 * 4
    print(f"peak above inputs and outputs: {extra} bytes; the up-sampled volume: {volume} bytes")
    assert extra < volume // 4


def test_depth_loss_trains_through_the_readout():
    """The gradient of DepthLoss reaches cost and matches the float64 composition.  The loss value: smooth-L1 has slope at
    most 1 and the loss is a mean, so the loss moves by at most the largest depth error, BOUND['depth'] times the largest depth."""
    from snvc_amd import depth as D
    from snvc_amd.models import loss3d
    c = DC.BY_NAME[DC.LOSS_CASE]
    cost, levels, _ = tensors(c, grad=True)
    gt = torch.from_numpy(DC.loss_target(c)).to(dev())
    loss = loss3d.DepthLoss()({"depth": D.depth_readout(cost, levels, gt.shape[-2:], align_corners=c.align)}, {"gt_depth": gt})
    loss.backward()
    err = abs(loss.item() - float(GOLD["loss64"]))
    print(f"loss {loss.item():.9g} against {float(GOLD['loss64']):.9g}: error {err:.3g}, bound {BOUND['depth'] * DC.Z_FAR:.3g}")
    assert err <= BOUND["depth"] * DC.Z_FAR
    assert cost.grad is not None and float(cost.grad.abs().max()) > 0
    within("d cost of DepthLoss", cost.grad, GOLD["lossgrad64"], FACTOR * float(GOLD["loss_e32"][1]))


# ---------------------------------------------------------------------------------------------------- points
def point_tensors(c):
    depth, P, conf = DC.point_inputs(c)
    return depth, P, conf, torch.from_numpy(depth).to(dev()), torch.from_numpy(P).to(dev()), torch.from_numpy(conf).to(dev())


def expected_valid(depth, conf, min_conf, z_range):
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(depth) & (depth >= np.float32(z_range[0])) & (depth < np.float32(z_range[1]))
        return ok & (conf >= np.float32(min_conf)) if conf is not None else ok


@pytest.mark.parametrize("c", DC.POINT_CASES, ids=[c.name for c in DC.POINT_CASES])
@pytest.mark.parametrize("filt", ["all", "z_range", "min_conf"])
def test_points_are_bit_equal_to_the_reference(c, filt):
    from snvc_amd import depth as D
    depth, P, conf, dt, Pt, ct = point_tensors(c)
    kw = {"all": {}, "z_range": {"z_range": (10.0, 40.5)}, "min_conf": {"conf": ct, "min_conf": 0.5}}[filt]
    pts, valid = D.depth_to_points(dt, Pt, origin=c.origin, stride=c.stride, **kw)
    want_valid = expected_valid(depth, conf if filt == "min_conf" else None, kw.get("min_conf", 0.0), kw.get("z_range", (0.0, np.inf)))
    share = want_valid.mean()
    assert (0.3 < share < 0.7) if filt != "all" else share > 0.95
    assert valid.dtype == torch.bool and np.array_equal(valid.cpu().numpy(), want_valid)
    want = np.where(want_valid[..., None], GOLD[f"points/{c.name}"], np.float32(0))
    got = pts.cpu().numpy()
    assert got.shape == want.shape and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def compaction_inputs(c, variant):
    depth, P, conf = DC.point_inputs(c)
    depth = depth.copy()
    if variant == "none_and_all":           # sample 0 has no valid pixel, the last sample only valid ones
        depth[0] = -1.0
        depth[-1] = np.where(np.isfinite(depth[-1]), depth[-1], np.float32(5.0))
    return depth, P, conf


@pytest.mark.parametrize("c", [DC.POINTS_BY_NAME["single"], DC.POINTS_BY_NAME["blocks"]], ids=["7x9", "40x130"])
@pytest.mark.parametrize("variant", ["half", "none_and_all"])
def test_compaction_keeps_the_pixel_order(c, variant):
    from snvc_amd import depth as D
    depth, P, conf = compaction_inputs(c, variant)
    dt, Pt, ct = (torch.from_numpy(v).to(dev()) for v in (depth, P, conf))
    kw = {"conf": ct, "min_conf": 0.5} if variant == "half" else {}
    full, valid = D.depth_to_points(dt, Pt, origin=c.origin, stride=c.stride, **kw)
    pts, counts = D.depth_to_points(dt, Pt, origin=c.origin, stride=c.stride, compact=True, **kw)
    n, h, w = c.shape
    assert pts.shape == (n, h * w, 3) and counts.shape == (n,) and counts.dtype == torch.int32 and pts.is_cuda and counts.is_cuda
    full, valid, pts, counts = full.cpu().numpy(), valid.cpu().numpy(), pts.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(counts, valid.reshape(n, -1).sum(1))
    if variant == "none_and_all":
        assert counts[0] == 0 and counts[-1] == h * w
    for k in range(n):
        want = full[k][valid[k]]                          # row-major pixel order
        assert np.array_equal(pts[k, :counts[k]].view(np.uint32), want.view(np.uint32))
        assert not pts[k, counts[k]:].any()


def test_nothing_waits_for_the_device():
    """Read-out forward + backward and the compaction under torch.cuda.set_sync_debug_mode("error") (honoured by this torch build
    on ROCm: a blocking copy raises under it, checked first)."""
    from snvc_amd import depth as D
    c = DC.BY_NAME["a"]
    cost, levels, gy = tensors(c, grad=True)
    P = torch.from_numpy(DC.point_inputs(DC.POINTS_BY_NAME["single"])[1]).to(dev())
    D.depth_to_points(D.depth_readout(cost.detach(), levels, size=c.out[1:]), P, compact=True)      # the library is loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            levels.cpu()
        got, conf = D.depth_readout(cost, levels, size=c.out[1:], confidence=True)
        got.backward(gy)
        pts, counts = D.depth_to_points(got.detach(), P, conf=conf, min_conf=0.2, z_range=(DC.Z_NEAR, 40.0), compact=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert cost.grad is not None and pts.is_cuda and counts.is_cuda and 0 < int(counts.sum()) < got.numel()


@pytest.mark.parametrize("shape,out,align", [((1, 12, 3, 4), (5, 6, 8), False), ((2, 12, 3, 4), (5, 6, 9), True)], ids=["half", "aligned"])
def test_fewer_levels_than_planes_stay_on_the_kernels(shape, out, align):
    """Only H and W must not shrink: D_out < D walks the planes in steps of more than one.  Held to the float64 composition
    on the same device, with the table's bounds."""
    from snvc_amd import depth as D
    r = np.random.default_rng(5)
    cost = torch.from_numpy((3.0 * r.standard_normal(shape)).astype(np.float32)).to(dev()).requires_grad_(True)
    gy = torch.from_numpy(r.standard_normal((shape[0],) + out[1:]).astype(np.float32)).to(dev())
    levels = torch.linspace(DC.Z_NEAR, DC.Z_FAR, out[0], device=dev())
    h0, t0 = routes()
    got = D.depth_readout(cost, levels, size=out[1:], align_corners=align)
    assert routes() == (h0 + 1, t0)
    got.backward(gy)
    c64 = cost.detach().double().requires_grad_(True)
    want, _ = D._readout_torch(c64, levels.double(), out[1:], align)
    want.backward(gy.double())
    within("depth", got, want.detach().cpu().numpy(), BOUND["depth"])
    within("d cost", cost.grad, c64.grad.cpu().numpy(), BOUND["grad"])
