"""GPU checks of the training losses on the HIP route (snvc_amd.models.loss3d, csrc/loss.hip): loss and gradient against
the reference's float64 results on the small cases (tests/golden/loss3d_ref.npz) and against the float64 restatement of
tests/loss_cases.py at working sizes, exact zeros where the mask excludes an element, run-to-run bit equality, strided
predictions, empty masks, the deferred input checks, one training step through VernierScale, and no host synchronisation.

Bounds: 1e-5 relative on the scalar and 1e-5 of the gradient's maximum (the project's fp32 whole-tensor bound); the
p in {0, 1} occupancy case element by element, |got - ref| <= 1e-5 |ref|.  Every test prints the measured error beside the
reference's own float32-against-float64 error (e32) of the golden file.

No synchronisation: this torch build honours torch.cuda.set_sync_debug_mode("error") on ROCm (a blocking copy raises under
it, checked by the test itself first), so forward + backward run under "error"."""
import os

import numpy as np
import pytest
import torch

import golden_cases as GC
import loss_cases as LC
from snvc_amd.models import loss3d

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "loss3d_ref.npz"))
HIP_SMALL = sorted(n for n in LC.SMALL if LC.SMALL[n][0] in LC.HIP_KINDS)
EPS = 2.0 ** -23


def dev():
    return torch.device("cuda:0")


def _run(name, x=None):
    x = x or LC.inputs(name, torch.float32, dev())
    loss, grads = LC.loss_and_grads(lambda v: LC.call(loss3d, name, v), x)
    return loss.cpu(), {k: g.cpu() for k, g in grads.items()}


def _compare(name, loss, grads, ref_loss, ref_grads, e32=None, elementwise=False):
    assert loss.dtype == torch.float32 and loss.shape == ref_loss.shape, name
    top = float(ref_loss.abs().max()) if ref_loss.numel() else 0.0
    e_loss = float((loss.double() - ref_loss).abs().max()) / top if top > 0 else float(loss.abs().max()) if loss.numel() else 0.0
    e_grad = 0.0
    for k, ref in ref_grads.items():
        g = grads[k]
        assert g.shape == ref.shape and g.dtype == torch.float32, (name, k)
        err = (g.double() - ref).abs()
        gtop = float(ref.abs().max())
        e_grad = max(e_grad, float(err.max()) / gtop if gtop > 0 else float(g.abs().max()))
        assert bool((g[ref == 0] == 0).all()), f"{name}/{k}: a gradient the reference has at exactly 0 is not 0"
        if elementwise:
            assert bool((err <= 1e-5 * ref.abs()).all()), f"{name}/{k}: element-wise, worst {float((err / ref.abs().clamp_min(1e-300)).max()):.2e}"
    ref32 = "" if e32 is None else f"  reference float32: loss {e32[0]:.1e} grad {e32[1]:.1e}  (8 x max(e32, 2^-23): {8 * max(e32[0], EPS):.1e} / {8 * max(e32[1], EPS):.1e})"
    print(f"[loss] {name:14s} HIP: loss {e_loss:.1e} grad {e_grad:.1e}{ref32}")
    assert e_loss <= 1e-5, (name, e_loss)
    assert e_grad <= 1e-5, (name, e_grad)
    return e_loss, e_grad


@pytest.mark.parametrize("name", HIP_SMALL)
def test_small_cases_against_the_reference(name):
    loss, grads = _run(name)
    ref_grads = {k: torch.from_numpy(GOLD[f"grad64/{name}/{k}"]) for k in grads}
    _compare(name, loss, grads, torch.from_numpy(GOLD[f"loss64/{name}"]), ref_grads, GOLD[f"e32/{name}"], elementwise=name == "occ_edge")


def test_occupancy_with_saturated_predictions_is_finite():
    loss, grads = _run("occ_edge")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grads["pred"]).all())
    x = LC.inputs("occ_edge")
    p, t = x["diff"]["pred"].detach().reshape(-1), x["const"]["gt"].reshape(-1)
    for value in (0.0, 1.0):                         # the case does hold saturated predictions at ignored and at counted voxels
        assert bool(((p == value) & (t == -1)).any()) and bool(((p == value) & (t == 0)).any()) and bool(((p == value) & (t == 1)).any())


@pytest.mark.parametrize("name", sorted(LC.WORK))
def test_working_sizes_against_the_float64_restatement(name):
    ref_loss, ref_grads = LC.loss_and_grads(lambda v: LC.restate(name, v), LC.inputs(name))
    loss, grads = _run(name)
    _compare(name, loss, grads, ref_loss, ref_grads)
    again_loss, again = _run(name)                   # the same bits twice
    assert torch.equal(loss, again_loss) and all(torch.equal(grads[k], again[k]) for k in grads)


@pytest.mark.parametrize("name", HIP_SMALL)
def test_two_runs_give_the_same_bits(name):
    a, b = _run(name), _run(name)
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])


@pytest.mark.parametrize("name", ["occ", "offset", "depth", "w_mean", "depthreg", "msew", "disp_sl1"])
def test_gradient_is_exactly_zero_where_the_mask_excludes(name):
    x = LC.inputs(name, torch.float32, dev())
    _, grads = _run(name, x)
    kind, o = LC.CASES[name]
    c = {k: v.cpu() for k, v in x["const"].items()}
    for k, g in grads.items():
        if kind == "occ":
            out = c["gt"] == -1
        elif kind == "offset":
            out = (c["occ"] != 1)[:, None].expand(-1, g.size(1), -1, -1, -1)
        elif kind in ("depth",):
            out = ~((c["gt"] != -1) & (c["gt"] < 60))
        elif kind == "depthreg":
            out = (~((c["gt"] != -1) & (c["gt"] < 60)))[:, None].expand_as(g)
        elif kind == "wloss":
            out = (~c["mask"])[:, None].expand_as(g)
        elif kind == "disp":
            out = (~c["mask"])[:, None]
        else:
            out = torch.zeros_like(g, dtype=torch.bool)
        assert bool(out.any()) or kind == "msew"
        assert bool((g[out] == 0).all()), (name, k)
        assert bool((g[~out] != 0).any())


@pytest.mark.parametrize("name", ["mse", "occ_odd", "depth", "depthreg", "w_mean_odd", "sl1rows", "focal"])
def test_strided_predictions(name):
    """A transposed view, and a channel slice of a wider buffer: the same loss and gradient as the dense tensor."""
    want_loss, want = _run(name)
    for make in ("transpose", "slice"):
        x = LC.inputs(name, torch.float32, dev())
        for k, t in list(x["diff"].items()):
            base = t.detach()
            if make == "transpose":
                view = base.transpose(0, -1).contiguous().transpose(0, -1)
            else:
                wide = torch.zeros((base.size(0), 3 * base.size(1)) + tuple(base.shape[2:]), device=base.device)
                wide[:, base.size(1):2 * base.size(1)] = base
                view = wide[:, base.size(1):2 * base.size(1)]
            assert torch.equal(view, base)
            x["diff"][k] = view.requires_grad_(True)
        loss, grads = _run(name, x)
        assert torch.equal(loss, want_loss), (name, make)
        assert all(torch.equal(grads[k], want[k]) for k in want), (name, make)


@pytest.mark.parametrize("name", ["occ_empty", "offset_empty", "depth_empty"])
def test_empty_mask_gives_zero_loss_and_zero_gradient(name):
    x = LC.inputs(name, torch.float32, dev())
    out = LC.call(loss3d, name, x)
    assert out.dim() == 0 and out.dtype == torch.float32 and out.requires_grad and float(out.detach()) == 0.0
    out.backward()
    for t in x["diff"].values():
        assert t.grad is not None and not bool(t.grad.any())


def test_depth_regression_with_an_empty_mask():
    x = LC.inputs("depthreg", torch.float32, dev())
    x["const"]["gt"].fill_(-1.0)
    out = LC.call(loss3d, "depthreg", x)
    out.backward()
    assert float(out.detach()) == 0.0 and not bool(x["diff"]["cost"].grad.any())


def test_deferred_input_checks_raise():
    loss3d.check()                                   # nothing pending
    x = LC.inputs("msew", torch.float32, dev())
    x["const"]["gt"][:, 1] = -1.0                    # part 1 without a positive target
    out = LC.call(loss3d, "msew", x)                 # does not raise: nothing waits for the device
    assert bool(torch.isnan(out))                    # the mean over no element
    with pytest.raises(loss3d.LossInputError, match="positive"):
        loss3d.check()
    loss3d.check()                                   # the flag was cleared
    y = LC.inputs("focal", torch.float32, dev())
    y["const"]["targets"][3, 3] = 2
    LC.call(loss3d, "focal", y)
    torch.cuda.synchronize()
    with pytest.raises(loss3d.LossInputError, match="0 or 1"):
        LC.call(loss3d, "focal", LC.inputs("focal", torch.float32, dev()))      # the next call looks
    LC.call(loss3d, "focal", LC.inputs("focal", torch.float32, dev()))
    loss3d.check()
    z = LC.inputs("focal_w", torch.float32, dev())
    z["const"]["targets"][0, 0] = 0.5
    LC.call(loss3d, "focal_w", z)
    with pytest.raises(loss3d.LossInputError, match="0 or 1"):
        loss3d.check()


def test_disparity_regression_is_differentiable():
    from snvc_amd import ops
    g = torch.Generator().manual_seed(5)
    for shape in ((2, 12, 6, 8), (1, 5, 3, 7)):
        x = torch.softmax(torch.randn(*shape, generator=g), 1)
        depth = torch.linspace(2.0, 40.0, shape[1])
        up = torch.randn(shape[0], *shape[2:], generator=g)
        xr = x.double().requires_grad_(True)
        (torch.sum(xr * depth.double()[None, :, None, None], 1) * up.double()).sum().backward()
        xd = x.to(dev()).requires_grad_(True)
        with torch.no_grad():
            plain = ops.disparity_regression(xd, depth.to(dev()))
        out = ops.disparity_regression(xd, depth.to(dev()))
        assert out.requires_grad and not plain.requires_grad and torch.equal(out.detach(), plain)      # the same kernel, bit for bit
        (out * up.to(dev())).sum().backward()
        assert float((xd.grad.cpu().double() - xr.grad).abs().max()) <= 1e-5 * float(xr.grad.abs().max())


def test_depth_regression_loss_trains_the_depth_head_through_the_plain_ops():
    """depth_regression_loss equals DepthLoss over the differentiable ops.disparity_regression of a softmax."""
    from snvc_amd import ops
    x = LC.inputs("depthreg", torch.float32, dev())
    cost, levels, gt = x["diff"]["cost"], x["const"]["levels"], x["const"]["gt"]
    fused = loss3d.depth_regression_loss(cost, levels, gt)
    fused.backward()
    g_fused, cost.grad = cost.grad.clone(), None
    two = loss3d.DepthLoss()({"depth": ops.disparity_regression(torch.softmax(cost, 1), levels)}, {"gt_depth": gt})
    two.backward()
    assert abs(float(fused.detach()) - float(two.detach())) <= 1e-5 * abs(float(two.detach()))
    assert float((g_fused - cost.grad).abs().max()) <= 1e-5 * float(cost.grad.abs().max())


def _model(grid):
    import types
    from benchlib.common import seeded_state
    from snvc_amd.models.vernier import VernierScale
    cfg = types.SimpleNamespace(vernier_type="BEV_type3", backbone="hrfeat", gn=False, grid_resolution=list(grid),
                                resolution=GC.RESOLUTION, x_range=(-1.0, 1.0), z_range=(-1.0, 1.0), num_parts=9)
    cfg.hrfeat = types.SimpleNamespace(output_channel=32, name="identity")
    cfg.n_sample_h, cfg.n_sample_w, cfg.n_sample_l = grid
    m = VernierScale(cfg)
    m.load_state_dict(seeded_state(m, 91))
    return m, cfg


def test_one_training_step_through_vernier_scale():
    """VernierScale forward, VoxelMSELoss + OccupancyLoss + CoordinateLoss, backward: every parameter gradient of the step
    with the HIP losses against the same step with the torch route of the losses (float32, on the GPU), at the project's bound
    for gradients, 1e-5 of each gradient's maximum.  The torch route carries float32 rounding of its own, so both routes are
    also measured against the step whose loss gradients are taken in float64 (the model's outputs cast up, the torch route's
    arithmetic, the gradients cast down and sent through the model's backward), and the HIP route is held to 1e-5 against
    that one too.  Every figure is printed.  The compared steps follow one warm-up step: the model's first backward of a
    process differs from its later ones by 2.2e-5 in coord_head.0.bn2.weight whichever route the losses take (printed as
    well), while a repeated HIP step is bit-equal.  Measured on an MI355X: hip vs torch 1.4e-6, hip vs float64 1.2e-6,
    torch vs float64 1.3e-6."""
    grid = (16, 16, 24)
    m, cfg = _model(grid)
    m = m.eval().to(dev())                           # frozen BatchNorm: the step is a linear function of the loss gradients
    lf, rf, gpl, gpr = (t.to(dev()) for t in GC.trunk_inputs(2, 32, 16, 16, grid, 92))
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        shapes = {k: v.shape for k, v in m(lf, rf, gpl.clone(), gpr.clone()).items()}
    hm = torch.rand(shapes["ncf"], generator=g).to(dev())
    u = torch.rand(shapes["occupancy"], generator=g)
    occ = torch.where(u < 0.3, -1.0, torch.where(u < 0.5, 1.0, 0.0)).to(dev())
    corners = torch.randn(shapes["coordinates"][0], 9, 3, generator=g).to(dev())
    losses = (loss3d.VoxelMSELoss(), loss3d.OccupancyLoss(), loss3d.CoordinateLoss(cfg))

    def total_of(out, dtype=torch.float32):
        return (losses[0](out, hm.to(dtype)) + losses[1](out, occ.to(dtype)) + losses[2](out, {"gt_corners_local": corners.to(dtype)}))

    def step(route):
        m.zero_grad(set_to_none=True)
        out = m(lf, rf, gpl.clone(), gpr.clone())
        if route == "hip":
            total = total_of(out)
            total.backward()
        elif route == "torch":
            with loss3d._torch_route():
                total = total_of(out)
            total.backward()
        else:                                        # the loss and its gradients in float64
            keys = sorted(out)
            up = {k: out[k].detach().double().requires_grad_(True) for k in keys}
            total = total_of(up, torch.float64)
            g64 = torch.autograd.grad(total, [up[k] for k in keys])
            torch.autograd.backward([out[k] for k in keys], [t.float() for t in g64])
        return float(total.detach()), {k: p.grad.detach().cpu().double() for k, p in m.named_parameters() if p.grad is not None}

    first = step("hip")[1]                           # see the docstring: the model's first backward is not its later ones
    l_hip, g_hip = step("hip")
    l_ref, g_ref = step("torch")
    l_64, g_64 = step("float64")
    again = step("hip")[1]
    assert set(g_hip) == set(g_ref) == set(g_64) and len(g_ref) >= 30

    def worst(got, ref):
        errs = {k: float((got[k] - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref if float(ref[k].abs().max()) > 0}
        k = max(errs, key=errs.get)
        return errs[k], k
    rerun, warm = worst(again, g_hip), worst(first, g_hip)
    hip_torch, hip_64, torch_64 = worst(g_hip, g_ref), worst(g_hip, g_64), worst(g_ref, g_64)
    print(f"[loss] training step: loss hip {l_hip:.7f} torch {l_ref:.7f} float64 {l_64:.9f}")
    print(f"[loss] training step: worst parameter gradient error over its maximum: hip vs torch {hip_torch[0]:.1e} ({hip_torch[1]}), "
          f"hip vs float64 {hip_64[0]:.1e} ({hip_64[1]}), torch vs float64 {torch_64[0]:.1e} ({torch_64[1]}), "
          f"hip vs hip again {rerun[0]:.1e} ({rerun[1]}), the process's first step vs hip {warm[0]:.1e} ({warm[1]})")
    assert abs(l_hip - l_ref) <= 1e-5 * abs(l_ref) and abs(l_hip - l_64) <= 1e-5 * abs(l_64)
    assert hip_64[0] <= 1e-5, hip_64
    assert hip_torch[0] <= 1e-5, hip_torch


@pytest.mark.parametrize("name", ["occ", "occ_tail", "mse_w_rows", "msew_tail", "offset", "depth", "w_mean", "disp_sl1", "focal", "focal_i64", "sl1rows"])
def test_prediction_one_element_into_its_buffer(name):
    """A contiguous prediction that starts 4 bytes into its allocation (a view that .contiguous() returns as it is): row
    lengths are multiples of 4 but the pointer is not 16-byte aligned, so the scalar form of the kernels runs."""
    x = LC.inputs(name, torch.float32, dev())
    for k, t in list(x["diff"].items()):
        buf = torch.zeros(t.numel() + 1, device=dev())
        buf[1:] = t.detach().reshape(-1)
        view = buf[1:].view(t.shape)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        x["diff"][k] = view.requires_grad_(True)
    loss, grads = _run(name, x)
    ref_grads = {k: torch.from_numpy(GOLD[f"grad64/{name}/{k}"]) for k in grads}
    _compare(name + "+4B", loss, grads, torch.from_numpy(GOLD[f"loss64/{name}"]), ref_grads, GOLD[f"e32/{name}"])


@pytest.mark.parametrize("name", ["occ", "offset", "mse", "mse_w_rows", "msew", "depth", "w_mean", "disp_sl1", "focal", "focal_i64", "focal_bool", "sl1rows", "depthreg"])
def test_forward_and_backward_never_wait_for_the_device(name):
    x = LC.inputs(name, torch.float32, dev())
    LC.call(loss3d, name, x).backward()              # first call: loads the library, allocates the pinned flag copy
    torch.cuda.synchronize()
    for t in x["diff"].values():
        t.grad = None
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):            # the mode is honoured by this build: a blocking copy raises
            x["const"][next(iter(x["const"]))].cpu()
        out = LC.call(loss3d, name, x)
        out.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(t.grad is not None for t in x["diff"].values())
    loss3d.check()
