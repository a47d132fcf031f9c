"""The HRNet backbone on the MI355X: the fusion kernel against the torch composition it replaces, the eval forward against
the reference's outputs (tests/golden/hrnet_ref.npz, made by tests/golden/make_golden_hrnet.py), training against the same
module's torch route, and VernierScale from RoI images end to end."""
import copy
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from benchlib import hrnet as B
from benchlib.common import seeded_state
from snvc_amd import _hrnet
from snvc_amd.models import hrnet as H
from snvc_amd.models import submodule as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hrnet_ref.npz"))
DEV = "cuda:0"

# (N, C, H, W, factors of terms 0..k)
FUSE_CASES = [
    (2, 3, 16, 16, (1,)), (2, 3, 16, 16, (1, 2)), (2, 3, 16, 16, (1, 4)), (2, 3, 16, 16, (1, 8)),
    (2, 3, 16, 16, (1, 1)), (1, 5, 32, 64, (1, 2, 4)), (2, 4, 32, 32, (1, 2, 4, 8)), (2, 4, 16, 24, (1, 1, 2, 4)),
    (1, 3, 8, 12, (1, 2, 4)),           # W not a multiple of 8: the scalar form
    (1, 2, 16, 16, (2, 1, 4)),          # a term 0 of factor 2
]


def _terms(n, c, h, w, factors, seed, offset=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    out = []
    for f in factors:
        numel = n * c * (h // f) * (w // f)
        buf = torch.randn(numel + offset, generator=g).to(DEV)
        out.append(buf[offset:].view(n, c, h // f, w // f))       # offset 1: a contiguous tensor that is not 16-byte aligned
    return out


def _torch_fuse(terms, factors):
    y = F.interpolate(terms[0], scale_factor=factors[0], mode="nearest") if factors[0] > 1 else terms[0]
    for t, f in zip(terms[1:], factors[1:]):
        y = y + (F.interpolate(t, scale_factor=f, mode="nearest") if f > 1 else t)
    return torch.relu(y)


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("case", FUSE_CASES)
def test_fusion_forward_and_backward_against_torch(case, offset):
    n, c, h, w, factors = case
    terms = _terms(n, c, h, w, factors, seed=len(factors) * 100 + h + w, offset=offset)
    exp = _torch_fuse(terms, factors)
    got = _hrnet.fuse_forward(terms, list(factors))
    assert torch.equal(got, exp)
    assert torch.equal(_hrnet.fuse_forward(terms, list(factors)), got)                       # repeatable
    if factors[0] == 1:                                                                       # in place into term 0
        t0 = terms[0].clone()
        res = _hrnet.fuse_forward([t0] + terms[1:], list(factors), out=t0)
        assert res is t0 and torch.equal(t0, exp)
    # backward: torch autograd of the same composition
    leaves = [t.detach().clone().requires_grad_(True) for t in terms]
    gy = torch.randn(exp.shape, generator=torch.Generator().manual_seed(7)).to(DEV)
    _torch_fuse(leaves, factors).backward(gy)
    g = _hrnet.fuse_backward(gy, exp, factors)
    assert torch.equal(_hrnet.fuse_backward(gy, exp, factors)[factors[-1]], g[factors[-1]])  # repeatable
    for leaf, f in zip(leaves, factors):
        if f == 1:
            assert torch.equal(g[1], leaf.grad)
        else:
            assert _rel(g[f], leaf.grad) <= 1e-6, (f, _rel(g[f], leaf.grad))
    # and through the autograd function
    leaves2 = [t.detach().clone().requires_grad_(True) for t in terms]
    H._FuseSumFn.apply(tuple(factors), *leaves2).backward(gy)
    for a, b in zip(leaves2, leaves):
        assert _rel(a.grad, b.grad) <= 1e-6


def test_fusion_rejects_a_mismatched_extent():
    t0, t1 = _terms(1, 2, 16, 16, (1, 2), 3)
    with pytest.raises(RuntimeError, match="not the output"):
        _hrnet.fuse_forward([t0, t1[:, :, :7].contiguous()], [1, 2])


def _model(cfg, seed):
    m = H.get_model(copy.deepcopy(cfg), False)
    m.load_state_dict(seeded_state(m, seed), strict=True)
    return m.to(DEV)


def _eval_err(m, x, ref):
    hip0, torch0 = S._ROUTES["hrnet_hip"], S._ROUTES["hrnet_torch"]
    with torch.no_grad():
        out = m.eval()(x.to(DEV))
    assert S._ROUTES["hrnet_hip"] == hip0 + 1 and S._ROUTES["hrnet_torch"] == torch0      # one decision, the HIP route
    assert out.shape == ref.shape
    return float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", list(B.SMALL))
def test_small_configs_eval_against_the_reference(name):
    """Max error over the output's largest magnitude; 3e-5 allowed (measured on the MI355X: 6.8e-7 to 1.2e-6)."""
    cfg, wseed, xseed = B.SMALL[name]
    n, h, w = B.SMALL_INPUT
    err = _eval_err(_model(cfg, wseed), B.image((n, B.in_channels(cfg), h, w), xseed), GOLD[f"small/{name}"])
    print(f"small/{name}: rel err {err:.3e}")
    assert err <= 3e-5, err


def test_w32_eval_against_the_reference():
    """HRNet-w32 at 1 x 3 x 256 x 256, 305 convolutions; 1e-4 of the output's largest magnitude allowed (measured on the
    MI355X: 2.5e-6)."""
    err = _eval_err(_model(B.W32, B.W32_SEEDS[0]), B.image((1, 3, 256, 256), B.W32_SEEDS[1]), GOLD["w32/out"])
    print(f"w32: rel err {err:.3e}")
    assert err <= 1e-4, err


def test_input_not_a_multiple_of_32_raises():
    cfg, wseed, _ = B.SMALL["s_basic"]
    m = _model(cfg, wseed).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="not the output"):
        m(torch.zeros(1, 3, 72, 72, device=DEV))


def test_training_against_the_torch_route():
    """Train-mode BatchNorm, forward and backward: the HIP route against the same module's torch route (MIOpen) on the
    GPU: output, input gradient, every parameter gradient, running_mean / running_var.  Measured on the MI355X (max error
    over the largest magnitude): output 6.1e-6, input gradient 7.6e-6, parameter gradients 4.5e-5, running stats 6.9e-6."""
    cfg, wseed, xseed = B.SMALL["s_two_modules"]
    n, h, w = B.SMALL_INPUT
    runs = []
    for hip in (True, False):
        m = _model(cfg, wseed).train()
        x = B.image((n, 3, h, w), xseed).to(DEV).requires_grad_(True)
        saved = H.HRNET_HIP[0]
        H.HRNET_HIP[0] = hip
        try:
            hip0 = S._ROUTES["hrnet_hip"]
            y = m(x)
            assert (S._ROUTES["hrnet_hip"] > hip0) == hip
        finally:
            H.HRNET_HIP[0] = saved
        gy = B.image(tuple(y.shape), 77).to(DEV)
        y.backward(gy)
        runs.append((y.detach(), x.grad, {k: p.grad for k, p in m.named_parameters()},
                     {k: v for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))}))
    (y1, gx1, gp1, rs1), (y2, gx2, gp2, rs2) = runs
    errs = {"out": _rel(y1, y2), "grad_x": _rel(gx1, gx2)}
    # the last module's fusion rows 1..3 do not reach the "default" head's output: no gradient on either route
    unused = {k for k in gp2 if gp2[k] is None}
    assert unused == {k for k in gp1 if gp1[k] is None} and unused == _unused(m)
    errs["grad_params"] = max(_rel(gp1[k], gp2[k]) for k in gp2 if k not in unused)
    errs["running_stats"] = max(_rel(rs1[k], rs2[k]) for k in rs2)
    print("training HIP vs torch route:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(torch.isfinite(gp1[k]).all() for k in gp2 if k not in unused)
    assert errs["out"] <= 1e-4 and errs["running_stats"] <= 1e-4
    assert errs["grad_x"] <= 1e-3 and errs["grad_params"] <= 1e-3, errs


def _unused(m):
    last = len(m.stage4) - 1
    return {k for k, _ in m.named_parameters() if k.startswith(tuple(f"stage4.{last}.fuse_layers.{i}." for i in (1, 2, 3)))}


def _e2e_cfg():
    import golden_cases as GC
    grid = (16, 16, 24)
    cfg = types.SimpleNamespace(vernier_type="BEV_type3", backbone="hrfeat", gn=False, grid_resolution=list(grid),
                                resolution=GC.RESOLUTION, x_range=(-1.0, 1.0), z_range=(-1.0, 1.0), num_parts=9)
    cfg.hrfeat = copy.deepcopy(B.E2E_HRNET)
    cfg.n_sample_h, cfg.n_sample_w, cfg.n_sample_l = grid
    return cfg


def test_vernier_scale_from_images_end_to_end():
    """VernierScale (BEV_type3) with the HIP backbone from RoI images against the reference's; then one training step
    through it reaches every backbone parameter.  Errors over each output's largest magnitude, measured on the MI355X:
    features 4.5e-7, ncf 1.3e-5, coordinates 0, occupancy 2.0e-3.  The occupancy error is the 3D trunk's at this input
    scale (the seeded small HRNet's features reach ~300, the trunk tests' unit-normal ones ~4): the same trunk fed the
    reference's own features gives 2.4e-3, so the backbone adds nothing to it; 5e-3 is allowed there."""
    from snvc_amd.models.vernier import VernierScale
    cfg = _e2e_cfg()
    m = VernierScale(cfg)
    assert isinstance(m.feat_net, H.HighResolutionNet)
    m.load_state_dict(seeded_state(m, B.E2E_SEEDS[0]), strict=True)
    m.to(DEV).eval()
    imgs, gpl, gpr = B.e2e_inputs(cfg, B.E2E_SEEDS[1])
    hip0 = S._ROUTES["hrnet_hip"]
    with torch.no_grad():
        out = m(imgs[0].to(DEV), imgs[1].to(DEV), gpl.to(DEV), gpr.to(DEV))
        assert S._ROUTES["hrnet_hip"] == hip0 + 2                                  # left and right
        feats = [m.feat_net(im.to(DEV)) for im in imgs]

    def err(a, ref):
        return float(np.abs(a.cpu().numpy().astype(np.float64) - ref).max() / np.abs(ref).max())
    errs = {k: err(out[k], GOLD[f"e2e/{k}"]) for k in ("ncf", "occupancy", "coordinates")}
    errs["features"] = max(err(f, GOLD[f"e2e/{s}_feat"]) for f, s in zip(feats, ("left", "right")))
    # the same trunk fed with the reference's own features: how much of the error is the trunk's alone
    feat_net, m.feat_net = m.feat_net, torch.nn.Identity()
    try:
        with torch.no_grad():
            tr = m(*[torch.from_numpy(GOLD[f"e2e/{s}_feat"]).to(DEV) for s in ("left", "right")], gpl.to(DEV), gpr.to(DEV))
    finally:
        m.feat_net = feat_net
    errs.update({f"trunk_only_{k}": err(tr[k], GOLD[f"e2e/{k}"]) for k in ("ncf", "occupancy", "coordinates")})
    print("end to end from images:", {k: f"{v:.2e}" for k, v in errs.items()})
    assert errs["features"] <= 3e-5, errs
    assert errs["trunk_only_occupancy"] <= 5e-3 and errs["occupancy"] <= 5e-3, errs
    assert errs["coordinates"] <= 3e-4 and errs["ncf"] <= 1e-3, errs

    m.train()
    out = m(imgs[0].to(DEV), imgs[1].to(DEV), gpl.to(DEV), gpr.to(DEV))
    (out["ncf"].mean() + out["occupancy"].mean() + out["coordinates"].mean()).backward()
    unused = _unused(m.feat_net)
    grads = {k: p.grad for k, p in m.feat_net.named_parameters()}
    assert {k for k, g in grads.items() if g is None} == unused
    assert all(torch.isfinite(g).all() and g.abs().max() > 0 for k, g in grads.items() if k not in unused)
