"""The DSGN image backbone on the MI355X: the dilated depth-1 layer against F.conv2d, the SPP kernels against
F.avg_pool2d / F.interpolate, the eval forward against the reference's outputs (tests/golden/dsgn_ref*.npz, made by
tests/golden/make_golden_dsgn.py) and against the same module's torch route at full size, the torch route's cases, and
backbone features feeding the global stack."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dsgn_cases as DC
from benchlib.common import seeded_state
from snvc_amd import _dsgn, _lib, ops
from snvc_amd.models import submodule as S
from test_gpu_parity import TIGHT, check

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {}
for _f in DC.FILES:
    _z = np.load(os.path.join(ROOT, "tests", "golden", _f))
    GOLD.update({k: _z[k] for k in _z.files})
DEV = "cuda:0"


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))


def _model(fields, seed, gn=None):
    m = S.feature_extraction(DC.cfg(**fields))
    m.load_state_dict(seeded_state(m, seed), strict=True)
    return m.eval()


# ------------------------------------------------------------------ the dilated depth-1 layer
@pytest.mark.parametrize("cin,cout", [(16, 16), (32, 32), (128, 192), (192, 192), (192, 40)])
@pytest.mark.parametrize("hw", [(37, 53), (96, 312)])
def test_dilated_layer_vs_torch(cin, cout, hw):
    g = torch.Generator().manual_seed(cin * 1000 + cout + hw[0])
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 2, dilation=2, bias=False)
    bn = torch.nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g) * (2.0 / (9 * cin)) ** 0.5)
        bn.weight.uniform_(0.5, 1.5, generator=g); bn.bias.uniform_(-0.2, 0.2, generator=g)
        bn.running_mean.uniform_(-0.2, 0.2, generator=g); bn.running_var.uniform_(0.5, 1.5, generator=g)
    bn.eval()
    n = 2
    x = torch.randn((n, cin) + hw, generator=g)
    res = torch.randn((n, cout) + hw, generator=g)
    with torch.no_grad():
        raw = F.conv2d(x.double(), conv.weight.double(), None, 1, 2, 2)
        ref = (raw - bn.running_mean.double()[:, None, None]) / torch.sqrt(bn.running_var.double() + bn.eps)[:, None, None] \
            * bn.weight.double()[:, None, None] + bn.bias.double()[:, None, None]
        ref = F.relu(ref + res.double()).float()
        conv, bn = conv.to(DEV), bn.to(DEV)
        # channel-slice input and output: the layer reads channels 8.. of a wider buffer and writes channels 4.. of another
        xbuf = torch.zeros((n, cin + 8) + hw, device=DEV); xbuf[:, 8:] = x.to(DEV)
        obuf = torch.full((n, cout + 12) + hw, 7.0, device=DEV)
        before = S._ROUTES["conv2d_dilated_direct"]
        y = S.fused_conv2d(conv, bn, xbuf[:, 8:], relu=True, residual=res.to(DEV), out=obuf[:, 4:4 + cout])
        assert S._ROUTES["conv2d_dilated_direct"] == before + 1
        assert y.data_ptr() == obuf[:, 4:].data_ptr()
        assert bool((obuf[:, :4] == 7).all()) and bool((obuf[:, 4 + cout:] == 7).all()), "wrote outside its slice"
        print(f"dilated {cin}->{cout} {hw}: max rel err {_rel(y.cpu(), ref):.2e}")
        check(y.cpu().numpy(), ref.numpy(), TIGHT, "relu(bn(dilated conv) + res)")
        plain = S.fused_conv2d(conv, None, x.to(DEV))
        check(plain.cpu().numpy(), raw.float().numpy(), TIGHT, "dilated conv")
        with ops.conv_variant(_lib.ALGO_DIRECT):        # the direct form is the only form of this layer
            assert torch.equal(S.fused_conv2d(conv, None, x.to(DEV)), plain)


# ------------------------------------------------------------------ SPP kernels
@pytest.mark.parametrize("hw", [(96, 312), (64, 100), (130, 77)])
def test_spp_pool_vs_avg_pool2d(hw):
    g = torch.Generator().manual_seed(hw[1])
    x = torch.randn((2, 24) + hw, generator=g).to(DEV)
    buf = torch.randn((2, 40) + hw, generator=g).to(DEV)
    buf[:, 10:34] = x                                   # and from a channel slice
    for src in (x, buf[:, 10:34]):
        outs = _dsgn.spp_pool(src)
        for k, o in zip(_dsgn.WINDOWS, outs):
            ref = F.avg_pool2d(x, k, k)
            assert o.shape == ref.shape
            err = _rel(o, ref)
            print(f"pool {k} {hw}: max rel err {err:.2e}")
            if k == 8:
                assert torch.equal(o, ref), "8 x 8 windows are summed in F.avg_pool2d's order"
            assert err < 1e-5, (k, err)               # 16 .. 64: sums of 8 x 8 sums, another summation order


@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("hw", [(96, 312), (64, 100), (37, 53)])
def test_spp_upsample_vs_interpolate(hw, align):
    g = torch.Generator().manual_seed(hw[0] + hw[1] + align)
    h, w = hw
    maps = [torch.randn((2, 32, max(h // k, 1), max(w // k, 1)), generator=g).to(DEV) for k in (8, 16, 32, 64)]
    wide = torch.full((2, 200, h, w), 3.0, device=DEV)
    _dsgn.spp_upsample(maps, wide[:, 50:178], align)
    worst = 0.0
    for k, m in enumerate(maps):
        ref = F.interpolate(m, (h, w), mode="bilinear", align_corners=align)
        got = wide[:, 50 + 32 * k:50 + 32 * (k + 1)]
        worst = max(worst, float((got - ref).abs().max()))
    print(f"upsample {hw} align_corners={align}: max abs diff {worst:.3e}")
    assert worst == 0.0, "the upsampling is F.interpolate's arithmetic"
    assert bool((wide[:, :50] == 3).all()) and bool((wide[:, 178:] == 3).all())


# ------------------------------------------------------------------ whole module, eval
@pytest.mark.parametrize("name", sorted(DC.GOLDEN))
def test_eval_matches_the_reference(name):
    fields, shape, wseed, xseed = DC.GOLDEN[name]
    m = _model(fields, wseed).to(DEV)
    before = S._ROUTES["dsgn_hip"]
    with torch.no_grad():
        feat, rpn = m(DC.image(shape, xseed).to(DEV))
    assert S._ROUTES["dsgn_hip"] == before + 1
    for key, got in ((f"out/{name}", feat), (f"rpn/{name}", rpn)):
        if key not in GOLD:
            assert got is None, key
            continue
        ref = torch.from_numpy(GOLD[key])
        got = got[:, :ref.size(1)].cpu()
        err = _rel(got, ref)
        print(f"{key}: max err / max |ref| = {err:.2e}")
        assert err < 1e-4, (key, err)


@pytest.mark.parametrize("gn", [False, True])
def test_full_size_matches_the_torch_route(gn):
    """N = 2 (a stereo pair), 384 x 1248, reslike-det-small: the HIP route against the same module's torch route."""
    m = _model(dict(backbone="reslike-det-small", GN=gn, align_corners=False), 5).to(DEV)
    x = DC.image((2, 3, 384, 1248), 6).to(DEV)
    with torch.no_grad():
        dil = S._ROUTES["conv2d_dilated_direct"]
        hip, _ = m(x)
        assert S._ROUTES["conv2d_dilated_direct"] == dil + 8, "layer4's eight dilated layers took the dilated kernel"
        S.DSGN_HIP[0] = False
        try:
            ref, _ = m(x)
        finally:
            S.DSGN_HIP[0] = True
    assert hip.shape == (2, 32, 96, 312)
    err = _rel(hip, ref)
    print(f"full size GN={gn}: max err / max |ref| = {err:.2e}")
    assert err < 1e-4, err


# ------------------------------------------------------------------ torch route
def test_autograd_and_train_mode_take_the_torch_route():
    fields, shape, wseed, xseed = DC.GOLDEN["tiny_nobranch"]
    m = _model(fields, wseed).to(DEV)
    x = DC.image(shape, xseed).to(DEV)
    with torch.no_grad():
        ref = m._forward_torch(x)[0]
    t0, h0 = S._ROUTES["dsgn_torch"], S._ROUTES["dsgn_hip"]
    y = m(x)[0]                                         # autograd on, parameters require grad
    assert y.requires_grad and S._ROUTES["dsgn_torch"] == t0 + 1 and S._ROUTES["dsgn_hip"] == h0
    assert _rel(y.detach(), ref) < 1e-5                # MIOpen may pick other algorithms under autograd
    m.train()
    with torch.no_grad():
        y = m(x)[0]
        exp = m._forward_torch(x)[0]
    assert S._ROUTES["dsgn_torch"] == t0 + 2 and S._ROUTES["dsgn_hip"] == h0
    assert _rel(y, exp) < 1e-5                         # batch statistics: the same torch route, run twice


# ------------------------------------------------------------------ composition with the global stack
def test_backbone_features_feed_the_global_stack():
    import bench
    from snvc_amd.models.stereo_volume import GlobalStack
    m = _model(dict(backbone="reslike-det-small", GN=False, align_corners=False), 7).to(DEV)
    imgs = DC.image((2, 3, 256, 512), 8).to(DEV)
    with torch.no_grad():
        hip, _ = m(imgs)
        S.DSGN_HIP[0] = False
        try:
            ref, _ = m(imgs)
        finally:
            S.DSGN_HIP[0] = True
        scale = 1.0 / float(ref.abs().max())               # features of unit range for the stack's seeded weights
        stack = GlobalStack(32)
        stack.load_state_dict(bench.seeded_state(stack))
        stack.eval().to(DEV)
        shift = (torch.arange(24, dtype=torch.float32, device=DEV) / 2).view(1, -1)
        outs = [stack.forward_pair((f[0:1] * scale).contiguous(), (f[1:2] * scale).contiguous(), shift, 1) for f in (hip, ref)]
    err = _rel(outs[0], outs[1])
    print(f"global stack from HIP vs torch features: max err / max |ref| = {err:.2e}")
    assert torch.isfinite(outs[0]).all() and err < 1e-3, err
