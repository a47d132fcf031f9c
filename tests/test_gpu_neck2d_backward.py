"""The 2D layers under autograd against float64: every row of tests/neck2d_backward_cases.py through ``fused_conv2d`` /
``fused_deconv2d`` (``_Conv2dNormActFn``) and every composition through the HRNet blocks, the fusion and ``_FuseSumFn``, on the HIP
route -- asserted through ``_ROUTES`` -- against the table's float64 CPU reference.

y and dx at ``TIGHT`` (the data gradient is a forward form of the family: the family's forward tolerance), dW at 2e-5 (what
test_conv3d_wgrad_vs_float64 allows the auto and fp32 forms), dgamma / dbeta / dbias and a masked residual gradient at ``TIGHT``,
running statistics at 1e-5; a residual gradient behind no activation, or added after it, equals gy bit for bit and is the very tensor
the epilogue's backward was given (no pass writes a copy of it); what was not asked for is None; two runs give equal bits.  Measured
per row and quantity (HIP 6e-9 to 1.5e-6): profiles/neck2d_backward/measured_errors.txt; what the test catches:
profiles/neck2d_backward/negative_check.txt.
"""
import contextlib

import pytest
import torch

import neck2d_backward_cases as NB
from test_gpu_parity import TIGHT, check, dev

pytestmark = pytest.mark.gpu

TOL = {"y": TIGHT, "dx": TIGHT, "dw": 2e-5, "dgamma": TIGHT, "dbeta": TIGHT, "dbias": TIGHT, "dres": TIGHT,
       "running_mean": 1e-5, "running_var": 1e-5}
GRADS = ("dx", "dw", "dgamma", "dbeta", "dbias", "dres")


def _routes():
    from snvc_amd.models import submodule as S
    return S._ROUTES["neck2d_hip_train"], S._ROUTES["neck2d_torch"], S._ROUTES["hrnet_torch"]


def _layer(row, data):
    """The row's modules on the device: conv (or transposed conv), norm or None."""
    nn = torch.nn
    if row.kind == NB.DECONV:
        conv = nn.ConvTranspose2d(row.cin, row.cout, kernel_size=3, padding=1, output_padding=1, stride=2, bias=False)
    elif row.kind == NB.WHOLE:
        conv = nn.Conv2d(row.cin, row.cout, (row.h, row.w), bias=row.norm == "bias")
    else:
        k, s = row.kind[1], row.kind[2]
        conv = nn.Conv2d(row.cin, row.cout, k, s, (k - 1) // 2, bias=row.norm == "bias")
    norm = None
    if row.norm in ("bn_train", "bn_frozen"):
        norm = nn.BatchNorm2d(row.cout, eps=1e-5, momentum=0.1)
        norm.train(row.norm == "bn_train")
    elif row.norm == "gn":
        norm = nn.GroupNorm(row.groups, row.cout, eps=1e-5)
    with torch.no_grad():
        conv.weight.copy_(data["weight"])
        if conv.bias is not None:
            conv.bias.copy_(data["bias"])
        if norm is not None:
            norm.weight.copy_(data["gamma"])
            norm.bias.copy_(data["beta"])
        if isinstance(norm, nn.BatchNorm2d):
            norm.running_mean.copy_(data["running_mean"])
            norm.running_var.copy_(data["running_var"])
    conv.weight.requires_grad_("weight" in row.needs)
    for p in ([conv.bias] if conv.bias is not None else []) + (list(norm.parameters()) if norm is not None else []):
        p.requires_grad_("affine" in row.needs)
    return conv.to(dev()), (norm.to(dev()) if norm is not None else None)


def run_hip(row, data, gy, forced=True):
    """One forward + backward of the row on the HIP route; every result on the CPU, a gradient that was not produced as None."""
    from snvc_amd import _lib, ops
    from snvc_amd.models import submodule as S
    conv, norm = _layer(row, data)
    x = data["x"].to(dev()).requires_grad_("x" in row.needs)
    res = data["residual"].to(dev()).requires_grad_("residual" in row.needs) if row.residual != "none" else None
    variant = ops.conv_variant(getattr(_lib, row.variant)) if (row.variant and forced) else contextlib.nullcontext()
    seen, inner = [], S._epilogue_backward

    def spy(rec, gy, *a, **kw):         # what the epilogue's backward hands back for the residual, next to the gy it was given
        got = inner(rec, gy, *a, **kw)
        seen.append((gy, got[1]))
        return got
    S._epilogue_backward = spy
    try:
        return _run(row, S, conv, norm, x, res, variant, gy, seen)
    finally:
        S._epilogue_backward = inner


def _run(row, S, conv, norm, x, res, variant, gy, seen):
    with variant:
        if row.kind == NB.DECONV:
            y = S.fused_deconv2d(conv, norm, x, relu=row.act == "relu", residual=res)
        else:
            y = S.fused_conv2d(conv, norm, x, relu=row.act == "relu", sigmoid=row.act == "sigmoid", residual=res,
                               residual_after_act=row.residual == "after", transposed_input=row.transposed_input)
        y.backward(gy.to(dev()))
    cpu = lambda t: None if t is None else t.detach().cpu()      # noqa: E731
    out = dict(y=cpu(y), dx=cpu(x.grad), dw=cpu(conv.weight.grad), dres=cpu(res.grad) if res is not None else None,
               dgamma=cpu(norm.weight.grad) if norm is not None else None, dbeta=cpu(norm.bias.grad) if norm is not None else None,
               dbias=cpu(conv.bias.grad) if conv.bias is not None else None)
    if row.norm == "bn_train":
        out["running_mean"], out["running_var"] = cpu(norm.running_mean), cpu(norm.running_var)
    assert len(seen) == 1
    out["gres_is_gy"] = torch.tensor(seen[0][1] is not None and seen[0][1].data_ptr() == seen[0][0].data_ptr())
    return out


def _same_bits(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), f"{what}: {k} differs in bits"


@pytest.mark.parametrize("row", NB.ROWS, ids=[r.name for r in NB.ROWS])
def test_row(row):
    data = NB.build(row)
    ref = NB.reference(row, data)
    before = _routes()
    got = run_hip(row, data, ref["gy"])
    after = _routes()
    assert after == (before[0] + 1, before[1], before[2]), "one layer through the HIP autograd function, none on a torch route"
    want = NB.requested(row)
    errs = {k: NB.rel_err(got[k], ref[k]) for k in ["y"] + want + [k for k in ("running_mean", "running_var") if k in ref]}
    print(f"measured {row.name}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    for k in GRADS:
        assert (got[k] is not None) == (k in want), f"{row.name}: {k} asked for: {k in want}, returned: {got[k] is not None}"
    for k in errs:
        if k == "dres" and NB.residual_gradient_is_gy(row):
            assert torch.equal(got[k], ref["gy"]), "behind no activation, or added after it, the residual's gradient is gy itself"
            assert bool(got["gres_is_gy"]), "... the very tensor: no pass writes a copy of gy"
        else:
            check(got[k].numpy(), ref[k].float().numpy(), TOL[k], f"{row.name} {k}")
    _same_bits(run_hip(row, data, ref["gy"]), got, f"{row.name}: second run")
    if row.same_as:                     # a ``needs`` variant: what is still returned equals the full row's bit for bit
        full = run_hip(NB.BY_NAME[row.same_as], data, ref["gy"])
        for k in ["y"] + want:
            assert torch.equal(got[k], full[k]), f"{row.name}: {k} changed with needs_input_grad"
    if row.variant:
        assert not torch.equal(run_hip(row, data, ref["gy"], forced=False)["y"], got["y"]), "the forced form is a different kernel"


def _comp_hip(c, gy):
    from snvc_amd.models import hrnet as H
    m = NB.make_module(c)
    xs0, _ = NB.comp_inputs(c)
    xs = [x.to(dev()).requires_grad_(i != c.frozen) for i, x in enumerate(xs0)]
    if c.what == "fuse_sum":
        outs, which = [H._FuseSumFn.apply(tuple(c.factors), *xs)], 0
    else:
        m = m.to(dev())
        outs, which = (m(xs), NB.FUSE_ROW) if c.what == "fuse_row" else ([m(xs[0])], 0)
    outs[which].backward(gy.to(dev()))
    cpu = lambda t: None if t is None else t.detach().cpu()      # noqa: E731
    out = {f"y{i}": cpu(o) for i, o in enumerate(outs)}
    out.update({f"dx{i}": cpu(x.grad) for i, x in enumerate(xs)})
    if m is not None:
        out.update({"d " + k: cpu(p.grad) for k, p in m.named_parameters()})
        out.update({k: cpu(v) for k, v in m.state_dict().items() if k.endswith(("running_mean", "running_var"))})
    return out


@pytest.mark.parametrize("c", NB.COMPOSITIONS, ids=[c.name for c in NB.COMPOSITIONS])
def test_composition(c):
    from snvc_amd.models import submodule as S
    ref = NB.comp_reference(c)
    before, hip0 = _routes(), S._ROUTES["hrnet_hip"] + S._ROUTES["neck2d_hip"]
    got = _comp_hip(c, ref["gy"])
    after = _routes()
    assert after == (before[0] + c.layers, before[1], before[2]), (before, after, c.layers)
    assert c.what == "fuse_sum" or S._ROUTES["hrnet_hip"] + S._ROUTES["neck2d_hip"] == hip0 + 1
    exp = {f"y{i}": v for i, v in enumerate(ref["ys"])}
    exp.update({f"dx{i}": v for i, v in enumerate(ref["dx"])})
    exp.update({"d " + k: v for k, v in ref.get("params", {}).items()})
    exp.update(ref.get("stats", {}))
    assert set(exp) == set(got)
    errs = {}
    for k, e in exp.items():
        assert (got[k] is None) == (e is None), f"{c.name}: {k}"
        if e is not None:
            errs[k] = NB.rel_err(got[k], e)
    worst = max(errs, key=errs.get)
    print(f"measured {c.name}: " + ", ".join(f"{k} {errs[k]:.1e}" for k in errs if k[0] in "y" or k.startswith("dx")) + f", worst {worst} {errs[worst]:.1e}")
    if c.frozen is not None:
        assert got[f"dx{c.frozen}"] is None
    for k, e in exp.items():
        if e is not None:
            check(got[k].numpy(), e.float().numpy(), 1e-5 if "running" in k else TIGHT, f"{c.name} {k}")
    _same_bits(_comp_hip(c, ref["gy"]), got, f"{c.name}: second run")


@pytest.mark.parametrize("name", sorted(NB.REFUSED))
def test_refused(name):
    """What the table leaves out by name is refused aloud, not computed some other way."""
    from snvc_amd.models import submodule as S
    nn = torch.nn
    x = torch.randn(2, 8, 6, 8, device=dev(), requires_grad=True)
    with pytest.raises(NotImplementedError):
        if name == "bias_with_norm":
            S.fused_conv2d(nn.Conv2d(8, 8, 3, 1, 1, bias=True).to(dev()), nn.BatchNorm2d(8).to(dev()).train(), x, relu=True)
        elif name == "dilated_training":
            S.fused_conv2d(nn.Conv2d(8, 8, 3, 1, 2, dilation=2, bias=False).to(dev()), None, x)
        elif name == "out_training":
            S.fused_conv2d(nn.Conv2d(8, 8, 3, 1, 1, bias=False).to(dev()), None, x, out=torch.empty(2, 8, 6, 8, device=dev()))
        else:
            assert name == "deconv_bias"
            S.fused_deconv2d(nn.ConvTranspose2d(8, 8, 3, 2, 1, 1, bias=True).to(dev()), None, x)
