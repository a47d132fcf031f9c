"""The batch statistics that the convolution kernels take in their own epilogues (train-mode BatchNorm: scale, shift, running_mean,
running_var come from them), held to the float64 moments of the very tensor the call returned, within the bound of sums taken in
float64 from the first element on (tests/stats_cases.py: the cases, the reference, the bound; tests/test_stats_cases_host.py shows on the
CPU that a float32 accumulator over runs of only 8 values misses this bound a hundredfold on the `offset` data).

  fp32 route      ops.Conv3dLayer.forward_stats: the Winograd stride-1 and stride-2 epilogues (XMODE 3) and the transposed layer's
                  (deconv3d_mfma_kernel<Cfg, 5>), csrc/conv3d.hip
  split route     ops.Conv3dLayerX3.forward_stats: the 32x32x16 forms' float32 epilogue (stride 1, stride 2, transposed) and the
                  16x16x32 form's, csrc/conv3d_f16.hip; two transposed cases on either side of the 4096 slots per sample from which
                  the slots are folded in two rounds (conv_stats_fold_rows_kernel)
  sheared layer   ops.sheared_expand_stats, which never summed in float32: the control
each on ordinary, offset (|mean| 50 .. 400 x the spread) and near-constant (one channel a single value) data; then one train-mode conv +
BatchNorm3d layer through models/submodule._norm_forward per route, statistics from the epilogue against statistics from the separate
pass over the same bits."""
import ctypes

import numpy as np
import pytest
import torch

import epilogue_ref as ER
import stats_cases as SC
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

U = ER.U
_id = lambda v: v.replace(" ", "_")     # noqa: E731


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("kind", SC.KINDS, ids=_id)
@pytest.mark.parametrize("name", list(SC.FP32_LAYERS), ids=_id)
def test_fp32_route(name, kind):
    """raw bit-identical to the plain launch, None where the layer takes no form that carries the epilogue, statistics: check_stats"""
    from snvc_amd import ops
    ci, co, sp, st, tr, _ = SC.layer_of("fp32", name)
    x, w = SC.conv_inputs("fp32", name, kind)
    gamma, beta = SC.gamma_beta(co)
    layer = ops.Conv3dLayer(_t(w), 3, st, 1, 1, tr)
    xd = _t(x)
    got = layer.forward_stats(xd, _t(gamma), _t(beta), SC.EPS)
    if name in SC.FP32_UNSUPPORTED:
        assert got is None
        return
    assert got is not None, "this layer takes a kernel form that carries the statistics epilogue"
    assert torch.equal(got[0], layer(xd))
    SC.check_stats(_np(got[0]), gamma, beta, [_np(v) for v in got[1:]], kind == "ordinary", f"fp32 route, {name}, {kind}")


def _x3_call(name, kind):
    from snvc_amd import ops
    ci, co, sp, st, tr, _ = SC.layer_of("x3", name)
    x, w = SC.conv_inputs("x3", name, kind)
    gamma, beta = SC.gamma_beta(co)
    wd, xd = _t(w), _t(x)
    forced = SC.x3_algo(SC.X3_FORCED[name]) if name in SC.X3_FORCED else None
    lay = ops.Conv3dLayerX3(wd, 3, st, 1, 1, tr, algo=forced, w_mul_dev=ops.split_scale_of(wd))
    mul = ops.split_scale_of(xd)
    xs = ops.to_split(xd, mul_dev=mul)
    got = lay.forward_stats(xs, mul, _t(gamma), _t(beta), SC.EPS)
    assert got is not None, "this kernel form carries the statistics epilogue"
    assert lay.algo == SC.x3_algo(SC.X3_FORM[name]), "the launch took another kernel form than the table names"
    assert torch.equal(got[0], lay.forward_f32(xs, mul))
    SC.check_stats(_np(got[0]), gamma, beta, [_np(v) for v in got[1:]], kind == "ordinary", f"split route, {name}, {kind}")
    return lay, xs


@pytest.mark.parametrize("kind", SC.KINDS, ids=_id)
@pytest.mark.parametrize("name", list(SC.X3_LAYERS), ids=_id)
def test_split_route(name, kind):
    """As test_fp32_route on the split kernels, the form asked of the layer after its launch"""
    _x3_call(name, kind)


@pytest.mark.parametrize("kind", SC.KINDS, ids=_id)
@pytest.mark.parametrize("name", list(SC.X3_FOLD_LAYERS), ids=_id)
def test_split_route_slot_fold(name, kind):
    """4160 slots per sample: folded 64 -> 1 into the scratch first; 4096: by the per-channel kernel alone.  Which of the two a case
    is, is read from the workspace size the library asks for: the slots, the scratch of the first round or none, the per-sample sums."""
    from snvc_amd import _lib
    lay, xs = _x3_call(name, kind)
    ci, co, sp, st, tr, _ = SC.layer_of("x3", name)
    d = lay._desc(SC.N, sp, 0, lay.algo, 0, 0, 0)
    doubles, scratch = SC.x3_workspace_doubles(SC.N, co, SC.x3_slots(name))
    assert int(_lib.lib().snvc_f16x3_conv3d_stats_workspace_bytes(ctypes.byref(d))) == 8 * doubles
    assert (scratch > 0) == (SC.X3_FOLD_SLOTS[name] > SC.FOLD_SINGLE_ROUND_MAX) and SC.x3_slots(name) == SC.X3_FOLD_SLOTS[name]


@pytest.mark.parametrize("kind", SC.KINDS, ids=_id)
@pytest.mark.parametrize("name", list(SC.SHEARED), ids=_id)
def test_sheared_first_layer(name, kind):
    """snvc_sheared_expand_stats stores no raw result: the reference is the tensor snvc_sheared_expand writes from the same operands
    (one float32 addition per element in both)."""
    from snvc_amd import ops
    q, m0 = SC.SHEARED[name]
    g, gcol, planes, (off, off_col) = SC.sheared_inputs(name, kind)
    gamma, beta = SC.gamma_beta(SC.SHEARED_SHAPE[1])
    gd, gcd, pd = _t(g), _t(gcol), _t(planes)
    raw = torch.empty(SC.SHEARED_SHAPE, device=dev())
    ops.sheared_expand(gd, gcd, pd, None, None, raw, q, m0, off, off_col, 0)
    got = ops.sheared_expand_stats(gd, gcd, pd, _t(gamma), _t(beta), SC.SHEARED_SHAPE, q, m0, off, off_col, SC.EPS)
    SC.check_stats(_np(raw), gamma, beta, [_np(v) for v in got], kind == "ordinary", f"sheared first layer, {name}, {kind}")


# =============================================================================== one layer through _norm_forward
@pytest.mark.parametrize("x3", [True, False], ids=["split_route", "fp32_route"])
def test_layer_statistics_from_the_epilogue_and_from_the_separate_pass(x3, monkeypatch):
    """One train-mode Conv3d(32 -> 32, k3) + BatchNorm3d + ReLU on offset input through submodule._norm_forward, as the autograd function
    calls it: once with the statistics from the convolution's epilogue (the route counter moves), once with forward_stats answering
    None, i.e. snvc_norm_stats over the raw tensor.  raw is the same bits both times, so both sets of statistics lie within the bounds
    em, ev, b_scale, b_shift (stats_cases / epilogue_ref.norm_stats_bounds, each + u |value| for its float32) of the same float64
    moments, and of each other within twice that:
      running_mean, running_var   m = momentum, unbias = count / (count - 1):  2 m (em + u |mean|),  2 m unbias (ev + u var), plus the
                                  update's own float32 rounding on each side, 2^-23 (|running| + |batch|) (test_bn_track's bound);
      y                           |raw| 2 b_scale + 2 b_shift + 3 u M, the last term affine_act's own (_check_affine)."""
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    name = "s1 32->32"
    ci, co, sp, st, tr, _ = SC.layer_of("x3", name)
    x, w = SC.conv_inputs("x3", name, "offset")
    gamma, beta = SC.gamma_beta(co)
    monkeypatch.setattr(S, "X3_TRAIN", [x3])
    conv = torch.nn.Conv3d(ci, co, 3, padding=1, bias=False).to(dev())
    norms = [torch.nn.BatchNorm3d(co, eps=SC.EPS).to(dev()).train() for _ in range(2)]
    with torch.no_grad():
        conv.weight.copy_(_t(w))
        for bn in norms:
            bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta))
            bn.running_mean.copy_(_t(np.linspace(-1, 1, co))); bn.running_var.copy_(_t(np.linspace(0.5, 2, co)))
    rm0, rv0 = _np(norms[0].running_mean).astype(np.float64), _np(norms[0].running_var).astype(np.float64)
    xd = _t(x)
    plan = S.plan_for(conv, "", xd.device)
    assert S._x3_train_route(conv, xd) == x3
    layer = S._X3TrainLayer(S._x3_train_layers(conv, plan)[0]) if x3 else S._get_layer(conv, plan)
    with torch.no_grad():
        before = S._ROUTES["conv_stats_epilogue"]
        a = S._norm_forward(layer, norms[0], plan, xd, None, ER.EPI_RELU, None, True)
        assert S._ROUTES["conv_stats_epilogue"] == before + 1
        monkeypatch.setattr(type(layer), "forward_stats", lambda self, *args, **kw: None)
        b = S._norm_forward(layer, norms[1], plan, xd, None, ER.EPI_RELU, None, True)
        assert S._ROUTES["conv_stats_epilogue"] == before + 1
    assert torch.equal(a.raw, b.raw) and a.y is not a.raw and b.y is not b.raw
    raw = _np(a.raw)
    for rec, what in ((a, "epilogue"), (b, "separate pass")):
        SC.check_stats(raw, gamma, beta, [_np(v) for v in (rec.scale, rec.shift, rec.mean, rec.var)], False, f"_norm_forward x3={x3}, {what}")
    err, ref, (em, ev, b_scale, b_shift) = SC.stats_errors(raw, gamma, beta, [_np(v) for v in (a.scale, a.shift, a.mean, a.var)])
    count = raw.size // co
    m, unbias = norms[0].momentum, count / (count - 1.0)
    d_mean = np.abs(_np(norms[0].running_mean).astype(np.float64) - _np(norms[1].running_mean))
    d_var = np.abs(_np(norms[0].running_var).astype(np.float64) - _np(norms[1].running_var))
    b_rm = 2 * m * (em + U * np.abs(ref["mean"]))[0] + 2 * 2.0 ** -23 * (np.abs(rm0) + np.abs(ref["mean"][0]))
    b_rv = 2 * m * unbias * (ev + U * ref["var"])[0] + 2 * 2.0 ** -23 * (np.abs(rv0) + unbias * ref["var"][0])
    assert (d_mean <= b_rm).all(), f"running_mean: {d_mean.max():.3e} > {b_rm[np.argmax(d_mean - b_rm)]:.3e}"
    assert (d_var <= b_rv).all(), f"running_var: {d_var.max():.3e} > {b_rv[np.argmax(d_var - b_rv)]:.3e}"
    assert all(int(bn.num_batches_tracked) == 1 for bn in norms)
    _, m_y = ER.affine_act_ref(raw, ref["scale"], ref["shift"], None, ER.EPI_RELU, False)
    bc = lambda v: v[0][None, :, None, None, None]      # noqa: E731
    b_y = np.abs(raw.astype(np.float64)) * 2 * bc(b_scale) + 2 * bc(b_shift) + 3 * U * m_y
    d_y = np.abs(_np(a.y).astype(np.float64) - _np(b.y))
    assert np.isfinite(_np(a.y)).all() and np.isfinite(_np(b.y)).all()
    assert (d_y <= b_y).all(), f"y: {d_y.max():.3e} apart, bound {b_y.flat[np.argmax(d_y - b_y)]:.3e}"
