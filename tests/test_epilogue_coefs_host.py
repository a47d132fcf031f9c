"""The coefficient step of the training epilogue's backward (snvc_amd/models/submodule.py::_backward_coefs: GroupNorm, train-mode
and frozen BatchNorm) on float64 CPU tensors against the float64 restatement in tests/epilogue_ref.py (pinned to float64 torch autograd
by tests/test_epilogue_ref_host.py).  Both sides evaluate the same expressions in float64, so they differ by a few 2^-53 of the
magnitude of each expression's terms; the bound is 1e-12 of that magnitude, element by element (the margin of
tests/test_wgrad_ref_host.py).  Float64 ``mean`` / ``var`` keep the train-mode BatchNorm case on the torch branch (float32 batch
statistics take one GPU launch, held to the same reference by tests/test_gpu_epilogue.py)."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import epilogue_ref as ER

EPS = float(np.float32(1e-5))
KEYS = ("coef_g", "coef_raw", "coef_const", "dgamma", "dbeta")
SHAPES = [(2, 6, 2), (2, 6, 3), (2, 70, 35)]                  # n, c, GroupNorm groups
COUNTS = [20, 773]                                            # S: elements per (n, c)


def _case(n, c, rows, seed):
    """Sums as a reduction over ordinary data leaves them, statistics with an offset (mean about 3, var in (0.25, 4): sgr - mu * sg
    cancels), gamma of both signs."""
    r = np.random.default_rng(seed)
    return dict(sums=r.standard_normal((n, c, 2)) * np.array([5.0, 15.0]), mean=3.0 + r.standard_normal(rows),
                var=r.uniform(0.25, 4.0, rows), gamma=r.uniform(0.5, 2, c) * r.choice([-1.0, 1.0], c))


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _norm(cls, *args, gamma=None):
    norm = cls(*args, eps=EPS, affine=gamma is not None).double()
    if gamma is not None:
        with torch.no_grad():
            norm.weight.copy_(_t(gamma))
    return norm


def _check(got, ref, mags, what, gamma_given):
    assert len(got) == len(KEYS)
    for key, g in zip(KEYS, got):
        if ref[key] is None or (key in ("dgamma", "dbeta") and not gamma_given):
            assert g is None, f"{what} {key}: expected None"
            continue
        assert g.dtype == torch.float64, (what, key, g.dtype)
        g = g.numpy()
        assert g.shape == ref[key].shape, (what, key, g.shape, ref[key].shape)
        over = np.abs(g - ref[key]) - 1e-12 * mags[key]
        assert over.max() <= 0.0, f"{what} {key}: |got - ref| exceeds 1e-12 of the magnitude by {over.max():.3e}"


@pytest.mark.parametrize("with_gamma", [True, False], ids=["gamma", "no_gamma"])
@pytest.mark.parametrize("s", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "n%d_c%d_g%d" % v)
def test_groupnorm(shape, s, with_gamma):
    from snvc_amd.models import submodule as S
    n, c, groups = shape
    d = _case(n, c, (n, groups), 7 + c + groups + s)
    gamma = d["gamma"] if with_gamma else None
    got = S._backward_coefs(_t(d["sums"]), _t(d["mean"]), _t(d["var"]), _norm(nn.GroupNorm, groups, c, gamma=gamma), s)
    ref, mags = ER.gn_backward_coefs_ref(d["sums"], d["mean"], d["var"], gamma, groups, (c // groups) * s, EPS)
    _check(got, ref, mags, f"groupnorm {shape} S={s}", with_gamma)
    if not with_gamma:                 # the coefficients of gamma = 1
        ones, ones_m = ER.gn_backward_coefs_ref(d["sums"], d["mean"], d["var"], np.ones(c), groups, (c // groups) * s, EPS)
        _check(got[:3] + (None, None), ones, ones_m, f"groupnorm {shape} S={s} against gamma = 1", False)


@pytest.mark.parametrize("with_gamma", [True, False], ids=["gamma", "no_gamma"])
@pytest.mark.parametrize("s", COUNTS)
@pytest.mark.parametrize("shape", [(2, 6), (2, 70)], ids=lambda v: "n%d_c%d" % v)
def test_train_batchnorm(shape, s, with_gamma):
    from snvc_amd.models import submodule as S
    n, c = shape
    d = _case(n, c, (1, c), 11 + c + s)
    gamma = d["gamma"] if with_gamma else None
    got = S._backward_coefs(_t(d["sums"]), _t(d["mean"]), _t(d["var"]), _norm(nn.BatchNorm3d, c, gamma=gamma).train(), s)
    ref, mags = ER.bn_backward_coefs_ref(d["sums"], d["mean"][0], d["var"][0], gamma, n * s, EPS)
    _check(got, ref, mags, f"train batchnorm {shape} S={s}", with_gamma)
    if not with_gamma:
        ones, ones_m = ER.bn_backward_coefs_ref(d["sums"], d["mean"][0], d["var"][0], np.ones(c), n * s, EPS)
        _check(got[:3] + (None, None), ones, ones_m, f"train batchnorm {shape} S={s} against gamma = 1", False)


@pytest.mark.parametrize("with_gamma", [True, False], ids=["gamma", "no_gamma"])
@pytest.mark.parametrize("shape", [(2, 6), (2, 70)], ids=lambda v: "n%d_c%d" % v)
def test_frozen_batchnorm(shape, with_gamma):
    """Eval mode: the running statistics, no statistics of this forward (mean = var = None); the count does not enter."""
    from snvc_amd.models import submodule as S
    n, c = shape
    d = _case(n, c, (c,), 13 + c)
    gamma = d["gamma"] if with_gamma else None
    bn = _norm(nn.BatchNorm3d, c, gamma=gamma).eval()
    with torch.no_grad():
        bn.running_mean.copy_(_t(d["mean"])); bn.running_var.copy_(_t(d["var"]))
    got = S._backward_coefs(_t(d["sums"]), None, None, bn, 20)
    ref, mags = ER.frozen_bn_backward_coefs_ref(d["sums"], d["mean"], d["var"], gamma, EPS)
    _check(got, ref, mags, f"frozen batchnorm {shape}", with_gamma)
    if not with_gamma:
        ones, ones_m = ER.frozen_bn_backward_coefs_ref(d["sums"], d["mean"], d["var"], np.ones(c), EPS)
        _check(got[:3] + (None, None), ones, ones_m, f"frozen batchnorm {shape} against gamma = 1", False)


def test_float32_cast_at_the_caller():
    """What act_backward_apply is handed: contiguous float32, [C] for BatchNorm and [N, C] for GroupNorm, None passed through."""
    from snvc_amd.models import submodule as S
    n, c, groups, s = 2, 6, 3, 20
    d = _case(n, c, (n, groups), 5)
    gn = S._f32_coefs(*S._backward_coefs(_t(d["sums"]), _t(d["mean"]), _t(d["var"]), _norm(nn.GroupNorm, groups, c, gamma=d["gamma"]), s)[:3])
    d = _case(n, c, (1, c), 6)
    bn = S._f32_coefs(*S._backward_coefs(_t(d["sums"]), _t(d["mean"]), _t(d["var"]), _norm(nn.BatchNorm3d, c, gamma=d["gamma"]).train(), s)[:3])
    for coefs, shape in ((gn, (n, c)), (bn, (c,))):
        for v in coefs:
            assert v.dtype == torch.float32 and v.is_contiguous() and tuple(v.shape) == shape, (v.dtype, v.shape, shape)
    frozen = _norm(nn.BatchNorm3d, c, gamma=d["gamma"]).eval()
    a, b, cc = S._f32_coefs(*S._backward_coefs(_t(d["sums"]), None, None, frozen, s)[:3])
    assert a.dtype == torch.float32 and a.is_contiguous() and tuple(a.shape) == (c,) and b is None and cc is None
