"""tests/epilogue_ref.py against float64 torch on the CPU: the GPU tests of the epilogue passes (tests/test_gpu_epilogue.py) rest on
that helper, so it is pinned here first.  Reference semantics: nn.BatchNorm3d in train mode / nn.GroupNorm, then ReLU and a residual
added before or after it; gradients by float64 autograd of the same composition."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import epilogue_ref as ER

EPS = float(np.float32(1e-5))
FLAG_SETS = [0, ER.EPI_RELU, ER.EPI_RELU | ER.EPI_ADD_PRE, ER.EPI_ADD_POST, ER.EPI_RELU | ER.EPI_ADD_POST, ER.EPI_ADD_PRE]


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max()
    assert err <= 1e-12 * max(np.abs(b).max(), 1e-300), f"{what}: {err:.3e} of {np.abs(b).max():.3e}"


def _data(n, c, sp, seed):
    r = np.random.default_rng(seed)
    f = lambda a: a.astype(np.float32)
    return dict(x=f(r.standard_normal((n, c) + sp) * 3 + 0.5), res=f(r.standard_normal((n, c) + sp)), gy=f(r.standard_normal((n, c) + sp)),
                gamma=f(r.uniform(0.5, 2, c) * r.choice([-1.0, 1.0], c)), beta=f(r.standard_normal(c)))


def _torch_chain(d, groups, per_sample, flags):
    """y and the gradients of sum(y * gy) by float64 autograd."""
    x, res = (torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("x", "res"))
    gamma, beta = (torch.tensor(d[k], dtype=torch.float64, requires_grad=True) for k in ("gamma", "beta"))
    v = F.group_norm(x, groups, gamma, beta, EPS) if per_sample else F.batch_norm(x, None, None, gamma, beta, True, 0.1, EPS)
    if flags & ER.EPI_ADD_PRE:
        v = v + res
    if flags & ER.EPI_RELU:
        v = F.relu(v)
    if flags & ER.EPI_ADD_POST:
        v = v + res
    (v * torch.tensor(d["gy"], dtype=torch.float64)).sum().backward()
    g = lambda t: np.zeros(d["x"].shape) if t.grad is None else t.grad.numpy()
    return v.detach().numpy(), g(x), g(gamma), g(beta), g(res)


@pytest.mark.parametrize("flags", FLAG_SETS)
@pytest.mark.parametrize("norm", [("bn", 12, False), ("gn", 4, True), ("gn", 1, True), ("gn", 12, True)])
def test_chain_vs_float64_autograd(norm, flags):
    """y, dx, dgamma, dbeta and dresidual of norm -> [+res] -> relu -> [+res] to 1e-12 relative; GroupNorm with cpg = 3, 12 and 1"""
    _, groups, per_sample = norm
    d = _data(3, 12, (2, 3, 6), 11 + flags)
    got = ER.chain_ref(d["x"], d["res"], d["gy"], d["gamma"], d["beta"], groups, per_sample, flags, EPS)
    y, dx, dgamma, dbeta, dres = _torch_chain(d, groups, per_sample, flags)
    _close(got["y"], y, "y")
    _close(got["draw"], dx, "dx")
    _close(got["dgamma"], dgamma, "dgamma")
    _close(got["dbeta"], dbeta, "dbeta")
    _close(got["dres"], dres, "dresidual")


def test_norm_stats_layout_and_defaults():
    """mean / var layouts as ops.norm_stats returns them; gamma = None is 1, beta = None is 0; the biased variance"""
    d = _data(3, 12, (2, 3, 6), 3)
    x = torch.tensor(d["x"], dtype=torch.float64)
    scale, shift, mean, var = ER.norm_stats_ref(d["x"], None, None, 4, True, EPS)
    assert scale.shape == (3, 12) and shift.shape == (3, 12) and mean.shape == (3, 4) and var.shape == (3, 4)
    rows = x.reshape(3, 4, -1)
    _close(mean, rows.mean(2).numpy(), "mean")
    _close(var, rows.var(2, unbiased=False).numpy(), "var")
    _close(ER.affine_act_ref(d["x"], scale, shift, None, 0, True)[0], F.group_norm(x, 4, None, None, EPS).numpy(), "group_norm")
    scale, shift, mean, var = ER.norm_stats_ref(d["x"], None, d["beta"], 12, False, EPS)
    assert scale.shape == (1, 12) and mean.shape == (1, 12)
    _close(var[0], x.transpose(0, 1).reshape(12, -1).var(1, unbiased=False).numpy(), "batch var")
    want = F.batch_norm(x, None, None, None, torch.tensor(d["beta"], dtype=torch.float64), True, 0.1, EPS)
    _close(ER.affine_act_ref(d["x"], scale, shift, None, 0, False)[0], want.numpy(), "batch_norm")


def test_sigmoid_and_magnitude():
    d = _data(2, 6, (1, 4, 5), 5)
    sc, sh = d["gamma"], d["beta"]
    x = torch.tensor(d["x"], dtype=torch.float64, requires_grad=True)
    v = x * torch.tensor(sc, dtype=torch.float64).view(1, -1, 1, 1, 1) + torch.tensor(sh, dtype=torch.float64).view(1, -1, 1, 1, 1)
    y = torch.sigmoid(v)
    (y * torch.tensor(d["gy"], dtype=torch.float64)).sum().backward()
    got, m = ER.affine_act_ref(d["x"], sc, sh, None, ER.EPI_SIGMOID, False)
    _close(got, y.detach().numpy(), "sigmoid")
    g = ER.act_grad_ref(d["x"], d["gy"], None, sc, sh, ER.EPI_SIGMOID, False)
    draw, _ = ER.act_backward_apply_ref(d["x"], g, sc, None, None, False)          # dx = scale * g
    _close(draw, x.grad.numpy(), "sigmoid dx")
    y2, m2 = ER.affine_act_ref(d["x"], sc, sh, d["res"], ER.EPI_RELU | ER.EPI_ADD_POST, False)
    xs = ER.f64(d["x"]) * ER.f64(sc).reshape(1, -1, 1, 1, 1)
    _close(m2, np.abs(xs) + np.abs(ER.f64(sh)).reshape(1, -1, 1, 1, 1) + np.abs(ER.f64(d["res"])) + np.abs(y2), "M")


def test_per_sample_coefficients_are_indexed_by_n_and_c():
    """a value per (n, c): the helper's own indexing against an explicit loop"""
    r = np.random.default_rng(9)
    n, c, sp = 3, 4, (1, 2, 3)
    raw, g = r.standard_normal((n, c) + sp).astype(np.float32), r.standard_normal((n, c) + sp).astype(np.float32)
    a, b, cc = (r.standard_normal((n, c)).astype(np.float32) for _ in range(3))
    draw, _ = ER.act_backward_apply_ref(raw, g, a.reshape(-1), b, cc, True)
    y, _ = ER.affine_act_ref(raw, a, b.reshape(-1), None, 0, True)
    for i in range(n):
        for j in range(c):
            _close(draw[i, j], ER.f64(a[i, j]) * g[i, j] + ER.f64(b[i, j]) * raw[i, j] + ER.f64(cc[i, j]), "draw")
            _close(y[i, j], ER.f64(raw[i, j]) * a[i, j] + ER.f64(b[i, j]), "y")


def test_relu_derivative_is_zero_at_zero_and_edges_are_cleared():
    raw = np.array([[[[[0.0, 1.0, -1.0, 1e-9, 3.0]]]]], dtype=np.float32)
    gy = np.ones_like(raw)
    g = ER.act_grad_ref(raw, gy, None, None, None, ER.EPI_RELU, False)
    assert g.ravel().tolist() == [0.0, 1.0, 0.0, 1.0, 1.0]
    sh = np.array([-1.0], dtype=np.float32)                                   # v = raw - 1: 1.0 sits on the edge, 0.0 does not
    raw2 = np.array([[[[[0.0, 1.0, 1.0 + 2.0 ** -22, 1.0 - 2.0 ** -23, 3.0]]]]], dtype=np.float32)
    assert ER.clear_relu_edges(raw2, None, sh, None, ER.EPI_RELU, False) == 3
    v, _ = ER.preact_ref(raw2, None, sh, None, ER.EPI_RELU, False)[0], None
    y, m = ER.affine_act_ref(raw2, None, sh, None, ER.EPI_RELU, False)
    assert not ER.relu_edge(v, m).any() and raw2[0, 0, 0, 0, 0] == 0.0 and raw2[0, 0, 0, 0, 4] == 3.0
    z = np.zeros((1, 1, 1, 1, 4), dtype=np.float32)                           # the exact-zero block is no edge and stays
    assert ER.clear_relu_edges(z, np.array([2.0], dtype=np.float32), None, z.copy(), ER.EPI_RELU | ER.EPI_ADD_PRE, False) == 0
    assert not z.any()


@pytest.mark.parametrize("count", [1, 2, 50])
def test_bn_track_vs_batchnorm3d(count):
    """two train-mode steps of nn.BatchNorm3d in float64: running statistics and the counter; count == 1 keeps the biased variance"""
    r = np.random.default_rng(count)
    c = 5
    bn = torch.nn.BatchNorm3d(c, momentum=0.1).double().train()
    with torch.no_grad():
        bn.running_mean.copy_(torch.tensor(r.standard_normal(c)))
        bn.running_var.copy_(torch.tensor(r.uniform(0.5, 2, c)))
    rm, rv, nbt = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy(), 0
    for step in range(2):
        x = r.standard_normal((count, c, 1, 1, 1)) * 2 + 1
        if count > 1:
            bn(torch.tensor(x))
        mean, var = x.reshape(count, c).mean(0), x.reshape(count, c).var(0)
        rm, rv, nbt, _ = ER.bn_track_ref(rm, rv, nbt, mean, var, count, 0.1)
        if count > 1:
            _close(rm, bn.running_mean.numpy(), "running_mean")
            _close(rv, bn.running_var.numpy(), "running_var")
            assert nbt == int(bn.num_batches_tracked)
        else:       # torch refuses a single value per channel in train mode: the definition, with the biased variance (0 here)
            assert nbt == step + 1 and np.all(var == 0.0)
    if count == 1:
        _close(rv, bn.running_var.numpy() * 0.9 ** 2, "running_var, count 1")
