"""Every row / chunk form of the first-layer kernels (csrc/sheared_conv.hip) that a small launch reaches, one case each
(tests/first_layer_cases.py).  Each test first asks the library which form its shape takes and which launch numbers it uses
(include/snvc_forms.h) and fails if the case no longer reaches what it is there for; then it runs the op and compares:

  sheared expand          bit for bit with the numpy restatement of ``ops.sheared_expand``'s definition: one float32 add, and with
                          scale / bias float32(float32(x * sc) + bi) -- the two roundings the fused backward's mask recomputes
  its amax words          the maximum over the words is the bit pattern of max|y| of the stored tensor
  its statistics          the float64 mean / variance of the REFERENCE tensor: mean 1e-6, var rtol 1e-6, scale rtol 2e-6, shift 2e-6
  warped expand           the built-volume route (device cost volume, bit-equal to the C oracle, and the fp32 3D convolution over it) at
                          2e-5; the register-window form against the r3 form at 2e-6; and bit for bit against every (n, c) slice run
                          on its own, which runs one row per workgroup -- the form the older tests hold to the oracle
  split producers         the cases of tests/test_gpu_split_format.py at the deeper shapes: host definition of the format, bit for bit
  sheared weight gradient float64 correlation at 1e-5; two calls give equal bits
  adjoint, fused backward the numpy sums of the existing tests: 1e-5 for sums, exact for one-term slots

The ``*_case`` functions are also rows of tests/test_gpu_guard_ops.py and tests/test_gpu_guard_split.py.  References are computed once
per case and never written to.
"""
import functools
import os

import numpy as np
import pytest
import torch

import first_layer_cases as FC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snvc_forms.h")) as _f:
    HEADER = _f.read()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _assert_form(entry, args, form, want):
    """The launcher's decision for these sizes: the form's name and the launch numbers of ``want``."""
    from snvc_amd import _forms
    rc, info, text = _forms.first_layer(entry, *args)
    names = {v: k for k, v in _forms.enum_names(HEADER, "FL").items()}
    assert rc > 0 and names[rc] == form, f"the launcher takes {names.get(rc, rc)} ({text}), the case is there for {form}"
    assert {k: info[k] for k in want} == want, info
    return info


def _same_bits(got, exp, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float32, (what, got.shape, exp.shape, got.dtype)
    bad = np.ascontiguousarray(got).view(np.uint32) != np.ascontiguousarray(exp).view(np.uint32)
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, the first at {i}: got {got[i]!r}, expected {exp[i]!r}")


def _nan(shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------------------------------------------------- sheared expand
@functools.lru_cache(maxsize=None)
def _expand_reference(name):
    c = FC.EXPAND_BY_NAME[name]
    n, ch, h, w, d, q, m0 = c.shape
    g, gcol, planes, scale, bias, (off, wu, off_col, wu_col) = FC.expand_inputs(c.shape, 300 + len(name))
    x = FC.sheared_expand_ref(g, gcol, planes, (n, ch, d, h, w), q, m0, off, off_col)
    return _frozen(g, gcol, planes, scale, bias, x) + ((off, wu, off_col, wu_col),)


def _expand_form(c, entry, flags=0):
    n, ch, h, w, d, q, m0 = c.shape
    off, wu, off_col, wu_col = FC.sheared_geometry(q, m0, d, w)
    base = {FC.SHEARED_EXPAND: "EXPAND_Q", FC.SHEARED_EXPAND_AMAX: "EXPAND_AMAX_Q", FC.SHEARED_EXPAND_STATS: "STATS_Q"}[entry]
    info = _assert_form(entry, (n, ch, d, h, w, q, m0, wu, wu_col, flags), f"{base}{q}", c.info)
    assert h - (info["blocks"] - 1) * info["RB"] == c.last and info["RB"] * (w // 4) == c.active


def sheared_expand_case(name, mode):
    """``plain``: no scale, no bias (and once more without planes): one float32 add.  ``affine``: scale and bias, without and with
    ReLU: two more roundings.  ``amax``: scale and bias, and the words."""
    from snvc_amd import ops
    c = FC.EXPAND_BY_NAME[name]
    n, ch, h, w, d, q, m0 = c.shape
    g, gcol, planes, scale, bias, x, (off, wu, off_col, wu_col) = _expand_reference(name)
    gd, gcd, pd = _dev(g), _dev(gcol), _dev(planes)
    shape = (n, ch, d, h, w)
    if mode == "plain":
        _expand_form(c, FC.SHEARED_EXPAND)
        out = _nan(shape)
        ops.sheared_expand(gd, gcd, pd, None, None, out, q, m0, off, off_col, 0)
        _same_bits(out, x, f"sheared_expand {name}")
        out.fill_(float("nan"))
        ops.sheared_expand(gd, gcd, None, None, None, out, q, m0, off, off_col, 0)
        _same_bits(out, FC.sheared_expand_ref(g, gcol, None, shape, q, m0, off, off_col), f"sheared_expand {name}, no planes")
    elif mode == "affine":
        sd, bd = _dev(scale), _dev(bias)
        for relu in (False, True):
            _expand_form(c, FC.SHEARED_EXPAND, FC.RELU if relu else 0)
            out = _nan(shape)
            ops.sheared_expand(gd, gcd, pd, sd, bd, out, q, m0, off, off_col, ops.EPI_RELU if relu else 0)
            _same_bits(out, FC.affine_ref(x, scale, bias, relu), f"sheared_expand {name}, scale and bias, relu={relu}")
    else:
        _expand_form(c, FC.SHEARED_EXPAND_AMAX)
        out = _nan(shape)
        words = ops.amax_word(torch.device(DEV))
        ops.sheared_expand(gd, gcd, pd, _dev(scale), _dev(bias), out, q, m0, off, off_col, 0, amax=words)
        y = FC.affine_ref(x, scale, bias, False)
        _same_bits(out, y, f"sheared_expand_amax {name}")
        assert words.element_size() == 4
        got = int(words.cpu().numpy().view(np.uint32).max())
        assert got == int(np.abs(y).max().view(np.uint32)), f"amax words hold {got:#x}, max|y| is {int(np.abs(y).max().view(np.uint32)):#x}"


@pytest.mark.parametrize("mode", ["plain", "affine", "amax"])
@pytest.mark.parametrize("name", [c.name for c in FC.EXPAND])
def test_sheared_expand(name, mode):
    sheared_expand_case(name, mode)


def sheared_stats_case(name):
    """snvc_sheared_expand_stats (MODE 1: per-block float64 partials, fewer blocks than rows) against the float64 statistics of the
    reference tensor -- not of the kernel's own expand."""
    from snvc_amd import ops
    c = FC.EXPAND_BY_NAME[name]
    n, ch, h, w, d, q, m0 = c.shape
    g, gcol, planes, _, _, x, (off, wu, off_col, wu_col) = _expand_reference(name)
    _expand_form(c, FC.SHEARED_EXPAND_STATS)
    r = np.random.default_rng(17)
    gamma, beta = r.uniform(0.5, 1.5, ch).astype(np.float32), r.standard_normal(ch).astype(np.float32)
    scale, shift, mean, var = ops.sheared_expand_stats(_dev(g), _dev(gcol), _dev(planes), _dev(gamma), _dev(beta), (n, ch, d, h, w), q, m0, off,
                                                       off_col, 1e-5)
    e_scale, e_shift, e_mean, e_var = FC.stats_ref(x, gamma, beta, 1e-5)
    np.testing.assert_allclose(mean.cpu().numpy()[0], e_mean, rtol=0, atol=1e-6)
    np.testing.assert_allclose(var.cpu().numpy()[0], e_var, rtol=1e-6)
    np.testing.assert_allclose(scale.cpu().numpy()[0], e_scale, rtol=2e-6)
    np.testing.assert_allclose(shift.cpu().numpy()[0], e_shift, rtol=0, atol=2e-6)


@pytest.mark.parametrize("name", [c.name for c in FC.STATS])
def test_sheared_expand_stats(name):
    sheared_stats_case(name)


# -------------------------------------------------------------------------------------------------------------- warped expand
WARPED_CIN = 8


@functools.lru_cache(maxsize=None)
def _warped_inputs(name):
    c = {k.name: k for k in FC.WARPED}[name]
    n, ch, h, w, d = c.shape
    r = np.random.default_rng(400 + len(name))
    right = r.standard_normal((n, WARPED_CIN, h, w)).astype(np.float32)
    weight = (0.1 * r.standard_normal((ch, WARPED_CIN, 3, 3, 3))).astype(np.float32)
    planes = r.standard_normal((n, ch, 3, h, w)).astype(np.float32)
    return _frozen(right, weight, planes, FC.warped_shifts(n, d, w))


def warped_expand_case(name):
    """P, Q, E as the model forms them (three depth-1 layers on the right feature), then snvc_warped_expand in both forms."""
    from snvc_amd import ops
    from snvc_amd.models.stereo_volume import GlobalStack
    from test_gpu_parity import TIGHT, check
    c = {k.name: k for k in FC.WARPED}[name]
    n, ch, h, w, d = c.shape
    right, weight, planes, shift = _warped_inputs(name)
    for flags, form in ((0, "WARPED_WIN"), (FC.R3, "WARPED_R3")):
        info = _assert_form(FC.WARPED_EXPAND, (n, ch, d, h, w, 1, 0, 1, 1, flags), form, c.info)
        assert h - (info["blocks"] - 1) * info["RB"] == c.last and info["RB"] * (w // 4) == c.active
    assert _assert_form(FC.WARPED_EXPAND, (1, 1, d, h, w), "WARPED_WIN", dict(RB=1, blocks=h))
    rd, wd, pld, shd = _dev(right), _dev(weight), _dev(planes), _dev(shift)
    mk = lambda t: ops.Conv3dLayer(t.contiguous(), 3, 1, 1, 1, False, planar=True)      # noqa: E731
    lp, lq, le = (mk(t) for t in GlobalStack._commuted_weights(wd))
    r5 = rd.unsqueeze(2)
    p_, q_, e_ = lp(r5).squeeze(2), lq(r5).squeeze(2), le(rd[:, :, :, :4].contiguous().unsqueeze(2)).squeeze(2)
    win, r3 = _nan((n, ch, d, h, w)), _nan((n, ch, d, h, w))
    ops.warped_expand(p_, q_, e_, pld, shd, None, None, win, 0)
    ops.warped_expand(p_, q_, e_, pld, shd, None, None, r3, ops.WARPED_EXPAND_R3)
    built = ops.Conv3dLayer(wd, 3, 1, 1, 1, False)(ops.cost_volume_forward_right(rd, shd), None, None, None, 0, None, depth_planes=pld)
    check(win.cpu().numpy(), built.cpu().numpy(), TIGHT, f"warped_expand {name} vs the built volume")
    check(r3.cpu().numpy(), built.cpu().numpy(), TIGHT, f"warped_expand {name}, r3 form, vs the built volume")
    check(win.cpu().numpy(), r3.cpu().numpy(), 2e-6, f"warped_expand {name}, register-window form vs r3 form")
    # every (n, c) slice on its own: one row per workgroup, the same bits
    ps = p_.view(n, 3, ch, h, w).transpose(1, 2).contiguous()                  # [N, C, 3, H, W]
    qs = q_.view(n, 3, ch, h, w).transpose(1, 2).contiguous()
    es = e_.view(n, 9, ch, h, 4).transpose(1, 2).contiguous()                  # [N, C, 9, H, 4]
    alone = _nan((n, ch, d, h, w))
    for ni in range(n):
        for ci in range(ch):
            ops.warped_expand(ps[ni, ci].unsqueeze(0), qs[ni, ci].unsqueeze(0), es[ni, ci].unsqueeze(0), pld[ni:ni + 1, ci:ci + 1], shd[ni:ni + 1],
                              None, None, alone[ni:ni + 1, ci:ci + 1], 0)
    assert torch.equal(alone, win), f"warped_expand {name}: RB = {c.info['RB']} differs from the slices run one row per workgroup"


@pytest.mark.parametrize("name", [c.name for c in FC.WARPED])
def test_warped_expand(name):
    warped_expand_case(name)


# ------------------------------------------------------------------------------------------------------------ split producers
def _split_forms(name, q):
    _, (n, c, h, w, d), sheared, warped = FC.SPLIT_BY_NAME[name]
    grid = lambda g: dict(chunks=g[0], per_chunk=g[1], grid_x=h, grid_yz=(c + 7) // 8 * g[0] * n)      # noqa: E731
    return (n, c, h, w, d), grid(sheared), grid(warped)


def sheared_expand_split_case(name, q):
    """tests/test_gpu_split_format.sheared_expand_split_case at a deeper shape: NaN-filled output, EPI_STREAM_OUT on and off."""
    import test_gpu_split_format as SPLIT
    shape, sheared, _ = _split_forms(name, q)
    n, c, h, w, d = shape
    g, gcol = SPLIT.sheared_inputs(q, True, "none", shape)[:2]
    for flags in (FC.RELU, FC.RELU | FC.STREAM_OUT):
        _assert_form(FC.SHEARED_EXPAND_SPLIT, (n, c, d, h, w, q, 3, g.shape[3], gcol.shape[3], flags), f"SPLIT_Q{q}", sheared)
    SPLIT.sheared_expand_split_case(q, True, shape=shape)


SHEARED_SPLIT = [(s[0], q) for s in FC.SPLIT for q in FC.SPLIT_SHEARED_Q.get(s[0], (2,))]


@pytest.mark.parametrize("name,q", SHEARED_SPLIT, ids=[f"{n}-q{q}" for n, q in SHEARED_SPLIT])
def test_sheared_expand_split(name, q):
    sheared_expand_split_case(name, q)


def warped_expand_split_case(name):
    import test_gpu_split_format as SPLIT
    shape, _, warped = _split_forms(name, 0)
    n, c, h, w, d = shape
    for flags in (FC.RELU, FC.RELU | FC.STREAM_OUT):
        _assert_form(FC.WARPED_EXPAND_SPLIT, (n, c, d, h, w, 1, 0, 1, 1, flags), "WARPED_SPLIT", warped)
    SPLIT.warped_expand_split_case(True, shape=shape)


@pytest.mark.parametrize("name", [s[0] for s in FC.SPLIT])
def test_warped_expand_split(name):
    warped_expand_split_case(name)


# ------------------------------------------------------------------------------------------------------------ weight gradient
@functools.lru_cache(maxsize=None)
def _wgrad_reference(name, cin):
    wu, = {c.name: c for c in FC.WGRAD}[name].shape
    r = np.random.default_rng(500 + wu + cin)
    x = r.standard_normal((FC.WGRAD_N, cin, FC.WGRAD_H, wu)).astype(np.float32)
    gy = r.standard_normal((FC.WGRAD_N, FC.WGRAD_CO, FC.WGRAD_H, wu)).astype(np.float32)
    return _frozen(x, gy, FC.wgrad_ref(x, gy).astype(np.float32))


def sheared_wgrad_case(name, cin):
    """The 3 x 7 weight gradient with one and with two column chunks (the seam sits inside the 7-tap halo; the second chunk ends on a
    short 64-column tile) against the float64 correlation at the existing test's 1e-5; two calls give equal bits."""
    from snvc_amd import _forms, ops
    from test_gpu_parity import check
    c = {k.name: k for k in FC.WGRAD}[name]
    wu, = c.shape
    rc, info, text = _forms.sheared_wgrad(FC.WGRAD_N, cin, FC.WGRAD_CO, FC.WGRAD_H, wu)
    assert rc > 0 and {k: info[k] for k in c.info} == c.info, (rc, info, text)
    assert wu - (info["chunks"] - 1) * info["per_chunk"] == c.last
    x, gy, exp = _wgrad_reference(name, cin)
    xd, gd = _dev(x), _dev(gy)
    dk = ops.sheared_wgrad(xd, gd)
    again = ops.sheared_wgrad(xd, gd)
    assert torch.equal(dk, again), "two calls of snvc_sheared_wgrad differ"
    err = np.abs(dk.cpu().numpy().astype(np.float64) - exp).max() / np.abs(exp).max()
    print(f"sheared_wgrad {name} C={cin}: max error / max|ref| = {err:.3e}")
    check(dk.cpu().numpy(), exp, 1e-5, f"dK {name} C={cin}")


@pytest.mark.parametrize("cin", FC.WGRAD_C)
@pytest.mark.parametrize("name", [c.name for c in FC.WGRAD])
def test_sheared_wgrad(name, cin):
    sheared_wgrad_case(name, cin)


# -------------------------------------------------------------------------------------------------------------------- adjoint
def sheared_reduce_case(name):
    """More slots than the workgroup has threads: the second trip of the kernel's strided loops."""
    from snvc_amd import ops
    from test_gpu_parity import check
    c = {k.name: k for k in FC.REDUCE}[name]
    n, ch, d, h, w, q = c.shape
    m0 = FC.REDUCE_M0
    off, wu, off_col, wu_col = FC.sheared_geometry(q, m0, d, w)
    info = _assert_form(FC.SHEARED_REDUCE, (n, ch, d, h, w, q, m0, wu, wu_col), f"REDUCE_Q{q}", c.info)
    assert ((wu + q - 1) // q, wu_col) == FC.REDUCE_SLOTS[name] and max(FC.REDUCE_SLOTS[name]) > info["threads"]
    dy = np.random.default_rng(600 + d).standard_normal((n, ch, d, h, w)).astype(np.float32)
    dg, dgc = ops.sheared_reduce(_dev(dy), q, m0, wu, off, wu_col, off_col)
    line, last, terms = FC.line_sums(dy.astype(np.float64), q, m0, wu, off, wu_col, off_col)
    got = dg.cpu().numpy().reshape(line.shape)
    check(got, line.astype(np.float32), 1e-5, f"dG {name}")
    one = terms <= 1                                          # [3, wu]: slots with a single term (or none) are exact
    assert one.any() and (terms > 1).any()
    assert np.array_equal(got.transpose(0, 2, 3, 1, 4)[..., one], line.astype(np.float32).transpose(0, 2, 3, 1, 4)[..., one])
    check(dgc.cpu().numpy().reshape(last.shape), last.astype(np.float32), 0, f"dG' {name}")


@pytest.mark.parametrize("name", [c.name for c in FC.REDUCE])
def test_sheared_reduce(name):
    sheared_reduce_case(name)


# ------------------------------------------------------------------------------------------------------------- fused backward
def sheared_backward_case(name):
    """snvc_sheared_backward_reduce with all 64 lanes of a row at work (W = 512: what leaves lane 63 is final) and with one (W = 8);
    H = 5: a last block of one row.  The mask is that of float32(float32(x * scale) + shift) of the reference tensor."""
    from snvc_amd import ops
    from test_gpu_parity import check
    c = {k.name: k for k in FC.BACKWARD}[name]
    n, ch, d, h, w, q = c.shape
    m0 = q + 1
    shape = (n, ch, h, w, d, q, m0)
    g, gcol, planes, _, _, (off, wu, off_col, wu_col) = FC.expand_inputs(shape, 700 + w + q)
    info = _assert_form(FC.SHEARED_BACKWARD_REDUCE, (n, ch, d, h, w, q, m0, wu, wu_col), f"BWD_Q{q}", c.info)
    assert h - (info["blocks"] - 1) * info["RB"] == c.last
    x = FC.sheared_expand_ref(g, gcol, planes, (n, ch, d, h, w), q, m0, off, off_col)
    r = np.random.default_rng(701)
    gamma, beta = r.uniform(0.5, 1.5, ch).astype(np.float32), r.standard_normal(ch).astype(np.float32)
    scale, shift = (a.astype(np.float32) for a in FC.stats_ref(x, gamma, beta, 1e-5)[:2])
    gy = r.standard_normal((n, ch, d, h, w)).astype(np.float32)
    line, colsum, lastc, sums = ops.sheared_backward_reduce(_dev(g), _dev(gcol), _dev(planes), _dev(scale[None]), _dev(shift[None]), _dev(gy), q, m0,
                                                            off, off_col)
    v = FC.affine_ref(x, scale, shift, False)
    gm, raw = np.where(v > 0, gy, 0).astype(np.float64), x.astype(np.float64)
    exp_sums = np.stack([gm.sum((2, 3, 4)), (gm * raw).sum((2, 3, 4))], -1)
    np.testing.assert_allclose(sums.cpu().numpy(), exp_sums, rtol=2e-6, atol=2e-5)
    e_line, e_last, e_col = [], [], []
    for src in (gm, raw):
        a, b, _ = FC.line_sums(src, q, m0, wu, off, wu_col, off_col)
        e_line.append(a); e_last.append(b); e_col.append(FC.class_sums(src))
    e_line, e_last, e_col = np.stack(e_line), np.stack(e_last), np.stack(e_col)
    check(line.cpu().numpy().reshape(e_line.shape), e_line.astype(np.float32), 1e-5, f"line sums {name}")
    check(lastc.cpu().numpy().reshape(e_last.shape), e_last.astype(np.float32), 0, f"last-column slots {name}")
    check(colsum.cpu().numpy(), e_col.astype(np.float32), 1e-5, f"depth-class sums {name}")


@pytest.mark.parametrize("name", [c.name for c in FC.BACKWARD])
def test_sheared_backward_reduce(name):
    sheared_backward_case(name)
