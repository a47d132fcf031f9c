"""Every launcher form of the geometry ops on the device, one small case each (tests/geometry_cases.py; DESIGN.md section 4.4.1 lists
which case pins which form).  Each test first asks the library -- on the device, with the alignment of the tensors it is about to
pass -- which form the launcher takes and which launch numbers it uses, and fails if the case no longer reaches the form it is there
for; then it runs the op through the public wrappers and compares:

  cost volume        bit for bit with the C oracle (oracle/cost_volume_ref.c)
  gather, forward    bit for bit with the numpy restatement of ATen's grid_sampler (oracle/numpy_ref.py); half outputs with that
                     result rounded to half, split pairs with hi = half(v * mul), lo = half(v * mul - hi) computed in float32
  gather, backward   float64 autograd through F.grid_sample on the CPU: 2e-5 * max|ref| for the sorted form (and the same bits from
                     two calls), 2e-4 * max|ref| for the two float-atomics forms

Every reference is computed once per case (the guard-band suite runs these functions again) and never written to.
"""
import functools
import os

import numpy as np
import pytest
import torch

import geometry_cases as GC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snvc_forms.h")) as _f:
    HEADER = _f.read()


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _assert_form(c, *read):
    """The launcher's decision for this case on this device, with the alignment of the tensors the test passes (``read``).  What the
    wrappers allocate -- outputs, workspaces -- comes from torch's allocator, 256-byte aligned, and is taken as aligned here;
    ``_host`` checks that of every forward output once it is back, so that the query and the launch cannot disagree unseen."""
    from snvc_amd import _forms
    aligned = _forms.ALIGNED_OUT | (_forms.ALIGNED_IN if all(t.data_ptr() % 16 == 0 for t in read) else 0)
    rc, info, text = GC.query(c, aligned)
    names = {v: k for k, v in _forms.enum_names(HEADER, GC.ENUM_PREFIX[c.entry]).items()}
    if c.form is None:
        assert rc == -c.refusal[0] and text.startswith(c.refusal[1]), (rc, text)
        return
    assert rc > 0 and names[rc] == c.form, f"{c.name}: the launcher takes {names.get(rc, rc)} ({text}), the case is there for {c.form}"
    assert {k: info[k] for k in c.info} == c.info, (c.name, info)


def _host(t: torch.Tensor) -> np.ndarray:
    """The output on the host, after the check that it was 16-byte aligned as ``_assert_form`` told the query."""
    host = t.cpu().numpy()
    assert t.data_ptr() % 16 == 0, "the wrapper returned an output that is not 16-byte aligned: the form asserted above was asked for another alignment"
    return host


def _same_bits(got: np.ndarray, exp: np.ndarray):
    """Equal bit for bit, with NaN equal to NaN whatever its payload (signed zeros are told apart)."""
    assert got.shape == exp.shape and got.dtype == exp.dtype, (got.shape, exp.shape, got.dtype, exp.dtype)
    nan_g, nan_e = np.isnan(got), np.isnan(exp)
    word = {2: np.uint16, 4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    bad = (nan_g != nan_e) | (~nan_e & (got.view(word) != exp.view(word)))
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} elements differ, the first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} for {exp[tuple(np.argwhere(bad)[0])]!r}"


# -------------------------------------------------------------------------------------------------------------- cost volume
@functools.lru_cache(maxsize=None)
def _cv_forward_case(c):
    from oracle import native as O
    left, right, shift = GC.cv_forward_inputs(c)
    exp = O.cost_volume_forward(left, right, shift, c.shape[5])
    for a in (left, right, shift, exp):
        a.setflags(write=False)
    return left, right, shift, exp


@functools.lru_cache(maxsize=None)
def _cv_backward_case(c):
    from oracle import native as O
    g, shift = GC.cv_backward_inputs(c)
    e_left, e_right = O.cost_volume_backward(g, shift, c.shape[5])
    for a in (g, shift, e_left, e_right):
        a.setflags(write=False)
    return g, shift, e_left, e_right


@pytest.mark.parametrize("c", GC.BY_ENTRY["cv_fwd"], ids=str)
def test_cost_volume_forward(c):
    from snvc_amd import _lib, ops
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    left, right, shift, exp = _cv_forward_case(c)
    ch, ds = c.shape[1], c.shape[5]
    d_left, d_right, d_shift = _dev(left.copy()), _dev(right.copy()), _dev(shift.copy())
    _assert_form(c, d_left, d_right)
    if c.form is None:
        with pytest.raises(_lib.Unsupported, match=c.refusal[1].split(":")[0]):
            ops.cost_volume_forward_right(d_right, d_shift)
        return
    if c.right:
        _same_bits(_host(ops.cost_volume_forward_right(d_right, d_shift)), np.ascontiguousarray(exp[:, ch:]))
    else:
        _same_bits(_host(build_cost_volume(d_left, d_right, d_shift, ds)), exp)


@pytest.mark.parametrize("c", GC.BY_ENTRY["cv_bwd"], ids=str)
def test_cost_volume_backward(c):
    from snvc_amd import _lib, ops
    g, shift, e_left, e_right = _cv_backward_case(c)
    ch, ds = c.shape[1], c.shape[5]
    d_shift = _dev(shift.copy())
    _assert_form(c)
    if c.form is None:
        with pytest.raises(_lib.Unsupported, match=c.refusal[1].split(":")[0]):
            ops.cost_volume_backward_right(_dev(g[:, ch:].copy()), d_shift)
        return
    if c.right:
        _same_bits(ops.cost_volume_backward_right(_dev(g[:, ch:].copy()), d_shift).cpu().numpy(), e_right)
    else:
        g_left, g_right = ops.cost_volume_backward(_dev(g.copy()), d_shift, ds)
        _same_bits(g_left.cpu().numpy(), e_left)
        _same_bits(g_right.cpu().numpy(), e_right)


# ------------------------------------------------------------------------------------------------------------ gather, forward
@functools.lru_cache(maxsize=None)
def _gather_forward_case(key):
    """Inputs and the oracle's fp32 result; rows that differ only in the output kind share them."""
    from oracle import numpy_ref as NR
    c = next(x for x in GC.BY_ENTRY["gather_fwd"] if (x.shape, x.res, x.inf_pixel) == key)
    lf, rf, l_pts, r_pts = GC.gather_forward_inputs(c)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        exp = NR.sample_2d_feat(lf, rf, l_pts, r_pts, c.res)
    for a in (lf, rf, l_pts, r_pts, exp):
        a.setflags(write=False)
    return lf, rf, l_pts, r_pts, exp


@pytest.mark.parametrize("c", GC.BY_ENTRY["gather_fwd"], ids=str)
def test_voxel_gather_forward(c):
    from snvc_amd import _lib, ops
    lf, rf, l_pts, r_pts, exp = _gather_forward_case((c.shape, c.res, c.inf_pixel))
    d_lf, d_rf, d_lp, d_rp = (_dev(a.copy()) for a in (lf, rf, l_pts, r_pts))
    _assert_form(c, d_lp, d_rp)
    if c.kind == "f32":
        _same_bits(_host(ops.voxel_gather_forward(d_lf, d_rf, d_lp, d_rp, c.res)), exp)
    elif c.kind == "c8":
        with np.errstate(over="ignore"):
            exp_h = GC.to_c8(exp.astype(np.float16))
        _same_bits(_host(ops.voxel_gather_forward_f16(d_lf, d_rf, d_lp, d_rp, c.res)), exp_h)
    else:
        mul_dev = ops.split_scale_for(d_lf, d_rf)
        if c.form is None:
            with pytest.raises(_lib.Unsupported, match=c.refusal[1].split(":")[0]):
                ops.voxel_gather_forward_split(d_lf, d_rf, d_lp, d_rp, c.res, mul_dev)
            return
        pair = _host(ops.voxel_gather_forward_split(d_lf, d_rf, d_lp, d_rp, c.res, mul_dev))     # [N, 2, 2F/8, V, 8]
        mul = float(mul_dev.item())
        if c.inf_pixel:
            assert mul == 1.0                                         # the scale of a non-finite map
        else:
            assert mul >= 1024.0 and np.log2(mul) % 1 == 0, mul      # max|feature| of a few units lands in [2^13, 2^14)
        hi, lo = GC.split_pair(exp, mul)
        _same_bits(np.ascontiguousarray(pair[:, 0]), GC.to_c8(hi))
        _same_bits(np.ascontiguousarray(pair[:, 1]), GC.to_c8(lo))


# ----------------------------------------------------------------------------------------------------------- gather, backward
@functools.lru_cache(maxsize=None)
def _gather_backward_case(c):
    """Inputs, the float64 reference, and torch's own float32 CPU autograd measured against it: the scale of fp32 summation at
    this depth."""
    g, l_pts, r_pts = GC.gather_backward_inputs(c)
    ref = GC.grid_sample_grads(c, g, l_pts, r_pts, torch.float64)
    cpu32 = GC.grid_sample_grads(c, g, l_pts, r_pts, torch.float32)
    err32 = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(cpu32, ref)]
    for a in (g, l_pts, r_pts, *ref):
        a.setflags(write=False)
    return g, l_pts, r_pts, ref, err32


@pytest.mark.parametrize("c", GC.BY_ENTRY["gather_bwd"], ids=str)
def test_voxel_gather_backward(c):
    """Error relative to max|ref| against float64 autograd, with torch's float32 CPU autograd on the same inputs next to it (printed).
    Measured on an MI355X, left / right map: global atomics 1.2e-5 / 4.9e-6 (float32 CPU: the same), LDS atomics over two chunks
    2.4e-6 / 1.5e-6 (CPU 2.5e-6 / 1.5e-6), sorted 1.1e-6 / 9.9e-7 (CPU 1.7e-6 / 1.5e-6): the project's bounds hold with room, at
    the large V too, and the error is that of the float32 coordinate normalisation rather than of the summation."""
    from snvc_amd import ops
    g, l_pts, r_pts, ref, err32 = _gather_backward_case(c)
    n, f, hf, wf, _ = c.shape
    d_g, d_lp, d_rp = _dev(g.copy()), _dev(l_pts.copy()), _dev(r_pts.copy())
    _assert_form(c)
    if c.det:
        got = ops.voxel_gather_backward(d_g, d_lp, d_rp, (n, f, hf, wf), c.res)
        again = ops.voxel_gather_backward(d_g, d_lp, d_rp, (n, f, hf, wf), c.res)
        assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])           # no atomics: the same bits every time
    else:
        got = ops.voxel_gather_backward(d_g, d_lp, d_rp, (n, f, hf, wf), c.res, deterministic=False)
    tol = 2e-5 if c.det else 2e-4
    errs = []
    for side in range(2):
        out = got[side].cpu().numpy()
        assert np.isfinite(out).all() and np.abs(ref[side]).max() > 1.0
        errs.append(float(np.abs(out.astype(np.float64) - ref[side]).max() / np.abs(ref[side]).max()))
    print(f"{c.name}: |HIP - float64| / max|ref| = {errs[0]:.3e}, {errs[1]:.3e} (bound {tol:.0e}); float32 CPU autograd: "
          f"{err32[0]:.3e}, {err32[1]:.3e}")
    assert max(errs) <= tol, (c.name, errs, err32)
