"""GPU parity: the HIP path (through the C ABI in libsnvc_hip.so) against the CPU oracle and the
golden vectors generated from the imported reference.  Run with ``pytest -m gpu`` on an MI355X.

Tolerance: BASELINE.json's north_star asks for 1e-3 relative fp32.  `check` applies it twice -- on
max|err| / max|ref| and ELEMENT BY ELEMENT (|err| <= 1e-3*|ref| + 1e-3*rms(ref) for >= 99.99 % of
the elements, see `elementwise_tail`) -- and additionally bounds the much tighter error the
exact-fp32 MFMA path actually achieves.  Integer outputs are bit-exact.
"""
import numpy as np
import pytest
import torch

import golden_cases as GC

pytestmark = pytest.mark.gpu

REL = 1e-3          # contract (north_star)
TIGHT = 2e-5        # what an exact-fp32 FMA chain in a different summation order should meet
WINO7 = 3e-4        # Winograd F(4,7) (k7 layers): transform constants up to 52.5 amplify fp32 rounding; still 3x inside REL


def dev():
    return torch.device("cuda:0")


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def elementwise_tail(a, b, rel=REL):
    """north_star's "1e-3 relative", element by element: an element passes when
    |err| <= rel*|ref| + rel*rms(ref) (the rms term is the absolute floor for elements near zero,
    where a pure ratio is meaningless after ReLU / cancellation).  Returns (fraction failing, worst
    |err| / (rel*|ref| + rel*rms))."""
    a = np.asarray(a, dtype=np.float64).ravel()
    b = np.asarray(b, dtype=np.float64).ravel()
    rms = np.sqrt(np.mean(b * b)) if b.size else 0.0
    bound = rel * np.abs(b) + rel * max(rms, 1e-30)
    ratio = np.abs(a - b) / bound
    return float((ratio > 1.0).mean()) if b.size else 0.0, float(ratio.max()) if b.size else 0.0


def check(a, b, tol=TIGHT, what=""):
    """Three criteria: (1) the contract on the max-normalised error, (2) the tighter bound the exact-fp32
    path is expected to meet, (3) the ELEMENTWISE contract: at most 0.01 % of the elements may miss
    1e-3*|ref| + 1e-3*rms(ref), and none by more than 10x."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    e = rel_err(a, b)
    assert e <= REL, f"{what}: rel err {e:.3e} breaks the 1e-3 contract"
    assert e <= tol, f"{what}: rel err {e:.3e} above the expected {tol:.1e}"
    frac, worst = elementwise_tail(a, b)
    assert frac <= 1e-4 and worst <= 10.0, f"{what}: elementwise 1e-3 criterion: {100 * frac:.4f} % of elements outside, worst {worst:.2f}x"


def require_form(module, x_shape, want, residual=False, exact=False):
    """Asks the dispatcher which kernel form the convolution of ``module`` (a convbn_3d or its conv) takes for a dense, allocator-aligned
    input of ``x_shape`` under the conv_variant bits in force (snvc_conv3d_forward_form, include/snvc_forms.h), and requires ``want``:
    a test written for one form fails when its shapes stop reaching it, instead of passing on the direct kernel."""
    import math
    import os
    from snvc_amd import _forms, _lib, ops
    from snvc_amd.models.submodule import _get_layer, _Plan
    conv = module[0] if hasattr(module, "__getitem__") else module
    layer = _get_layer(conv, _Plan())
    n, in_sp = x_shape[0], tuple(x_shape[2:])
    out_sz = layer.cout * math.prod(layer.out_spatial(in_sp))
    flags = (_lib.EPI_RELU | _lib.EPI_ADD_PRE) if residual else 0
    d = layer._desc(n, in_sp, flags, ops._algo(exact), layer.cin * math.prod(in_sp), out_sz, out_sz if residual else 0)
    rc, _, text = _forms.conv3d_forward(d, _forms.ENTRY_FORWARD, 16, 16, 16 if residual else 0, 0, 0)
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snvc_forms.h")) as f:
        names = {v: k for k, v in _forms.enum_names(f.read(), "CF").items()}
    assert rc > 0 and names[rc] == want, f"the dispatcher takes {names.get(rc, rc)} ({text}) for {tuple(x_shape)}, the test is written for {want}"


@pytest.fixture(scope="module")
def G():
    return GC.load_golden()


def seeded(mod, seed):
    from oracle import torch_ref as T
    mod.load_state_dict(T.seeded_state_dict(mod, seed), strict=True)
    return mod.eval()


# =============================================================================== C ABI smoke
def test_library_loads_and_reports_errors():
    from snvc_amd import _lib
    L = _lib.lib()
    assert L.snvc_abi_version() == 6
    rc = L.snvc_cost_volume_forward(None, None, None, None, 1, 1, 3, 4, 1, 2, 0, None)
    assert rc == 1 and b"multiples of downsample" in L.snvc_last_error_string()


def test_cpu_tensors_are_rejected():
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    z = torch.zeros(1, 1, 2, 2)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        build_cost_volume(z, z, torch.zeros(1, 1), 1)


# =============================================================================== a1 / a2
CV_CASES = [
    # N, C, H, W, D, ds, dtype
    (2, 3, 5, 8, 4, 1, np.float32),      # vector path (W % 4 == 0)
    (1, 2, 4, 13, 5, 1, np.float32),     # scalar path, odd W
    (1, 2, 6, 12, 3, 2, np.float32),     # downsample 2
    (1, 2, 6, 9, 3, 3, np.float32),      # downsample 3
    (2, 2, 4, 16, 6, 1, np.float64),     # double
    (1, 4, 12, 40, 9, 1, np.float32),
]


def _cv_inputs(N, C, H, W, D, dtype, seed):
    r = np.random.default_rng(seed)
    L = r.standard_normal((N, C, H, W)).astype(dtype)
    R = r.standard_normal((N, C, H, W)).astype(dtype)
    s = (r.random((N, D)) * (W + 2)).astype(dtype)
    s[0, 0] = 0.0
    if D > 1:
        s[0, 1] = 2.0          # integer shift: exact copy, lx == 0 -> tap 2 gated in backward
    if D > 2:
        s[0, 2] = W + 5.0      # everything gated out
    return L, R, s


@pytest.mark.parametrize("N,C,H,W,D,ds,dtype", CV_CASES)
def test_cost_volume_forward_bit_exact(N, C, H, W, D, ds, dtype):
    from oracle import native as O
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    L, R, s = _cv_inputs(N, C, H, W, D, dtype, 5)
    exp = O.cost_volume_forward(L, R, s, ds)
    got = build_cost_volume(torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()),
                            torch.from_numpy(s).to(dev()), ds).cpu().numpy()
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(got, exp), f"max diff {np.abs(got - exp).max()}"


@pytest.mark.parametrize("N,C,H,W,D,ds,dtype", CV_CASES)
def test_cost_volume_backward_bit_exact(N, C, H, W, D, ds, dtype):
    from oracle import native as O
    from snvc_amd.extension.build_cost_volume import build_cost_volume_cuda
    _, _, s = _cv_inputs(N, C, H, W, D, dtype, 6)
    g = np.random.default_rng(7).standard_normal((N, 2 * C, D, H // ds, W // ds)).astype(dtype)
    eL, eR = O.cost_volume_backward(g, s, ds)
    gL, gR = build_cost_volume_cuda.build_cost_volume_backward(torch.from_numpy(g).to(dev()),
                                                               torch.from_numpy(s).to(dev()), ds)
    assert np.array_equal(gL.cpu().numpy(), eL), np.abs(gL.cpu().numpy() - eL).max()
    assert np.array_equal(gR.cpu().numpy(), eR), np.abs(gR.cpu().numpy() - eR).max()


def test_cost_volume_backward_any_shift_matches_the_oracle():
    """The C-ABI backward entry points take any shift array (the `shift >= 0` assert lives in the Python wrapper of the
    forward only, reference __init__.py:12): negative, fractional-negative, huge and NaN shifts through the fp32 / ds = 1
    two-candidate kernel give the oracle's bits (that kernel used to assume shift >= 0)."""
    from oracle import native as O
    from snvc_amd import ops
    r = np.random.default_rng(77)
    N, C, H, W, D = 2, 3, 4, 16, 10
    g = r.standard_normal((N, 2 * C, D, H, W)).astype(np.float32)
    s = r.uniform(-6, 6, (N, D)).astype(np.float32)
    s[0, :6] = [-0.5, -1.0, -2.75, -30.0, 1e9, -1e9]
    s[1, 0] = np.nan
    eL, eR = O.cost_volume_backward(g, s, 1)
    gL, gR = ops.cost_volume_backward(torch.from_numpy(g).to(dev()), torch.from_numpy(s).to(dev()), 1)
    assert np.array_equal(gL.cpu().numpy(), eL) and np.array_equal(gR.cpu().numpy(), eR, equal_nan=True)
    gR2 = ops.cost_volume_backward_right(torch.from_numpy(g[:, C:].copy()).to(dev()), torch.from_numpy(s).to(dev()))
    assert np.array_equal(gR2.cpu().numpy(), eR, equal_nan=True)


def test_cost_volume_known_answers():
    """The hand-derived KATs of tests/test_oracle_cost_volume.py, straight on the HIP kernel."""
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    R = torch.tensor([10., 20., 30., 40.], device=dev()).view(1, 1, 1, 4)
    out = build_cost_volume(torch.zeros_like(R), R, torch.tensor([[1.5]], device=dev()), 1)
    assert out[0, 1, 0, 0].tolist() == [0.0, 0.0, 15.0, 25.0]
    R = (torch.arange(7, dtype=torch.float32, device=dev()) + 1).view(1, 1, 1, 7)
    for k in (0, 1, 3, 6, 9):
        out = build_cost_volume(R, R, torch.tensor([[float(k)]], device=dev()), 1)[0, 1, 0, 0]
        exp = torch.zeros(7, device=dev())
        if k < 7:
            exp[k:] = R[0, 0, 0, :7 - k]
        assert torch.equal(out, exp)


def test_cost_volume_autograd_and_errors():
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    r = np.random.default_rng(3)
    L = torch.from_numpy(r.standard_normal((1, 2, 3, 8))).to(dev()).requires_grad_()
    R = torch.from_numpy(r.standard_normal((1, 2, 3, 8))).to(dev()).requires_grad_()
    s = torch.tensor([[0.0, 1.25, 3.0]], dtype=torch.float64, device=dev())
    out = build_cost_volume(L, R, s, 1)
    g = torch.from_numpy(r.standard_normal(tuple(out.shape))).to(dev())
    out.backward(g)
    # adjoint identity in fp64: <fwd(x), g> == <x, bwd(g)> (the op is linear in L and R)
    lhs = (out.detach() * g).sum().item()
    rhs = (L.detach() * L.grad).sum().item() + (R.detach() * R.grad).sum().item()
    assert abs(lhs - rhs) < 1e-9 * max(1.0, abs(lhs))
    with pytest.raises(AssertionError):
        build_cost_volume(L.detach(), R.detach(), -torch.ones_like(s), 1)      # reference __init__.py:12
    with pytest.raises(RuntimeError, match="match their size"):
        build_cost_volume(L.detach(), R.detach()[..., :4], s, 1)
    with pytest.raises(RuntimeError, match="same batch"):
        build_cost_volume(L.detach(), R.detach(), s.repeat(2, 1), 1)
    empty = build_cost_volume(L.detach()[:0], R.detach()[:0], s[:0], 1)
    assert empty.shape == (0, 4, 3, 3, 8)


# =============================================================================== a3
@pytest.mark.parametrize("name", list(GC.TRUNK_CASES))
def test_voxel_gather_vs_golden(name, G):
    from snvc_amd import ops
    grid, gn, n, fh, fw, seed = GC.TRUNK_CASES[name]
    lf, rf, gpl, gpr = GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1)
    keep = gpl.clone()
    d_gpl = gpl.to(dev())
    vox = ops.voxel_gather_forward(lf.to(dev()), rf.to(dev()), d_gpl, gpr.to(dev()), GC.RESOLUTION)
    assert torch.equal(d_gpl.cpu(), keep)   # coordinates are not modified
    vox = vox.view(n, 64, *grid).cpu()
    check(vox[:, ::7, ::3, ::5, ::5].numpy(), G[f"trunk/{name}/voxel_sub"], 1e-6, "voxel_sub")
    s = G[f"trunk/{name}/voxel_sum"]
    assert abs(vox.double().sum().item() - s[0]) <= 1e-6 * s[1]


def test_voxel_gather_vs_torch_ref_edge_cases():
    from oracle import torch_ref as T
    from snvc_amd import ops
    r = np.random.default_rng(9)
    n, f, hf, wf, grid = 2, 5, 7, 9, (2, 3, 5)     # odd sizes, F not a multiple of anything
    v = grid[0] * grid[1] * grid[2]
    lf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32))
    rf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32))
    res = (28, 36)                                   # non-square crop: x uses res[1], y uses res[0]
    pts = r.uniform(-10, 46, (n, 2, v)).astype(np.float32)
    pts[0, 0, :4] = [0.0, 36.0, -2.0, 1e9]           # exact borders, far outside
    pts[0, 1, :4] = [0.0, 28.0, 14.0, 3.0]
    pts[1, 0, 0] = np.nan
    gl, gr = torch.from_numpy(pts), torch.from_numpy(pts[:, :, ::-1].copy())
    exp = T.sample_2d_feat(lf, rf, gl, gr, res, grid).reshape(n, 2 * f, v)
    got = ops.voxel_gather_forward(lf.to(dev()), rf.to(dev()), gl.to(dev()), gr.to(dev()), res).cpu()
    # Non-finite coordinates (NaN, 1e9): pinned to the oracle (oracle/numpy_ref.py, the restatement of ATen's CPU
    # arithmetic): no tap is in range, the four weights are NaN, 0 * NaN = NaN -> the voxel's channels are NaN on
    # that camera's half and finite on the other; the 1e9 coordinate gives finite weights times zero taps = 0.
    from oracle import numpy_ref as NR
    exp_np = NR.sample_2d_feat(lf.numpy(), rf.numpy(), gl.numpy(), gr.numpy(), res)
    assert np.array_equal(got.numpy(), exp_np, equal_nan=True)
    assert np.isnan(got.numpy()[1, :f, 0]).all() and np.isfinite(got.numpy()[1, f:, 0]).all()
    assert (got.numpy()[0, :f, 3] == 0).all()
    # and against torch's grid_sample wherever torch is finite
    m = torch.isfinite(exp) & torch.isfinite(got)
    assert m.float().mean() > 0.98
    check(got[m].numpy(), exp[m].numpy(), 1e-6, "gather edge cases")


def test_voxel_gather_bit_exact_vs_numpy_oracle():
    from oracle import numpy_ref as NR
    from snvc_amd import ops
    grid, gn, n, fh, fw, seed = GC.TRUNK_CASES["G1"]
    lf, rf, gpl, gpr = GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1)
    exp = NR.sample_2d_feat(lf.numpy(), rf.numpy(), gpl.numpy(), gpr.numpy(), GC.RESOLUTION)
    got = ops.voxel_gather_forward(lf.to(dev()), rf.to(dev()), gpl.to(dev()), gpr.to(dev()), GC.RESOLUTION).cpu().numpy()
    assert np.array_equal(got, exp), np.abs(got - exp).max()


@pytest.mark.parametrize("res", [(28, 36), (64, 128), (256, 256)])
def test_voxel_gather_lds_path_bit_exact_with_edge_coordinates(res):
    """The LDS-staged kernel (V >= 4096, whole 16-byte rows) on both forms of the coordinate normalisation -- the
    division (crop sizes that are not powers of two) and its reciprocal-multiply twin (powers of two) -- with exact
    borders, far-outside, infinite and NaN coordinates (out-of-range taps read the zero slot), fp32 and C8-half
    outputs: bit-identical to the numpy oracle (and to its result rounded to half)."""
    from oracle import numpy_ref as NR
    from snvc_amd import ops
    r = np.random.default_rng(19)
    n, f, hf, wf, v = 2, 16, 9, 11, 8192
    lf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32))
    rf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32))
    lf[0, :, 0, 0] = np.inf                     # the pixel the select form used to park out-of-range taps on
    pts = np.stack([r.uniform(-0.2 * res[1], 1.2 * res[1], (n, v)), r.uniform(-0.2 * res[0], 1.2 * res[0], (n, v))], 1).astype(np.float32)
    pts[0, 0, :8] = [0.0, res[1], -2.0, 1e9, np.inf, -np.inf, np.nan, 0.5 * res[1]]
    pts[0, 1, :8] = [0.0, res[0], 0.5 * res[0], 3.0, 1.0, 2.0, 3.0, np.nan]
    pts[1, :, 100:200] = 1e-41                  # subnormal coordinates: x / 2^k and x * 2^-k round alike
    gl, gr = torch.from_numpy(pts), torch.from_numpy(pts[:, :, ::-1].copy())
    exp = NR.sample_2d_feat(lf.numpy(), rf.numpy(), gl.numpy(), gr.numpy(), res)
    dl, dr, dgl, dgr = lf.to(dev()), rf.to(dev()), gl.to(dev()), gr.to(dev())
    got = ops.voxel_gather_forward(dl, dr, dgl, dgr, res).cpu().numpy()
    assert np.array_equal(got, exp, equal_nan=True)
    half = ops.voxel_gather_forward_f16(dl, dr, dgl, dgr, res)          # [N, 2F/8, V, 8]
    exp_h = torch.from_numpy(exp).half().reshape(n, 2 * f // 8, 8, v).permute(0, 1, 3, 2)
    assert torch.equal(torch.nan_to_num(half.cpu().float(), nan=7.0), torch.nan_to_num(exp_h.float(), nan=7.0))


def test_voxel_gather_backward_adjoint():
    from snvc_amd import ops
    r = np.random.default_rng(10)
    n, f, hf, wf, v = 1, 3, 6, 6, 200
    lf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32)).to(dev())
    rf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32)).to(dev())
    gl = torch.from_numpy(r.uniform(-2, 26, (n, 2, v)).astype(np.float32)).to(dev())
    gr = torch.from_numpy(r.uniform(-2, 26, (n, 2, v)).astype(np.float32)).to(dev())
    out = ops.voxel_gather_forward(lf, rf, gl, gr, (24, 24))
    g = torch.from_numpy(r.standard_normal(tuple(out.shape)).astype(np.float32)).to(dev())
    dl, dr = ops.voxel_gather_backward(g, gl, gr, (n, f, hf, wf), (24, 24))
    lhs = (out.double() * g.double()).sum().item()
    rhs = (lf.double() * dl.double()).sum().item() + (rf.double() * dr.double()).sum().item()
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs))


@pytest.mark.parametrize("case", ["uniform", "coherent", "edges"])
def test_voxel_gather_backward_deterministic(case):
    """The sorted, atomics-free adjoint: equals torch autograd through F.grid_sample, equals the atomics form up to
    summation order, and is BIT-IDENTICAL run to run -- also when every voxel lands on a handful of pixels (the
    case that took the atomics form 77 ms) and with out-of-range / NaN coordinates."""
    import torch.nn.functional as F
    from snvc_amd import ops
    r = np.random.default_rng({"uniform": 1, "coherent": 2, "edges": 3}[case])
    n, f, hf, wf, v, res = 2, 32, 16, 16, 6000, (64, 64)
    if case == "edges":
        n, f, hf, wf, v, res = 1, 5, 7, 9, 333, (28, 36)
    lf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32))
    rf = torch.from_numpy(r.standard_normal((n, f, hf, wf)).astype(np.float32))
    if case == "coherent":      # a short line: thousands of voxels per pixel
        t = np.linspace(0, 1, v, dtype=np.float32)
        pts = np.stack([np.stack([20 + 6 * t, 30 + 2 * t])] * n)
    else:
        pts = r.uniform(-0.1 * res[1], 1.1 * res[1], (n, 2, v)).astype(np.float32)
    if case == "edges":
        pts[0, 0, :5] = [0.0, res[1], -3.0, 1e9, np.nan]
        pts[0, 1, :5] = [0.0, res[0], 14.0, 3.0, 5.0]
    gl = torch.from_numpy(pts.astype(np.float32))
    gr = torch.from_numpy(pts[:, :, ::-1].copy().astype(np.float32))
    g = torch.from_numpy(r.standard_normal((n, 2 * f, v)).astype(np.float32))
    dgl, dgr, dg = gl.to(dev()), gr.to(dev()), g.to(dev())
    a = ops.voxel_gather_backward(dg, dgl, dgr, (n, f, hf, wf), res)
    b = ops.voxel_gather_backward(dg, dgl, dgr, (n, f, hf, wf), res)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])                       # run-to-run bit identity
    c = ops.voxel_gather_backward(dg, dgl, dgr, (n, f, hf, wf), res, deterministic=False)
    # torch autograd (NaN coordinates give no gradient in both: weights are dropped with their voxel)
    finite = torch.isfinite(gl).all(dim=1) & torch.isfinite(gr).all(dim=1)           # [n, v]
    for side, (feat, p) in enumerate(((lf, gl), (rf, gr))):
        x = feat.clone().requires_grad_()
        pn = torch.nan_to_num(p, nan=-1e6)
        grid = torch.stack([pn[:, 0] / res[1] * 2 - 1, pn[:, 1] / res[0] * 2 - 1], dim=-1).view(n, 1, v, 2)
        out = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, :, 0]   # [n, f, v]
        (out * g[:, side * f:(side + 1) * f]).sum().backward()
        ref = x.grad
        scale = max(ref.abs().max().item(), 1.0)
        assert (a[side].cpu() - ref).abs().max().item() <= 2e-5 * scale, (case, side)
        assert (c[side].cpu() - ref).abs().max().item() <= 2e-4 * scale, (case, side)


def test_grid_projection_vs_oracle_and_golden(G):
    """a11: grid points -> camera frame -> P2/P3 -> crop affine, on the device, against the numpy
    restatement (itself bit-equal to the reference's methods, make_golden.py) and the golden samples."""
    import types
    from oracle import numpy_ref as NR
    from snvc_amd.geometry import GridProjector
    gp = GC.grid_proj_case()
    cfg = types.SimpleNamespace(x_range=gp["x_range"], y_range=gp["y_range"], z_range=gp["z_range"],
                                grid_resolution=gp["grid"])
    proj = GridProjector(cfg)
    cl, cr, g3 = proj.generate(gp["samples"], gp["P_left"], gp["P_right"], gp["trans_l"], gp["trans_r"], dev(),
                               with_grid_3d=True)
    el, er, eg = NR.grid_projection(gp["samples"], gp["P_left"], gp["P_right"], gp["trans_l"], gp["trans_r"],
                                    NR.init_3d_grid(gp["x_range"], gp["y_range"], gp["z_range"], gp["grid"]))
    cl, cr, g3 = cl.cpu().numpy(), cr.cpu().numpy(), g3.cpu().numpy()
    assert cl.dtype == np.float32 and cl.shape == el.shape == (3, 2, 16 * 32 * 48)
    # fp64 pipeline rounded to fp32 once: equal except where the fp64 value sits on a float32 tie
    for got, exp in ((cl, el), (cr, er)):
        np.testing.assert_allclose(got, exp, rtol=0, atol=2e-4)      # pixels
        assert (got == exp).mean() > 0.9999
    np.testing.assert_allclose(g3, eg, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(cl[:, :, ::37], G["gridproj/left_sub"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(cr[:, :, ::37], G["gridproj/right_sub"], rtol=0, atol=2e-4)
    np.testing.assert_allclose(g3[:, ::97], G["gridproj/grid3d_sub"], rtol=1e-13, atol=1e-13)
    # and it plugs straight into the gather (same tensors the dataset would have produced)
    from snvc_amd import ops
    lf = torch.randn(3, 8, 16, 16, device=dev())
    a = ops.voxel_gather_forward(lf, lf, torch.from_numpy(cl).to(dev()), torch.from_numpy(cr).to(dev()), (64, 64))
    b = ops.voxel_gather_forward(lf, lf, torch.from_numpy(el).to(dev()), torch.from_numpy(er).to(dev()), (64, 64))
    assert (a - b).abs().max().item() < 1e-3


# =============================================================================== a4
@pytest.mark.parametrize("name", list(GC.CONV_CASES))
def test_convbn_3d_vs_golden(name, G):
    from snvc_amd.models import submodule as S
    cin, cout, k, s, p, dil, gn, shape, seed = GC.CONV_CASES[name]
    m = seeded(S.convbn_3d(cin, cout, k, s, p, dilation=dil, gn=gn), seed).to(dev())
    with torch.no_grad():
        y = m(GC.randn((1, cin) + shape, seed + 1).to(dev())).cpu().numpy()
    # k7 runs on Winograd F(4,7): fp32 products and sums, but the transforms amplify rounding to ~1e-4
    check(y, G[f"conv/{name}"], WINO7 if k == 7 else TIGHT, name)


@pytest.mark.parametrize("k,dil", [(5, 1), (5, 2), (7, 1)])
@pytest.mark.parametrize("W", [24, 36, 44])
def test_k5_k7_winograd_vs_torch(k, dil, W):
    """The local model's 5x5x5 / 7x7x7 layers: Winograd F(4,5) / F(4,7) along W (and the polyphase form
    for dilation 2) against torch's fp32 convolution, with tile-ragged sizes, two channel groups, a
    residual epilogue; and the same layer forced onto the direct kernel (desc.algo = SNVC_ALGO_DIRECT)."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(50 + k + W)
    pad = dil * (k - 1) // 2
    tol = WINO7 if k == 7 else TIGHT
    for cin, cout, shape in ((32, 32, (6, 7, W)), (6, 64, (5, 9, W))):
        m = seeded(S.convbn_3d(cin, cout, k, 1, pad, dilation=dil), 60 + cin)
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        with torch.no_grad():
            ref = F.batch_norm(F.conv3d(x, m[0].weight, None, 1, pad, dil), m[1].running_mean, m[1].running_var,
                               m[1].weight, m[1].bias, False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
            m = m.to(dev())
            wino = {(5, 1): "WINO_K5", (5, 2): "WINO_K5D2", (7, 1): "WINO_K7"}[(k, dil)]
            direct = {(5, 1): "K5M", (5, 2): "K5D2M", (7, 1): "K7M"}[(k, dil)] + ("2" if cout > 32 else "1")
            require_form(m, x.shape, wino)
            require_form(m, x.shape, wino, residual=True)
            require_form(m, x.shape, direct, exact=True)
            check(m(x.to(dev())).cpu().numpy(), ref.numpy(), tol, f"k{k} d{dil} W={W} conv+bn")
            y = m.fused(x.to(dev()), relu=True, residual=res.to(dev()))
            check(y.cpu().numpy(), F.relu(ref + res).numpy(), tol, f"k{k} d{dil} W={W} relu(conv+res)")
            from snvc_amd.models.submodule import _get_layer, _Plan, _folded_bn
            plan = _Plan()
            layer = _get_layer(m[0], plan)
            sc, bi = _folded_bn(m[1], plan)
            y = layer(x.to(dev()), sc, bi, None, 0, None, exact=True)
            check(y.cpu().numpy(), ref.numpy(), TIGHT, f"k{k} d{dil} W={W} direct kernel")


@pytest.mark.parametrize("form", ["slice_pipelined", "per_chunk"])
@pytest.mark.parametrize("W", [40, 72, 44])
def test_k3_stride2_winograd_vs_torch(W, form):
    """Stride-2 3x3x3 layers: the polyphase + F(4,2) kernels (output width % 4 == 0) -- the default slice-pipelined
    refill (counted vmcnt waits) and the per-chunk refill form (SNVC_ALGO_WINO_TILE_STD) -- and the direct kernel
    (everything else, and desc.algo = SNVC_ALGO_DIRECT) against torch, batch 2, two channel groups, ragged tiles,
    odd channel counts (a half-empty last chunk), one and many chunks."""
    import torch.nn.functional as F
    from snvc_amd import _lib, ops
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(70 + W)
    bits = _lib.ALGO_WINO_TILE_STD if form == "per_chunk" else 0
    for cin, cout, shape in ((32, 64, (10, 6, W)), (7, 32, (4, 8, W)), (2, 32, (18, 10, W)), (64, 64, (6, 20, W))):
        m = seeded(S.convbn_3d(cin, cout, 3, 2, 1), 80 + cin)
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        with torch.no_grad(), ops.conv_variant(bits):
            ref = F.batch_norm(F.conv3d(x, m[0].weight, None, 2, 1), m[1].running_mean, m[1].running_var,
                               m[1].weight, m[1].bias, False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
            m = m.to(dev())
            rows16 = (W // 2) % 4 == 0          # output rows of 20 and 36 against rows of 22
            want = {("slice_pipelined", True): "WINO_S2_PIPE4", ("slice_pipelined", False): "WINO_S2_PIPE2",
                    ("per_chunk", True): "WINO_S2", ("per_chunk", False): "WINO_S2_V8"}[(form, rows16)]
            require_form(m, x.shape, want)
            require_form(m, x.shape, want, residual=True)
            check(m(x.to(dev())).cpu().numpy(), ref.numpy(), TIGHT, f"s2 W={W} conv+bn")
            y = m.fused(x.to(dev()), relu=True, residual=res.to(dev()))
            check(y.cpu().numpy(), F.relu(ref + res).numpy(), TIGHT, f"s2 W={W} relu(conv+res)")
            from snvc_amd import _lib, ops
            with ops.conv_variant(_lib.ALGO_DIRECT):
                require_form(m, x.shape, "K3S2M2" if cout > 32 else "K3S2M1")
                check(m(x.to(dev())).cpu().numpy(), ref.numpy(), TIGHT, f"s2 W={W} direct")
            with ops.conv_variant(_lib.ALGO_DIRECT | _lib.ALGO_GENERIC_EPILOGUE):
                require_form(m, x.shape, "K3S2M2" if cout > 32 else "K3S2M1")
                check(m(x.to(dev())).cpu().numpy(), ref.numpy(), TIGHT, f"s2 W={W} direct, generic epilogue")


def test_conv3d_epilogue_variants_and_slices():
    """relu / sigmoid / residual-before / residual-after, batch > 1, channel-sliced in/out,
    Cout not a multiple of 32 (27 and 1), Cin not a multiple of the staging chunk."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(21)
    x = torch.from_numpy(r.standard_normal((2, 6, 5, 6, 37)).astype(np.float32))
    for cout, k, pad, dil in ((27, 1, 0, 1), (1, 3, 1, 1), (40, 3, 1, 1), (33, 5, 4, 2)):
        conv = S.HipConv3d(6, cout, k, 1, pad, dilation=dil, bias=False)
        w = torch.from_numpy((r.standard_normal(tuple(conv.weight.shape)) * 0.1).astype(np.float32))
        conv.weight.data.copy_(w)
        conv = conv.to(dev())
        ref = F.conv3d(x, w, None, 1, pad, dil)
        res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
        with torch.no_grad():
            check(conv(x.to(dev())).cpu().numpy(), ref.numpy(), TIGHT, f"plain cout={cout}")
            y = conv.fused(x.to(dev()), relu=True, residual=res.to(dev()))
            check(y.cpu().numpy(), F.relu(ref + res).numpy(), TIGHT, "relu(conv+res)")
            y = conv.fused(x.to(dev()), relu=True, residual=res.to(dev()), residual_after_act=True)
            check(y.cpu().numpy(), (F.relu(ref) + res).numpy(), TIGHT, "relu(conv)+res")
            y = conv.fused(x.to(dev()), sigmoid=True)
            check(y.cpu().numpy(), torch.sigmoid(ref).numpy(), TIGHT, "sigmoid")
            # channel-sliced input and output (the in-place torch.cat of vernier.py:433)
            big_in = torch.zeros(2, 9, 5, 6, 37, device=dev())
            big_in[:, 2:8] = x.to(dev())
            big_out = torch.full((2, cout + 3,) + tuple(ref.shape[2:]), 7.0, device=dev())
            conv.fused(big_in[:, 2:8], out=big_out[:, 1:1 + cout])
            check(big_out[:, 1:1 + cout].cpu().numpy(), ref.numpy(), TIGHT, "sliced io")
            assert torch.all(big_out[:, 0] == 7.0) and torch.all(big_out[:, 1 + cout:] == 7.0)


@pytest.mark.parametrize("mode", ["default", "big", "std", "narrow", "direct"])
@pytest.mark.parametrize("W", [72, 78, 156])
def test_k3_kernel_variants_vs_torch(mode, W):
    """Every 3x3x3 / stride-1 kernel the dispatcher can pick -- Winograd F(4,3) with the 2x4x64
    register-staged tile, the 4x4x64 LDS-DMA tile, the 4x4x32 tile, their 8-byte-row versions
    (W % 4 == 2) and the direct kernel -- against torch's fp32 convolution, with the fused epilogue
    forms (BN affine + residual before / after ReLU) and tile-ragged D and H."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    from snvc_amd import _lib, ops
    bits = {"default": 0, "big": _lib.ALGO_WINO_TILE_BIG, "std": _lib.ALGO_WINO_TILE_STD,
            "narrow": _lib.ALGO_WINO_TILE_NARROW_REG, "direct": _lib.ALGO_DIRECT}[mode]
    r = np.random.default_rng(31 + W)
    for cin, cout, shape in ((32, 32, (5, 7, W)), (6, 64, (2, 9, W))):
        m = seeded(S.convbn_3d(cin, cout, 3, 1, 1), 40 + cin)
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        with torch.no_grad(), ops.conv_variant(bits):
            ref = F.batch_norm(F.conv3d(x, m[0].weight, None, 1, 1), m[1].running_mean, m[1].running_var,
                               m[1].weight, m[1].bias, False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
            m = m.to(dev())
            rows16 = W % 4 == 0                 # 72 and 156 against 78: the 8-byte-row twins
            want = {"default": "WINO_N3" if rows16 else "WINO_N8", "big": "WINO_BIG" if rows16 else "WINO_N8",
                    "std": "WINO" if rows16 else "WINO8", "narrow": "WINO_N" if rows16 else "WINO_N8",
                    "direct": "K3M2" if cout > 32 else "K3M1"}[mode]
            require_form(m, x.shape, want)
            require_form(m, x.shape, want, residual=True)
            check(m(x.to(dev())).cpu().numpy(), ref.numpy(), TIGHT, f"{mode} W={W} conv+bn")
            y = m.fused(x.to(dev()), relu=True, residual=res.to(dev()))
            check(y.cpu().numpy(), F.relu(ref + res).numpy(), TIGHT, f"{mode} W={W} relu(conv+res)")
            y = m.fused(x.to(dev()), relu=True, residual=res.to(dev()), residual_after_act=True)
            check(y.cpu().numpy(), (F.relu(ref) + res).numpy(), TIGHT, f"{mode} W={W} relu(conv)+res")


def test_deconv_vs_torch():
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(22)
    for cin, cout, shape in ((64, 64, (2, 3, 5)), (64, 32, (3, 4, 33)), (8, 5, (1, 1, 1))):
        m = S._deconvbn_3d(cin, cout, gn=False)
        seeded(m, 23)
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        with torch.no_grad():
            ref = F.batch_norm(F.conv_transpose3d(x, m[0].weight, None, 2, 1, 1), m[1].running_mean, m[1].running_var,
                               m[1].weight, m[1].bias, False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
            m = m.to(dev())
            check(m(x.to(dev())).cpu().numpy(), ref.numpy(), TIGHT, "deconv")
            y = m.fused(x.to(dev()), relu=True, residual=res.to(dev()))
            check(y.cpu().numpy(), F.relu(ref + res).numpy(), TIGHT, "relu(deconv+res)")


def test_conv_kernels_randomised_shapes():
    """Seeded sweep over layer kinds x ragged sizes x epilogue forms, every case against torch's fp32
    convolution: catches tile-edge, batch-stride and dispatch mistakes that fixed shapes miss."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(2026)
    kinds = [("k3", 3, 1, 1), ("k3s2", 3, 2, 1), ("k5", 5, 1, 1), ("k5d2", 5, 1, 2), ("k7", 7, 1, 1), ("deconv", 3, 2, 1), ("k1", 1, 1, 1)]
    import os
    for case in range(int(os.environ.get("SNVC_FUZZ_CASES", "42"))):
        name, k, stride, dil = kinds[case % len(kinds)]
        cin = int(r.choice([3, 8, 32, 33, 64]))
        cout = int(r.choice([32, 64, 32, 27, 1]))
        n = int(r.choice([1, 2]))
        if name == "deconv":
            shape = (int(r.integers(1, 5)), int(r.integers(1, 6)), int(r.choice([3, 6, 16, 34, 39])))
            m = S._deconvbn_3d(cin, cout, gn=False)
            ref_conv = lambda x, w: F.conv_transpose3d(x, w, None, 2, 1, 1)
        else:
            lo = 2 if stride == 2 else 1
            shape = (int(r.integers(lo, 9)), int(r.integers(lo, 11)), int(r.choice([4, 8, 12, 20, 36, 37, 42, 70])))
            pad = dil * (k - 1) // 2
            m = S.convbn_3d(cin, cout, k, stride, pad, dilation=dil)
            ref_conv = lambda x, w, s_=stride, p_=pad, d_=dil: F.conv3d(x, w, None, s_, p_, d_)
        seeded(m, 300 + case)
        x = torch.from_numpy(r.standard_normal((n, cin) + shape).astype(np.float32))
        mode = int(r.integers(0, 3))      # 0: bn, 1: relu(bn + res), 2: relu(bn) + res
        with torch.no_grad():
            ref = F.batch_norm(ref_conv(x, m[0].weight), m[1].running_mean, m[1].running_var, m[1].weight, m[1].bias,
                               False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(ref.shape)).astype(np.float32))
            exp = ref if mode == 0 else (F.relu(ref + res) if mode == 1 else F.relu(ref) + res)
            m = m.to(dev())
            xd, rd = x.to(dev()), res.to(dev())
            got = m(xd) if mode == 0 else m.fused(xd, relu=True, residual=rd, residual_after_act=(mode == 2))
        check(got.cpu().numpy(), exp.numpy(), WINO7 if k == 7 else TIGHT,
              f"case {case}: {name} {cin}->{cout} n={n} {shape} mode {mode}")


def test_deconv_fused_head_vs_separate_layers():
    """snvc_conv3d_forward_head: bn(deconv(x)) + residual projected to one channel inside the epilogue
    equals the two layers run one after the other (torch reference), and the fused path is really taken."""
    import torch.nn.functional as F
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(91)
    m = seeded(S._deconvbn_3d(64, 32, gn=False), 92)
    head = S.HipConv3d(32, 1, kernel_size=1, padding=0, stride=1, bias=False)
    head.weight.data.copy_(torch.from_numpy(r.standard_normal((1, 32, 1, 1, 1)).astype(np.float32)))
    hw_cpu = head.weight.detach().clone()
    wt_cpu, bn_cpu = m[0].weight.detach().clone(), [t.detach().clone() for t in (m[1].running_mean, m[1].running_var, m[1].weight, m[1].bias)]
    for shape in ((3, 5, 34), (4, 4, 8)):
        x = torch.from_numpy(r.standard_normal((2, 64) + shape).astype(np.float32))
        with torch.no_grad():
            y = F.batch_norm(F.conv_transpose3d(x, wt_cpu, None, 2, 1, 1), bn_cpu[0], bn_cpu[1], bn_cpu[2], bn_cpu[3],
                             False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(y.shape)).astype(np.float32))
            ref = F.conv3d(y + res, hw_cpu)
            md, hd = m.to(dev()), head.to(dev())
            plan = S._Plan()
            layer = S._get_layer(md[0], plan)
            sc, bi = S._folded_bn(md[1], plan)
            fused = ops.conv3d_forward_head(layer, x.to(dev()), sc, bi, res.to(dev()), ops.EPI_ADD_PRE, hd.weight)
            assert fused is not None, "the fused-head path must be taken for a 64->32 transposed layer"
            check(fused.cpu().numpy(), ref.numpy(), TIGHT, f"fused head {shape}")
            # with an activation between the layer and the head the in-epilogue projection is what fused_conv3d takes
            got = md.fused(x.to(dev()), relu=True, residual=res.to(dev()), head=hd)
            check(got.cpu().numpy(), F.conv3d(F.relu(y + res), hw_cpu).numpy(), TIGHT, f"fused_conv3d(relu, head=) {shape}")
            # a layer that does not qualify for it (64 output channels) silently runs the two layers separately
            m64 = seeded(S._deconvbn_3d(64, 64, gn=False), 93).to(dev())
            h64 = S.HipConv3d(64, 1, kernel_size=1, padding=0, stride=1, bias=False).to(dev())
            a = m64.fused(x.to(dev()), relu=True, head=h64)
            b = h64(m64.fused(x.to(dev()), relu=True))
            assert torch.equal(a, b)


def test_deconv_to_one_channel_vs_torch():
    """ConvTranspose3d(Cin, 1, k3, s2, p1, op1): the VALU kernel of conv3d_small.hip (rows of whole 16-byte pieces) and
    the MFMA kernel it falls back to, with every epilogue form, against torch."""
    import torch.nn.functional as F
    from snvc_amd import ops
    r = np.random.default_rng(191)
    for cin, shape in ((64, (3, 5, 36)), (5, (1, 1, 4)), (32, (4, 3, 156)), (16, (2, 3, 34)), (7, (2, 2, 5))):
        w = torch.from_numpy(r.standard_normal((cin, 1, 3, 3, 3)).astype(np.float32))
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        sc, bi = torch.tensor([1.7]), torch.tensor([-0.3])
        with torch.no_grad():
            raw = F.conv_transpose3d(x, w, None, 2, 1, 1)
            res = torch.from_numpy(r.standard_normal(tuple(raw.shape)).astype(np.float32))
            layer = ops.Conv3dLayer(w.to(dev()), 3, 2, 1, 1, True)
            xd, rd = x.to(dev()), res.to(dev())
            check(layer(xd).cpu().numpy(), raw.numpy(), TIGHT, f"deconv->1 {cin} {shape}")
            y = layer(xd, sc.to(dev()), bi.to(dev()), rd, ops.EPI_ADD_PRE | ops.EPI_RELU)
            check(y.cpu().numpy(), F.relu(raw * 1.7 - 0.3 + res).numpy(), TIGHT, f"relu(deconv->1 + res) {cin} {shape}")
            y = layer(xd, sc.to(dev()), bi.to(dev()), rd, ops.EPI_ADD_POST | ops.EPI_SIGMOID)
            check(y.cpu().numpy(), (torch.sigmoid(raw * 1.7 - 0.3) + res).numpy(), TIGHT, f"sigmoid(deconv->1) + res {cin} {shape}")
            # a batch-strided input (channel slice of a larger buffer)
            big = torch.from_numpy(r.standard_normal((2, cin + 3) + shape).astype(np.float32)).to(dev())
            ref2 = F.conv_transpose3d(big[:, 3:].cpu(), w, None, 2, 1, 1)
            check(layer(big[:, 3:]).cpu().numpy(), ref2.numpy(), TIGHT, f"deconv->1 slice {cin} {shape}")


def test_folded_head_tail_vs_separate_layers():
    """No activation between a layer with frozen statistics and a 1x1x1 head: fused_conv3d folds the pair into one
    layer to ONE channel (head(bn(conv(x)) + res) = conv'(x) + b' + head(res)).  Transposed (the hourglass tail) and
    plain layers, with and without a residual, with head(res) handed in; the route counter proves the path."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(291)
    for kind, cin, cout, shape in (("deconv", 64, 32, (3, 5, 36)), ("deconv", 64, 64, (2, 3, 34)), ("k3", 32, 32, (4, 6, 40)),
                                   ("k1", 16, 32, (3, 4, 8))):
        m = S._deconvbn_3d(cin, cout, gn=False) if kind == "deconv" else S.convbn_3d(cin, cout, 3 if kind == "k3" else 1, 1,
                                                                                      1 if kind == "k3" else 0)
        seeded(m, 292)
        head = S.HipConv3d(cout, 1, kernel_size=1, padding=0, stride=1, bias=False)
        head.weight.data.copy_(torch.from_numpy(r.standard_normal((1, cout, 1, 1, 1)).astype(np.float32)))
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        with torch.no_grad():
            conv = (F.conv_transpose3d(x, m[0].weight, None, 2, 1, 1) if kind == "deconv"
                    else F.conv3d(x, m[0].weight, None, 1, 1 if kind == "k3" else 0))
            y = F.batch_norm(conv, m[1].running_mean, m[1].running_var, m[1].weight, m[1].bias, False, 0.0, m[1].eps)
            res = torch.from_numpy(r.standard_normal(tuple(y.shape)).astype(np.float32))
            ref0, ref1 = F.conv3d(y, head.weight), F.conv3d(y + res, head.weight)
            md, hd, xd, rd = m.to(dev()), head.to(dev()), x.to(dev()), res.to(dev())
            before = S._ROUTES["folded_head"]
            check(md.fused(xd, head=hd).cpu().numpy(), ref0.numpy(), TIGHT, f"folded {kind} {cin}->{cout}")
            check(md.fused(xd, residual=rd, head=hd).cpu().numpy(), ref1.numpy(), TIGHT, f"folded {kind} {cin}->{cout} + res")
            check(md.fused(xd, residual=rd, head=hd, head_residual=hd(rd)).cpu().numpy(), ref1.numpy(), TIGHT,
                  f"folded {kind} {cin}->{cout} + given head(res)")
            assert S._ROUTES["folded_head"] == before + 3
            # parameters change -> the folded layer is rebuilt
            hd.weight.mul_(0.5)
            check(md.fused(xd, residual=rd, head=hd).cpu().numpy(), 0.5 * ref1.numpy(), TIGHT, "folded head after an update")
            # BatchNorm's parameters replaced by new ones whose version counters hold the same values -> rebuilt as well
            nw, nb = md[1].weight.detach() * 2.0 + 0.25, md[1].bias.detach() - 0.5
            for new, old in ((nw, md[1].weight), (nb, md[1].bias)):
                while new._version < old._version:
                    new.add_(0.0)
                assert new._version == old._version
            md[1].weight, md[1].bias = torch.nn.Parameter(nw), torch.nn.Parameter(nb)
            y2 = F.batch_norm(conv, md[1].running_mean.cpu(), md[1].running_var.cpu(), nw.cpu(), nb.cpu(), False, 0.0, md[1].eps)
            check(md.fused(xd, residual=rd, head=hd).cpu().numpy(), F.conv3d(y2 + res, hd.weight.cpu()).numpy(), TIGHT,
                  "folded head after a BatchNorm parameter swap")


def test_conv_avgpool_d4_fused_vs_separate():
    """SNVC_EPI_AVGPOOL_D4: conv4 + AvgPool3d((4,1,1)) of the local trunk (vernier.py:289,435-436) in one launch against
    torch; layers that do not qualify (W % 4 != 0, D % 4 != 0, GroupNorm) pool in a launch of their own."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(491)
    for cin, cout, shape, fused in ((64, 32, (8, 6, 40), True), (32, 64, (4, 9, 156), True), (64, 32, (12, 5, 36), True),
                                    (64, 32, (8, 6, 38), False), (64, 32, (6, 6, 40), False)):
        m = seeded(S.convbn_3d(cin, cout, 3, 1, 1), 492).to(dev())
        x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32))
        with torch.no_grad():
            ref = F.relu(F.batch_norm(F.conv3d(x, m[0].weight.cpu(), None, 1, 1), m[1].running_mean.cpu(), m[1].running_var.cpu(),
                                      m[1].weight.cpu(), m[1].bias.cpu(), False, 0.0, m[1].eps))
            if shape[0] % 4:
                ref = ref[:, :, :shape[0] // 4 * 4]
            exp = F.avg_pool3d(ref, (4, 1, 1), (4, 1, 1))
            b_f, b_s = S._ROUTES["conv_avgpool_fused"], S._ROUTES["conv_avgpool_separate"]
            got = S.fused_conv3d_avgpool_d4(m[0], m[1], x.to(dev()), relu=True)
            assert (S._ROUTES["conv_avgpool_fused"], S._ROUTES["conv_avgpool_separate"]) == ((b_f + 1, b_s) if fused else (b_f, b_s + 1))
        check(got.cpu().numpy(), exp.numpy(), TIGHT, f"conv + avgpool {cin}->{cout} {shape}")


def test_side_head_vs_separate_projection():
    """snvc_conv3d_forward_side_head: y is bit-identical to the plain launch and y_head = head(y); layers that do not
    qualify get the projection from a launch of their own."""
    import torch.nn.functional as F
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(391)
    head = S.HipConv3d(32, 1, kernel_size=1, padding=0, stride=1, bias=False)
    head.weight.data.copy_(torch.from_numpy(r.standard_normal((1, 32, 1, 1, 1)).astype(np.float32)))
    m = S.ConvBNReLU3d(seeded(S.convbn_3d(32, 32, 3, 1, 1), 392), torch.nn.ReLU(inplace=True)).to(dev())
    hd = head.to(dev())
    for shape, n in (((5, 6, 40), 2), ((4, 4, 156), 1), ((3, 9, 36), 1)):
        x = torch.from_numpy(r.standard_normal((n, 32) + shape).astype(np.float32)).to(dev())
        with torch.no_grad():
            plain = m.fused(x)
            before = S._ROUTES["side_head"]
            y, hy = m.fused(x, side_head=hd)
            assert S._ROUTES["side_head"] == before + 1, "the side-head launch must be taken for a 32->32 k3 layer"
            assert torch.equal(y, plain)
            check(hy.cpu().numpy(), F.conv3d(plain.cpu(), head.weight.cpu()).numpy(), TIGHT, f"side head {shape}")
    with torch.no_grad():   # rows of 8-byte pieces (W % 4 == 2) and 64 output channels: projection in its own launch
        x = torch.from_numpy(r.standard_normal((1, 32, 4, 4, 38)).astype(np.float32)).to(dev())
        y, hy = m.fused(x, side_head=hd)
        assert torch.equal(y, m.fused(x)) and torch.equal(hy, hd(y))


def test_train_mode_batchnorm_matches_torch():
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    ours = seeded(S.convbn_3d(8, 32, 3, 1, 1), 31)
    ref = seeded(T.convbn_3d(8, 32, 3, 1, 1), 31)
    ours.train(); ref.train()
    ours = ours.to(dev())
    x = GC.randn((3, 8, 4, 5, 9), 32)
    with torch.no_grad():
        yr = ref(x)
        yo = ours(x.to(dev()))
    check(yo.cpu().numpy(), yr.numpy(), 5e-5, "train BN output")
    check(ours[1].running_mean.cpu().numpy(), ref[1].running_mean.numpy(), 1e-5, "running_mean")
    check(ours[1].running_var.cpu().numpy(), ref[1].running_var.numpy(), 1e-5, "running_var")
    assert int(ours[1].num_batches_tracked) == int(ref[1].num_batches_tracked)


def _grads(module, inputs, loss_fn):
    for p in module.parameters():
        p.grad = None
    for t in inputs:
        t.grad = None
    loss_fn().backward()
    return [t.grad.detach().cpu() for t in inputs], {k: (v.grad.detach().cpu() if v.grad is not None else None)
                                                      for k, v in module.named_parameters()}


_WGRAD_CASES = {
    # name: (N, Cin, Cout, (D, H, W) of the input, ksize, stride)
    "k3 many tiles": (1, 32, 32, (10, 40, 96), 3, 1),         # 300 Winograd tiles over 80 partitions: first / steady / last tile of a partition
    "k3 ragged": (2, 40, 24, (5, 10, 44), 3, 1),              # border tiles in H and W, channel blocks of 8 and 24, two samples
    "k3 one tile": (1, 32, 64, (2, 4, 32), 3, 1),             # partitions without any tile
    "k3 rows of 8 bytes": (1, 32, 32, (4, 6, 38), 3, 1),      # W % 4 != 0: the direct form with float2 pieces
    "k3 odd width": (1, 32, 32, (3, 6, 37), 3, 1),            # scalar staging
    "k3s2": (2, 32, 64, (6, 12, 40), 3, 2),
    "k3s2 many tiles": (1, 32, 32, (12, 40, 160), 3, 2),      # 180 tiles over 80 partitions, interior and border tiles
    "k3s2 rows of 8 bytes": (1, 32, 64, (4, 12, 76), 3, 2),   # output rows of 38 floats: 8-byte dy pieces
    "k3s2 odd extents": (1, 40, 24, (5, 9, 44), 3, 2),        # odd input depth / height, partial channel blocks
    "k1": (1, 40, 32, (3, 5, 36), 1, 1),
    "k1 to one channel": (2, 32, 1, (4, 6, 40), 1, 1),
}


@pytest.mark.parametrize("variant", ["auto", "fp32", "direct"])
@pytest.mark.parametrize("case", sorted(_WGRAD_CASES))
def test_conv3d_wgrad_vs_float64(case, variant):
    """snvc_conv3d_wgrad against the float64 weight gradient of F.conv3d on the CPU: the default form (r6: 3x3x3 / stride 1 on
    16-byte rows = the split-operand f16x3 form; else the fp32 forms), the fp32 forms (ALGO_WGRAD_FP32: the Winograd-domain one on
    16-byte rows) and the direct form, on shapes that give a partition several tiles, none, and border tiles."""
    import torch.nn.functional as F
    from snvc_amd import _lib, ops
    N, cin, cout, shp, k, st = _WGRAD_CASES[case]
    r = np.random.default_rng(300 + sorted(_WGRAD_CASES).index(case))
    x = torch.from_numpy(r.standard_normal((N, cin) + shp).astype(np.float32))
    w = torch.zeros(cout, cin, k, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, stride=st, padding=k // 2)
    g = torch.from_numpy(r.standard_normal(tuple(y.shape)).astype(np.float32))
    (y * g.double()).sum().backward()
    with ops.conv_variant({"auto": 0, "fp32": _lib.ALGO_WGRAD_FP32, "direct": _lib.ALGO_DIRECT}[variant]):
        dw = ops.conv3d_wgrad(x.to(dev()), g.to(dev()), k, st, k // 2, 1)
        dw2 = ops.conv3d_wgrad(x.to(dev()), g.to(dev()), k, st, k // 2, 1)
    assert torch.equal(dw, dw2), "the weight gradient is deterministic"
    check(dw.cpu().numpy(), w.grad.float().numpy(), 5e-6 if variant == "direct" else 2e-5, f"wgrad {case} ({variant})")


@pytest.mark.parametrize("case", ["k3_bn_train", "k3_bn_eval", "k3s2_bn_train", "k3s2_odd_bn_train", "k3s2_odd_w_bn_eval", "deconv_bn_train",
                                  "k3_gn", "k1_plain"])
def test_layer_backward_vs_torch_autograd(case):
    """fwd+bwd of one fused layer (conv/deconv + norm + residual + ReLU) against torch autograd on
    the CPU restatement: dx, dW, dgamma, dbeta, dresidual."""
    import torch.nn.functional as F
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    r = np.random.default_rng(71)
    gn = case.endswith("gn")
    if case.startswith("deconv"):
        ours, ref = S._deconvbn_3d(64, 32, gn), T._deconv_norm(64, 32, gn)
        xs = (2, 64, 3, 4, 20)
    elif case.startswith("k3s2"):
        ours, ref = S.convbn_3d(32, 64, 3, 2, 1, gn=gn), T.convbn_3d(32, 64, 3, 2, 1, gn=gn)
        # r4: odd extents under autograd (nn.Conv3d(k3,s2,p1) takes any, reference submodule.py:170-181)
        xs = {"k3s2_odd_bn_train": (2, 32, 5, 7, 41), "k3s2_odd_w_bn_eval": (1, 32, 4, 6, 37)}.get(case, (2, 32, 4, 6, 40))
    elif case.startswith("k1"):
        ours, ref = S.convbn_3d(40, 32, 1, 1, 0, gn=gn), T.convbn_3d(40, 32, 1, 1, 0, gn=gn)
        xs = (1, 40, 3, 5, 36)
    else:
        ours, ref = S.convbn_3d(32, 32, 3, 1, 1, gn=gn), T.convbn_3d(32, 32, 3, 1, 1, gn=gn)
        xs = (2, 32, 3, 6, 37)
    sd = T.seeded_state_dict(ref, 72)
    ours.load_state_dict(sd); ref.load_state_dict(sd)
    train = not case.endswith("eval")
    ours.train(train); ref.train(train)
    ours = ours.to(dev())
    x = torch.from_numpy(r.standard_normal(xs).astype(np.float32))
    with torch.no_grad():
        ys = tuple(ref(x).shape)
    res = torch.from_numpy(r.standard_normal(ys).astype(np.float32))
    gy = torch.from_numpy(r.standard_normal(ys).astype(np.float32))
    # ReLU is discontinuous: where a pre-activation is within 1e-2 of zero, rounding differences
    # between the two implementations could flip the mask bit -- give those elements zero upstream
    # gradient so that the comparison does not depend on it
    with torch.no_grad():
        v = ref(x)
    gy_all = gy
    for res_after in (False, True):
        pre = v if res_after else v + res
        gy = gy_all.masked_fill(pre.abs() < 1e-2, 0.0)
        xr, rr = x.clone().requires_grad_(), res.clone().requires_grad_()
        (gx_r, gr_r), gp_r = _grads(ref, [xr, rr], lambda: (
            ((F.relu(ref(xr)) + rr) if res_after else F.relu(ref(xr) + rr)) * gy).sum())
        xo, ro = x.to(dev()).requires_grad_(), res.to(dev()).requires_grad_()
        gyd = gy.to(dev())
        (gx_o, gr_o), gp_o = _grads(ours, [xo, ro], lambda: (
            ours.fused(xo, relu=True, residual=ro, residual_after_act=res_after) * gyd).sum())
        tol = 2e-4
        check(gx_o.numpy(), gx_r.numpy(), tol, f"{case} dx (res_after={res_after})")
        check(gr_o.numpy(), gr_r.numpy(), tol, f"{case} dres")
        for k in gp_r:
            check(gp_o[k].numpy(), gp_r[k].numpy(), tol, f"{case} d{k}")


def test_training_step_global_stack_vs_torch_autograd():
    """BASELINE.json configs[3] in miniature: fwd+bwd through build_cost_volume + GlobalStack with
    train-mode BatchNorm, loss = mean(cost^2); every parameter gradient
    and the gradients w.r.t. the left/right features against C-oracle + torch-CPU autograd."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(81)
    C, H, W, D = 32, 8, 40, 8
    L = r.standard_normal((2, C, H, W)).astype(np.float32)
    R = r.standard_normal((2, C, H, W)).astype(np.float32)
    s = np.stack([np.linspace(0, D - 1, D) + 0.5 * (np.arange(D) % 2), np.linspace(0, 5, D)]).astype(np.float32)
    ref, ours = T.GlobalStack(C), GlobalStack(C)
    sd = T.seeded_state_dict(ref, 82)
    ref.load_state_dict(sd); ours.load_state_dict(sd)
    ref.train(); ours.train()
    ours = ours.to(dev())

    class CV(torch.autograd.Function):      # C oracle as an autograd op on the CPU
        @staticmethod
        def forward(ctx, l, rr):
            return torch.from_numpy(O.cost_volume_forward(l.detach().numpy(), rr.detach().numpy(), s, 1))

        @staticmethod
        def backward(ctx, g):
            gl, gr = O.cost_volume_backward(g.contiguous().numpy(), s, 1)
            return torch.from_numpy(gl), torch.from_numpy(gr)

    lr, rr = torch.from_numpy(L).requires_grad_(), torch.from_numpy(R).requires_grad_()
    (gl_r, gr_r), gp_r = _grads(ref, [lr, rr], lambda: ref(CV.apply(lr, rr)).pow(2).mean())
    lo, ro = torch.from_numpy(L).to(dev()).requires_grad_(), torch.from_numpy(R).to(dev()).requires_grad_()
    sh = torch.from_numpy(s).to(dev())
    from snvc_amd.models import submodule as S
    before_c = S._ROUTES["commuted_first_conv_train"]
    (gl_o, gr_o), gp_o = _grads(ours, [lo, ro], lambda: ours.forward_pair(lo, ro, sh, 1).pow(2).mean())
    assert S._ROUTES["commuted_first_conv_train"] == before_c + 1      # non-uniform shifts: the first layer's forward warps after the convolution
    assert S._ROUTES["commuted_first_conv_backward"] >= 1               # ... and so does its backward (r4)
    # feature gradients pass through ~10 ReLUs: a mask bit that flips on a pre-activation of ~1e-7
    # perturbs a small neighbourhood, so they are compared in the L2 sense
    def l2(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))
    assert l2(gl_o.numpy(), gl_r.numpy()) < 1e-3 and l2(gr_o.numpy(), gr_r.numpy()) < 1e-3
    assert set(gp_o) == set(gp_r)
    for k in gp_r:
        check(gp_o[k].numpy(), gp_r[k].numpy(), 1e-3, f"d {k}")
    # BatchNorm bookkeeping moved the same way
    for (k, a), (_, b) in zip(ours.state_dict().items(), ref.state_dict().items()):
        if "running" in k:
            check(a.cpu().numpy(), b.numpy(), 1e-4, k)
    # the same step with rounds 1-3's backward (right half built, 3D data and weight gradients over it)
    S.COMMUTED_BACKWARD[0] = False
    try:
        lb, rb = torch.from_numpy(L).to(dev()).requires_grad_(), torch.from_numpy(R).to(dev()).requires_grad_()
        nb = S._ROUTES["commuted_first_conv_backward"]
        (gl_b, gr_b), gp_b = _grads(ours, [lb, rb], lambda: ours.forward_pair(lb, rb, sh, 1).pow(2).mean())
        assert S._ROUTES["commuted_first_conv_backward"] == nb
    finally:
        S.COMMUTED_BACKWARD[0] = True
    assert l2(gl_o.numpy(), gl_b.numpy()) < 1e-3 and l2(gr_o.numpy(), gr_b.numpy()) < 1e-3
    for k in gp_r:
        check(gp_o[k].numpy(), gp_b[k].numpy(), 1e-3, f"d {k} (vs the built-volume backward)")


# =============================================================================== a5 / a6
@pytest.mark.parametrize("name", list(GC.HOURGLASS_CASES))
def test_hourglass_vs_golden(name, G):
    from snvc_amd.models import submodule as S
    c, gn, shape, seed = GC.HOURGLASS_CASES[name]
    m = seeded(S.hourglass(c, gn=gn), seed).to(dev())
    x = GC.randn((1, c) + shape, seed + 1).to(dev())
    with torch.no_grad():
        out, pre, post = m(x, None, None)
        check(out.cpu().numpy(), G[f"hourglass/{name}/out"], 5e-5, "out")
        check(pre.cpu().numpy(), G[f"hourglass/{name}/pre"], 5e-5, "pre")
        check(post.cpu().numpy(), G[f"hourglass/{name}/post"], 5e-5, "post")
        sq = m(x, GC.randn(tuple(pre.shape), seed + 2).to(dev()), GC.randn(tuple(post.shape), seed + 3).to(dev()))[0]
        check(sq.cpu().numpy(), G[f"hourglass/{name}/sq_out"], 5e-5, "sq_out")


@pytest.mark.parametrize("name", list(GC.HOURGLASS16_CASES))
def test_hourglass16_vs_golden(name, G):
    from snvc_amd.models import submodule as S
    c, gn, shape, seed = GC.HOURGLASS16_CASES[name]
    m = seeded(S.hourglass_downsample_16(c, gn=gn), seed).to(dev())
    with torch.no_grad():
        y = m(GC.randn((1, c) + shape, seed + 1).to(dev())).cpu()
    check(y[:, ::2, :, ::2, ::2].numpy(), G[f"hourglass16/{name}_sub"], 1e-4, name)
    s = G[f"hourglass16/{name}_sum"]
    assert abs(y.double().sum().item() - s[0]) <= 1e-5 * s[1]


# =============================================================================== a7 / a8 / a12
def _cfg(grid, gn):
    import types
    cfg = types.SimpleNamespace(vernier_type="BEV_type3", backbone="hrfeat", gn=gn, grid_resolution=list(grid),
                                resolution=GC.RESOLUTION, x_range=(-1.0, 1.0), z_range=(-1.0, 1.0), num_parts=9)
    cfg.hrfeat = types.SimpleNamespace(output_channel=32, name="identity")
    cfg.n_sample_h, cfg.n_sample_w, cfg.n_sample_l = grid
    return cfg


@pytest.mark.parametrize("name", list(GC.TRUNK_CASES))
def test_vernier_scale_vs_golden(name, G):
    from oracle import torch_ref as T
    from snvc_amd.models.vernier import VernierScale
    grid, gn, n, fh, fw, seed = GC.TRUNK_CASES[name]
    m = VernierScale(_cfg(grid, gn))
    # same keys as the reference (checked against the imported reference by make_golden.py via torch_ref)
    ref_keys = [(k, tuple(v.shape)) for k, v in T.VernierTrunk(32, grid, gn).state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref_keys
    seeded(m, seed).to(dev())
    lf, rf, gpl, gpr = GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1)
    from snvc_amd.models import submodule as S
    with torch.no_grad():
        hip0, torch0 = S._ROUTES["neck2d_hip"], S._ROUTES["neck2d_torch"]
        out = m(lf.to(dev()), rf.to(dev()), gpl.to(dev()), gpr.to(dev()))
        # every block of the 2D neck + heads ran on the HIP kernels, none on torch's -- eval BatchNorm folded into the conv
        # epilogues, GroupNorm as conv + statistics + normalise launches
        hip1, torch1 = S._ROUTES["neck2d_hip"], S._ROUTES["neck2d_torch"]
        assert hip1 > hip0 and torch1 == torch0
        vox = m.construct_voxel(lf.to(dev()), rf.to(dev()), gpl.to(dev()), gpr.to(dev()))
        bev, occ5, _ = m.trunk_3d(vox)
        idx, conf = m.ncf_argmax(out["ncf"])
    assert set(out) == {"ncf", "occupancy", "coordinates"}
    tol = 3e-4 if gn else 1e-4
    check(out["occupancy"].cpu().numpy(), G[f"trunk/{name}/occupancy"], tol, "occupancy")
    check(bev[:, ::5].cpu().numpy(), G[f"trunk/{name}/bev_sub"], tol, "bev")
    check(out["ncf"].cpu().numpy(), G[f"trunk/{name}/ncf"], 5 * tol, "ncf")
    check(out["coordinates"].cpu().numpy(), G[f"trunk/{name}/coordinates"], tol, "coordinates")
    # a12: the device argmax equals numpy's argmax of the same device heatmap, bit for bit ...
    flat = out["ncf"].cpu().numpy().reshape(n, 9, -1)
    assert np.array_equal(idx.cpu().numpy(), np.argmax(flat, axis=2))
    assert np.array_equal(conf.cpu().numpy(), flat.max(axis=2))
    # ... and equals the reference's indices wherever the reference's top-2 gap exceeds the
    # heatmap tolerance (an argmax is only defined up to the error of the values it ranks)
    gold = G[f"trunk/{name}/ncf"].reshape(n, 9, -1)
    srt = np.sort(gold, axis=2)
    safe = (srt[:, :, -1] - srt[:, :, -2]) > 2e-3 * np.abs(gold).max()
    assert np.array_equal(idx.cpu().numpy()[safe], G[f"trunk/{name}/argmax"][safe])
    assert safe.mean() > 0.5


@pytest.mark.parametrize("name", list(GC.TYPE2_CASES))
def test_vernier_scale_type2_vs_golden(name):
    """vernier_type='BEV_type2' (reference vernier.py:191-248, :391-410: the BEV_type3 trunk without the coordinate head) against the
    imported reference's own outputs (tests/golden/make_golden_type2.py): same state-dict keys, ncf / occupancy, coordinates None."""
    import os
    from oracle import torch_ref as T
    from snvc_amd.models.vernier import VernierScale
    G2 = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vernier_type2.npz"))
    grid, gn, n, fh, fw, seed = GC.TYPE2_CASES[name]
    cfg = _cfg(grid, gn)
    cfg.vernier_type = "BEV_type2"
    m = VernierScale(cfg)
    ref_keys = [(k, tuple(v.shape)) for k, v in T.VernierTrunk(32, grid, gn, vernier_type="BEV_type2").state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == ref_keys
    assert not hasattr(m, "coord_head")
    seeded(m, seed).to(dev())
    lf, rf, gpl, gpr = (t.to(dev()) for t in GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1))
    tol = 3e-4 if gn else 1e-4
    for precision in ("auto", "f32"):
        m.precision = precision
        with torch.no_grad():
            out = m(lf, rf, gpl.clone(), gpr.clone())
        assert set(out) == {"ncf", "occupancy", "coordinates"} and out["coordinates"] is None
        check(out["occupancy"].cpu().numpy(), G2[f"{name}/occupancy"], tol, f"type2 occupancy [{precision}]")
        check(out["ncf"].cpu().numpy(), G2[f"{name}/ncf"], 5 * tol, f"type2 ncf [{precision}]")
    cfg_bad = _cfg((16, 16, 24), False)
    cfg_bad.vernier_type = "3D"
    with pytest.raises(NotImplementedError):
        VernierScale(cfg_bad)


def test_vernier_forward_self_check():
    """forward(test=True): the numeric half of the reference's aggregation self-check (vernier.py:479-519).  A pinhole
    calibration stand-in projects the grid: the host re-projection of the checked voxel agrees with the projected grid that
    was fed in, and the reported voxel feature is the aggregated one."""
    from snvc_amd.models.vernier import VernierScale
    name = list(GC.TRUNK_CASES)[0]
    grid, gn, n, fh, fw, seed = GC.TRUNK_CASES[name]
    m = seeded(VernierScale(_cfg(grid, gn)), seed).to(dev())
    nh, nw, nl = grid
    v = nh * nw * nl
    r = np.random.default_rng(41)

    class Calib:                                      # x = f X / Z + cx, y = f Y / Z + cy
        def __init__(self, shift):
            self.shift = shift

        def project_rect_to_image(self, p):
            p = np.asarray(p, dtype=np.float64)
            return np.stack([8.0 * (p[:, 0] + self.shift) / p[:, 2] + 16.0, 8.0 * p[:, 1] / p[:, 2] + 12.0], axis=1)

    # a 3D grid whose projections are integers in feature-map pixels times the down-sampling factor 4
    px = r.integers(1, fw - 1, v).astype(np.float64)
    py = r.integers(1, fh - 1, v).astype(np.float64)
    z = r.uniform(4.0, 9.0, v)
    g3 = np.stack([(4.0 * px - 16.0) * z / 8.0, (4.0 * py - 12.0) * z / 8.0, z], axis=1)
    cal_l, cal_r = Calib(0.0), Calib(-0.5)
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    gl = np.stack([cal_l.project_rect_to_image(g3).T] * n).astype(np.float32)            # [n, 2, v] in image pixels
    gr = np.stack([cal_r.project_rect_to_image(g3).T] * n).astype(np.float32)
    lf, rf, _, _ = GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1)
    gpl, gpr = torch.from_numpy(gl).to(dev()), torch.from_numpy(gr).to(dev())
    meta = {"grid_3d": [g3], "calib_left": [cal_l], "calib_right": [cal_r], "trans_l": [eye], "trans_r": [eye],
            "grid_proj_left": gpl.clone(), "grid_proj_right": gpr.clone()}
    with torch.no_grad():
        out = m(lf.to(dev()), rf.to(dev()), gpl, gpr, meta_data=meta, test=True)
    assert set(out) == {"ncf", "occupancy", "coordinates"}
    chk = m.last_self_check
    assert np.abs(chk["projection_error_left"]).max() < 1e-3 and np.abs(chk["projection_error_right"]).max() < 1e-3
    # the feature comparison is the reference's eyeball check (nearest pixel of x / 4 against the kernel's bilinear sample
    # at x / 4 - 0.5): only its plumbing is asserted -- the voxel feature is construct_voxel's, the difference is finite
    i, j, k = chk["voxel"]
    with torch.no_grad():
        vox = m.construct_voxel(lf.to(dev())[:1], rf.to(dev())[:1], gpl[:1], gpr[:1])
    assert torch.equal(chk["voxel_feature"], vox[0, :, i, j, k].cpu()) and torch.isfinite(chk["feature_abs_diff"]).all()
    assert chk["feature_abs_diff"].shape == (64,)


@pytest.mark.parametrize("name", list(GC.GLOBAL_CASES))
def test_global_stack_vs_golden(name, G):
    from snvc_amd.models.stereo_volume import GlobalStack
    c, shape, seed = GC.GLOBAL_CASES[name]
    m = seeded(GlobalStack(c), seed).to(dev())
    with torch.no_grad():
        y = m(GC.randn((1, 2 * c) + shape, seed + 1).to(dev())).cpu().numpy()
    check(y, G[f"global/{name}"], 1e-4, name)


def test_lazy_cost_volume_reference_call_sequence():
    """``vol = build_cost_volume(l, r, s, 1); model(vol)`` under no_grad: ``vol`` is a LazyCostVolume with the volume's
    shape / dtype / device; GlobalStack consumes it on the fused path (== forward_pair, bit for bit, nothing built);
    any other use builds the real volume, whose values are the eager builder's, bit for bit."""
    from snvc_amd import ops
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    from snvc_amd.lazy import LazyCostVolume
    from snvc_amd.models.stereo_volume import GlobalStack
    C, H, W, D = 32, 8, 40, 8
    r = np.random.default_rng(11)
    L = torch.from_numpy(r.standard_normal((2, C, H, W)).astype(np.float32)).to(dev())
    R = torch.from_numpy(r.standard_normal((2, C, H, W)).astype(np.float32)).to(dev())
    S_ = torch.from_numpy(np.tile(np.linspace(0.0, 9.5, D, dtype=np.float32), (2, 1))).to(dev())
    m = seeded(GlobalStack(C), 3).to(dev())
    eager = ops.cost_volume_forward(L, R, S_, 1)
    with torch.no_grad():
        vol = build_cost_volume(L, R, S_, 1)
        assert isinstance(vol, LazyCostVolume) and not vol.is_materialized
        assert tuple(vol.shape) == tuple(eager.shape) and vol.dtype == eager.dtype and vol.device == eager.device
        assert vol.is_cuda and vol.is_contiguous() and vol.size(1) == 2 * C and vol.dim() == 5
        y_api = m(vol)                                   # the reference's call sequence
        assert not vol.is_materialized                   # ... never built the volume
        y_pair = m.forward_pair(L, R, S_, 1)
        assert torch.equal(y_api, y_pair)
        y_mat = m(eager)                                 # conv1 over the materialised 64 channels
        check(y_api.cpu().numpy(), y_mat.cpu().numpy(), 1e-5, "fused path vs materialised volume")
        # any other use: the real volume
        vol2 = build_cost_volume(L, R, S_, 1)
        s = (vol2 * 2.0).sum()                           # an aten operator
        assert vol2.is_materialized and torch.equal(vol2.materialize(), eager) and s.item() == (eager * 2.0).sum().item()
        vol3 = build_cost_volume(L, R, S_, 1)
        assert torch.equal(vol3[:, C:], eager[:, C:]) and torch.equal(vol3.cpu(), eager.cpu())
        vol4 = build_cost_volume(L, R, S_, 1)
        y4 = m.conv1.fused(vol4)                         # a kernel of this library asking for the pointer
        assert vol4.is_materialized and torch.equal(y4, m.conv1.fused(eager))
        y5 = m(vol4)                                     # materialised but only LOOKED at: still the fused path (r4)
        assert vol4.is_pristine and torch.equal(y5, y_pair)
        vol7 = build_cost_volume(L, R, S_, 1)
        vol7.add_(1.0)                                   # written to through an aten operator: the values are the tensor's own now
        assert vol7.is_materialized and not vol7.is_pristine
        assert torch.equal(m(vol7), m(eager + 1.0))
        L2 = L.clone()
        vol8 = build_cost_volume(L2, R, S_, 1)
        L2.add_(1.0)                                     # a source modified before the volume was ever built: it cannot be any more
        with pytest.raises(RuntimeError, match="modified in place"):
            m(vol8)
        vol9 = build_cost_volume(L2, R, S_, 1)
        peek = vol9[:, :1].clone()                       # built, then a source changes: the BUILT values stay the volume's values
        L2.add_(1.0)
        assert not vol9.is_pristine and torch.equal(m(vol9), m(vol9.materialize())) and torch.equal(peek, vol9.materialize()[:, :1])
        m.train()
        vol6 = build_cost_volume(L, R, S_, 1)            # train-mode BatchNorm: not the fused path
        y6 = m(vol6)
        assert vol6.is_materialized and torch.isfinite(y6).all()
        m.eval()
        with pytest.raises(AssertionError):
            build_cost_volume(L, R, S_ - 1.0, 1)
    # with autograd on: the eager autograd function, as before
    Lg = L.clone().requires_grad_()
    vol_g = build_cost_volume(Lg, R, S_, 1)
    assert not isinstance(vol_g, LazyCostVolume) and vol_g.grad_fn is not None and torch.equal(vol_g, eager)
    # other dtypes / downsample: eager
    with torch.no_grad():
        assert not isinstance(build_cost_volume(L.double(), R.double(), S_.double(), 1), LazyCostVolume)
        v2 = build_cost_volume(L, R, S_, 2)                  # r6: downsample 2 is lazy too (even extents); its values are the eager op's
        assert isinstance(v2, LazyCostVolume) and torch.equal(v2.materialize(), ops.cost_volume_forward(L, R, S_, 2))
        assert not isinstance(build_cost_volume(L, R, S_, 8), LazyCostVolume)


@pytest.mark.parametrize("tile", ["default", "big", "narrow"])
def test_global_pair_end_to_end_vs_oracle(tile):
    """cost-volume build + 3D CNN forward (the benchmarked unit) against C oracle + torch-CPU."""
    from snvc_amd import _lib, ops
    # depth-class planes through every Winograd tile form
    bits = {"default": 0, "big": _lib.ALGO_WINO_TILE_BIG, "std": _lib.ALGO_WINO_TILE_STD,
            "narrow": _lib.ALGO_WINO_TILE_NARROW_REG}[tile]
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(41)
    C, H, W, D = 32, 8, 40, 8
    L = r.standard_normal((1, C, H, W)).astype(np.float32)
    R = r.standard_normal((1, C, H, W)).astype(np.float32)
    s = (np.linspace(0, D - 1, D) + 0.5 * (np.arange(D) % 2)).astype(np.float32)[None]
    ref = seeded(T.GlobalStack(C), 42)
    ours = seeded(GlobalStack(C), 42).to(dev())
    dl, dr, dsh = torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()), torch.from_numpy(s).to(dev())
    with torch.no_grad(), ops.conv_variant(bits):
        vol_ref = O.cost_volume_forward(L, R, s, 1)
        exp = ref(torch.from_numpy(vol_ref)).numpy()
        got_fact = ours.forward_pair(dl, dr, dsh, 1).cpu().numpy()                   # factored first conv
        got_full = ours.forward_pair(dl, dr, dsh, 1, factored=False).cpu().numpy()   # materialised volume
        # the right-half builder is the full builder's right half, bit for bit
        assert np.array_equal(ops.cost_volume_forward_right(dr, dsh).cpu().numpy(), vol_ref[:, C:])
        # first layer alone: factored == full convolution over the concat volume
        full1 = ours.conv1(torch.from_numpy(vol_ref).to(dev())).cpu().numpy()
    from snvc_amd.models import submodule as S
    if tile == "default":   # the folded tail and conv2's side head are what forward_pair runs on
        with torch.no_grad():
            b_f, b_s = S._ROUTES["folded_head"] + S._ROUTES["x3_fused_tail"], S._ROUTES["side_head"]
            ours.forward_pair(dl, dr, dsh, 1)      # split mode (r5): the tail's tap contraction sits in conv5's epilogue (x3_fused_tail)
            assert (S._ROUTES["folded_head"] + S._ROUTES["x3_fused_tail"], S._ROUTES["side_head"]) == (b_f + 1, b_s + 1)
    check(got_full, exp, 1e-4, "pair (materialised)")
    check(got_fact, exp, 1e-4, "pair (factored)")
    check(got_fact, got_full, 2e-5, "factored vs materialised")
    exp1 = ref.conv1(torch.from_numpy(vol_ref)).detach().numpy()
    check(full1, exp1, 2e-5, "conv1")


def test_lazy_cost_volume_prefetches_the_consumers_first_layer():
    """r5: build_cost_volume runs the step of the model that consumed the previous lazy volume up to its host sync (the check of
    `shift`, with that model's first-layer prep queued in front of the wait); model(volume) resumes it.  Same values as forward_pair
    bit for bit; the reference's assert still fires AT build time; a volume that is looked at, given to another model, or whose
    consumer's weights changed in between is handled as before."""
    from snvc_amd import ops
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    C, H, W, D = 32, 8, 40, 8
    r = np.random.default_rng(12)
    L = torch.from_numpy(r.standard_normal((1, C, H, W)).astype(np.float32)).to(dev())
    R = torch.from_numpy(r.standard_normal((1, C, H, W)).astype(np.float32)).to(dev())
    S_ = torch.from_numpy(np.linspace(0.0, 3.5, D, dtype=np.float32)[None]).to(dev())
    S2 = (S_ * 0.77 + 0.05).contiguous()                 # not uniformly spaced by 1 or 1/2: the general path
    m, other = seeded(GlobalStack(C), 3).to(dev()), seeded(GlobalStack(C), 4).to(dev())
    with torch.no_grad():
        ref1, ref2 = m.forward_pair(L, R, S_, 1).clone(), m.forward_pair(L, R, S2, 1).clone()
        ref_other = other.forward_pair(L, R, S_, 1).clone()
        m(build_cost_volume(L, R, S_, 1))                # m is now the registered consumer
        n0 = S._ROUTES["lazy_prefetch_resumed"]
        vol = build_cost_volume(L, R, S_, 1)
        assert vol._prefetch is not None and vol.spacing == (2, 0) and not vol.is_materialized
        assert torch.equal(m(vol), ref1) and S._ROUTES["lazy_prefetch_resumed"] == n0 + 1 and not vol.is_materialized
        assert torch.equal(m(build_cost_volume(L, R, S2, 1)), ref2)              # the speculation was for another spacing: dropped inside
        assert S._ROUTES["lazy_prefetch_resumed"] == n0 + 2
        assert torch.equal(m(build_cost_volume(L, R, S_, 1)), ref1)              # ... and back
        with pytest.raises(AssertionError):                                        # reference __init__.py:12, at build time
            build_cost_volume(L, R, S_ - 1.0, 1)
        # looked at before the model sees it: the paused step is dropped, the values are the eager builder's
        vol = build_cost_volume(L, R, S_, 1)
        assert torch.equal(vol.materialize(), ops.cost_volume_forward(L, R, S_, 1)) and vol._prefetch is None
        assert torch.equal(m(vol), ref1)
        # another model consumes the volume m's step was started for
        vol = build_cost_volume(L, R, S_, 1)
        n1 = S._ROUTES["lazy_prefetch_resumed"]
        assert torch.equal(other(vol), ref_other) and S._ROUTES["lazy_prefetch_resumed"] == n1
        assert torch.equal(other(build_cost_volume(L, R, S_, 1)), ref_other)     # `other` is the consumer now
        assert S._ROUTES["lazy_prefetch_resumed"] == n1 + 1
        # the consumer's weights change between build and forward: not resumed, new weights used
        vol = build_cost_volume(L, R, S_, 1)
        other.conv1[0][0].weight.mul_(1.5)
        n2 = S._ROUTES["lazy_prefetch_resumed"]
        got = other(vol)
        assert S._ROUTES["lazy_prefetch_resumed"] == n2 and torch.equal(got, other.forward_pair(L, R, S_, 1))
        # a source written to after build: the error of the lazy volume, as before
        vol = build_cost_volume(L, R, S_, 1)
        L.add_(1.0)
        with pytest.raises(RuntimeError, match="modified in place"):
            other(vol)
        L.sub_(1.0)


def test_global_pair_groupnorm_split_tail_vs_oracle():
    """GlobalStack(gn=True) (convbn_3d(..., gn=True), reference submodule.py:41-49): behind the fp32 first layer the stack runs in
    split mode through fused_conv3d_x3's GroupNorm form (r5: conv -> fp32 raw -> statistics -> affine pass writing the pair);
    against the oracle's GroupNorm stack on the C oracle's volume, and against the same model on the fp32-MFMA kernels."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(43)
    C, H, W, D = 32, 16, 40, 16
    L = r.standard_normal((2, C, H, W)).astype(np.float32)
    R = r.standard_normal((2, C, H, W)).astype(np.float32)
    s = np.stack([np.linspace(0, (D - 1) / 2, D), np.linspace(0, D - 1, D)]).astype(np.float32)
    ref = seeded(T.GlobalStack(C, gn=True), 44)
    ours = seeded(GlobalStack(C, gn=True), 44).to(dev())
    dl, dr, dsh = torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()), torch.from_numpy(s).to(dev())
    with torch.no_grad():
        exp = ref(torch.from_numpy(O.cost_volume_forward(L, R, s, 1))).numpy()
        b = S._ROUTES["x3_gn_tail"]
        got = ours.forward_pair(dl, dr, dsh, 1).cpu().numpy()
        assert S._ROUTES["x3_gn_tail"] == b + 1, "the GroupNorm stack did not take its split-mode tail"
        from snvc_amd.extension.build_cost_volume import build_cost_volume
        got_api = ours(build_cost_volume(dl, dr, dsh, 1)).cpu().numpy()
        got32 = ours.forward_pair(dl, dr, dsh, 1, arithmetic="fp32").cpu().numpy()
        assert S._ROUTES["x3_gn_tail"] == b + 2
    check(got, exp, 1e-4, "GroupNorm pair (split tail)")
    check(got_api, exp, 1e-4, "GroupNorm pair through model(build_cost_volume(...))")
    check(got32, exp, 1e-4, "GroupNorm pair (fp32 MFMA)")


@pytest.mark.parametrize("case", ["ds2_whole", "ds2_whole_m3", "ds2_half", "ds2_half_m5", "ds4_whole", "ds4_whole_m2"])
@pytest.mark.parametrize("arith", ["auto", "fp32"])
def test_global_pair_downsample_sheared_vs_oracle(case, arith):
    """r6: downsample = ds > 1 on uniformly spaced planes takes the sheared first layer with q*ds phases of the row-subsampled right
    feature: two phases (ds 2, planes one input pixel apart: the existing 3 x 7 layers, the feature itself in the upsampled
    image's place) or four (ds 2 with half-pixel planes, ds 4 with whole-pixel planes: three 3 x 3 layers added 4 elements apart,
    the expand kernels' q = 4 form).  Against the oracle -- the C restatement of BuildCostVolume_cuda.cu:63-98 at that downsample + the
    torch-CPU stack -- and against the materialised route; eight phases (ds 4, half-pixel planes) still materialise."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.extension.build_cost_volume import build_cost_volume
    from snvc_amd.lazy import LazyCostVolume
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    ds = 4 if case.startswith("ds4") else 2
    q = 2 if "half" in case else 1
    m0 = int(case.rsplit("_m", 1)[1]) if "_m" in case else 0
    r = np.random.default_rng(51 + m0 + 7 * ds + q)
    C, H, W, D = 32, 8, 40, 12
    L = r.standard_normal((2, C, ds * H, ds * W)).astype(np.float32)
    R = r.standard_normal((2, C, ds * H, ds * W)).astype(np.float32)
    row = ((m0 + np.arange(D)) / q).astype(np.float32)
    s = np.stack([row, row])
    ref = seeded(T.GlobalStack(C), 52)
    ours = seeded(GlobalStack(C), 52).to(dev())
    dl, dr, dsh = torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()), torch.from_numpy(s).to(dev())
    a = None if arith == "auto" else "fp32"
    with torch.no_grad():
        exp = ref(torch.from_numpy(O.cost_volume_forward(L, R, s, ds))).numpy()
        b = S._ROUTES["ds_sheared_first_conv"]
        got = ours.forward_pair(dl, dr, dsh, ds, arithmetic=a).cpu().numpy()
        assert S._ROUTES["ds_sheared_first_conv"] == b + 1, "the call did not take the sheared first layer"
        got_mat = ours.forward_pair(dl, dr, dsh, ds, sheared=False, arithmetic=a).cpu().numpy()
        assert S._ROUTES["ds_sheared_first_conv"] == b + 1
        if ds == 4:
            ours.forward_pair(dl, dr, dsh * 0.5, 4)                                # eight phases: not this route
            assert S._ROUTES["ds_sheared_first_conv"] == b + 1
        if arith == "auto":
            vol = build_cost_volume(dl, dr, dsh, ds)                                 # the lazy volume covers downsample 2 and 4
            assert isinstance(vol, LazyCostVolume)
            got_api = ours(vol).cpu().numpy()
            assert S._ROUTES["ds_sheared_first_conv"] == b + 2 and not vol.is_materialized
            check(got_api, exp, 1e-4, "through model(build_cost_volume(...))")
            assert np.array_equal(build_cost_volume(dl, dr, dsh, ds).cpu().numpy(), O.cost_volume_forward(L, R, s, ds))    # any other use: the volume
    check(got, exp, 1e-4, f"{case} (sheared first layer)")
    check(got_mat, exp, 1e-4, f"{case} (materialised)")
    check(got, got_mat, 2e-5, "sheared vs materialised")


@pytest.mark.parametrize("spacing", ["half_pixel", "whole_pixel"])
def test_global_pair_groupnorm_sheared_first_layer_vs_oracle(spacing):
    """r6: GlobalStack(gn=True) on uniformly spaced planes takes the sheared first layer with GroupNorm statistics from the sheared
    statistics pass (one channel per group: per-sample, per-channel statistics; the concat volume and conv1's 64-channel
    convolution over it are not built): against the oracle's GroupNorm stack (reference submodule.py:41-49 composed as
    vernier.py:128-142) on the C oracle's volume, two samples with different statistics."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(47)
    C, H, W, D = 32, 16, 40, 16
    L = r.standard_normal((2, C, H, W)).astype(np.float32)
    R = r.standard_normal((2, C, H, W)).astype(np.float32)
    R[1] *= 3.0                                   # the two samples' statistics differ
    row = np.linspace(0, (D - 1) / 2, D) if spacing == "half_pixel" else np.linspace(2, D + 1, D)
    s = np.stack([row, row]).astype(np.float32)
    ref = seeded(T.GlobalStack(C, gn=True), 45)
    ours = seeded(GlobalStack(C, gn=True), 45).to(dev())
    dl, dr, dsh = torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()), torch.from_numpy(s).to(dev())
    with torch.no_grad():
        exp = ref(torch.from_numpy(O.cost_volume_forward(L, R, s, 1))).numpy()
        b = S._ROUTES["gn_sheared_first_conv"]
        got = ours.forward_pair(dl, dr, dsh, 1).cpu().numpy()
        assert S._ROUTES["gn_sheared_first_conv"] == b + 1, "the GroupNorm stack did not take the sheared first layer"
        from snvc_amd.extension.build_cost_volume import build_cost_volume
        got_api = ours(build_cost_volume(dl, dr, dsh, 1)).cpu().numpy()
        assert S._ROUTES["gn_sheared_first_conv"] == b + 2
        got_general = ours.forward_pair(dl, dr, dsh, 1, sheared=False).cpu().numpy()       # the materialised route, as r5
        assert S._ROUTES["gn_sheared_first_conv"] == b + 2
        with pytest.raises(AssertionError):
            ours.forward_pair(dl, dr, dsh - 5.0, 1)
    check(got, exp, 1e-4, "GroupNorm pair (sheared first layer)")
    check(got_api, exp, 1e-4, "GroupNorm pair through model(build_cost_volume(...))")
    check(got_general, exp, 1e-4, "GroupNorm pair (materialised volume)")


@pytest.mark.parametrize("case", ["random", "whole_pixels", "beyond_the_image", "odd_width", "deep"])
def test_warped_expand_backward_vs_oracle(case):
    """snvc_warped_expand_backward (r4: the adjoint of the any-shift first layer) against the C oracle's cost-volume backward
    (BuildCostVolume_cuda.cu:152-205 restated): a[kd][kw] is the right-feature gradient of a volume gradient that holds dy moved
    by the (kd, kw) tap -- plane e takes dy's plane e-kd+1, column w' takes column w'-kw+1, zero padding outside.  Fractional,
    whole, zero shifts, shifts beyond the image, repeated and non-monotone rows; the depth-class sums bit-equal to
    snvc_depth_class_sums."""
    from oracle import native as O
    from snvc_amd import ops
    r = np.random.default_rng(171 + len(case))
    N, C, D, H, W = {"odd_width": (1, 2, 7, 3, 37), "deep": (1, 1, 37, 2, 72)}.get(case, (2, 3, 9, 5, 40))
    dy = r.standard_normal((N, C, D, H, W)).astype(np.float32)
    s = r.uniform(0, 14, (N, D))
    if case == "whole_pixels":
        s = np.floor(s)
        s[0, 0] = 0.0
    elif case == "beyond_the_image":
        s[:, ::2] = r.uniform(W - 2, W + 3, (N, (D + 1) // 2))
        s[0, 1], s[-1, 3] = float(W), float(W - 1)
    else:
        s[0, 2], s[-1, 5], s[0, 4] = 0.0, 3.0, 0.25
        s[0, 6] = s[0, 5]
    s = s.astype(np.float32)
    a, dpl = ops.warped_expand_backward(torch.from_numpy(dy).to(dev()), torch.from_numpy(s).to(dev()))
    a = a.cpu().numpy()
    for kd in range(3):
        for kw in range(3):
            g = np.zeros((N, 2 * C, D, H, W), np.float32)
            for e in range(D):
                d = e - kd + 1
                if 0 <= d < D:
                    lo, hi = max(0, kw - 1), min(W, W + kw - 1)          # w' with 0 <= w' - kw + 1 <= W-1
                    g[:, C:, e, :, lo:hi] = dy[:, :, d, :, lo - kw + 1:hi - kw + 1]
            _, exp = O.cost_volume_backward(g, s, 1)
            check(a[:, kd, kw], exp, 1e-5, f"a[{kd}][{kw}] ({case})")
    ref = ops.depth_class_sums(torch.from_numpy(dy).to(dev())) if (H * W) % 4 == 0 else None
    if ref is not None:
        assert torch.equal(dpl, ref)
    else:
        exp = np.stack([dy[:, :, 0], dy[:, :, 1:-1].sum(2), dy[:, :, -1]], axis=2)
        check(dpl.cpu().numpy(), exp, 1e-5, "depth-class sums")


@pytest.mark.parametrize("case", ["random", "whole_pixels", "beyond_the_image", "ragged_rows", "sweep_up", "sweep_down", "sweep_cfg1",
                                  "sweep_quarter"])
def test_commuted_first_conv_any_shift_vs_oracle_and_built_volume(case):
    """Any shift array (inference): the first convolution over the warped half as three interpolations of three 2D convolutions
    (snvc_warped_expand, csrc/sheared_conv.hip) -- against the C oracle's cost volume + the torch-CPU stack and against the path
    that builds the right half and runs the 3D convolution over it; first layer alone at the exact-fp32 tolerance.  Two samples
    with different, non-monotone shift rows: fractional, whole, zero, and larger than the image width."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(161 + len(case))
    C, D = 32, 12
    # 12 rows of 11 quads; like every shape here one row per workgroup (RB = 1: 12 * 32 * 2 workgroups stay below 1024) -- the larger row
    # blocks are in tests/test_gpu_first_layer_forms.py (the hourglass needs multiples of 4)
    H, W = (12, 44) if case == "ragged_rows" else (8, 40)
    L = r.standard_normal((2, C, H, W)).astype(np.float32)
    R = r.standard_normal((2, C, H, W)).astype(np.float32)
    s = r.uniform(0, 20, (2, D))
    if case == "whole_pixels":
        s = np.floor(s)
    elif case.startswith("sweep"):       # monotone plane sweeps: the register windows move by 0, +-1, +-2 columns per plane
        d_ = np.arange(D, dtype=np.float64)
        s = {"sweep_up": np.stack([0.7 * d_ + 0.3, 1.9 * d_]), "sweep_down": np.stack([30.0 - 1.3 * d_, 25.5 - 2.0 * d_]),
             "sweep_cfg1": np.stack([d_ + 0.5 * (d_ % 2), 3.0 + d_ + 0.5 * (d_ % 2)]),
             "sweep_quarter": np.stack([0.25 * d_, 40.0 + 0.25 * d_])}[case]
    elif case == "beyond_the_image":
        s[:, ::2] = r.uniform(W - 2, W + 3, (2, (D + 1) // 2))
        s[0, 1], s[1, 3] = float(W), float(W - 1)
    else:
        s[0, 2], s[1, 5], s[0, 7], s[1, 0] = 0.0, 3.0, 0.25, 19.999
    s = s.astype(np.float32)
    ref = seeded(T.GlobalStack(C), 162)
    ours = seeded(GlobalStack(C), 162).to(dev())
    dl, dr, dsh = torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()), torch.from_numpy(s).to(dev())
    with torch.no_grad():
        exp = ref(torch.from_numpy(O.cost_volume_forward(L, R, s, 1))).numpy()
        before = S._ROUTES["commuted_first_conv"]
        got = ours.forward_pair(dl, dr, dsh, 1).cpu().numpy()
        assert S._ROUTES["commuted_first_conv"] == before + 1
        v1c = ours.last_first_layer().clone()
        built = ours.forward_pair(dl, dr, dsh, 1, commuted=False).cpu().numpy()
        assert S._ROUTES["commuted_first_conv"] == before + 1
        v1b = ours.last_first_layer().clone()
    check(v1c.cpu().numpy(), v1b.cpu().numpy(), TIGHT, f"first layer, warp after convolution vs built volume ({case})")
    check(got, exp, 1e-4, f"pair vs oracle ({case})")
    check(got, built, 2e-5, f"pair, warp after convolution vs built volume ({case})")
    # the r3 kernel form (SNVC_WARPED_EXPAND_R3) and the register-window form agree to fp32 rounding
    from snvc_amd import ops
    ops.WARPED_EXPAND_FORM[0] = ops.WARPED_EXPAND_R3
    try:
        with torch.no_grad():
            ours.forward_pair(dl, dr, dsh, 1)
            v1r = ours.last_first_layer().clone()
    finally:
        ops.WARPED_EXPAND_FORM[0] = 0
    check(v1c.cpu().numpy(), v1r.cpu().numpy(), 2e-6, f"first layer, register-window form vs r3 form ({case})")


def test_shift_structure_flags():
    """snvc_shift_structure: the one-launch replacement of the wrapper's `assert torch.all(shift >= 0)` also classifies the
    array (whole- / half-pixel uniform spacing, exactly in fp32)."""
    from snvc_amd import ops
    D = 192
    ar = np.arange(D, dtype=np.float32)
    mk = lambda rows: torch.from_numpy(np.stack(rows).astype(np.float32)).to(dev())      # noqa: E731
    assert ops.shift_structure(mk([ar / 2, ar / 2])) == (True, False, True, 0.0)                 # cfg2: linspace(0, 95.5, 192)
    assert ops.shift_structure(mk([3 + ar])) == (True, True, False, 3.0)
    assert ops.shift_structure(mk([1.5 + ar / 2] * 3)) == (True, False, True, 1.5)
    assert ops.shift_structure(mk([ar / 2, ar / 2 + 0.25]))[:3] == (True, False, False)          # rows differ
    bad = ar / 2
    bad[77] = np.nextafter(bad[77], np.float32(1e9))
    assert ops.shift_structure(mk([bad]))[:3] == (True, False, False)                            # one ulp off: general path
    assert ops.shift_structure(mk([ar - 1]))[:2] == (False, True)                                # negative shift: the wrapper's assert
    nan = ar.copy(); nan[5] = np.nan
    assert ops.shift_structure(mk([nan]))[0] is False
    assert ops.shift_structure(mk([np.linspace(0, 5, D)]))[:3] == (True, False, False)


def test_shift_structure_tickets_and_non_finite():
    """two unresolved tickets do not share their 16-byte result; an all-+inf shift array is "non-negative" and
    "uniform" but is not a spacing (no OverflowError); resolved tickets are reused."""
    from snvc_amd import ops
    ar = np.arange(16, dtype=np.float32)
    a = torch.from_numpy((ar / 2)[None].copy()).to(dev())
    b = torch.from_numpy((5 + ar)[None].copy()).to(dev())
    ta, tb = ops.shift_structure_begin(a), ops.shift_structure_begin(b)
    assert ta is not tb and ta[0].data_ptr() != tb[0].data_ptr()
    assert ops.shift_spacing_result(tb, 16) == (True, (1, 5))
    assert ops.shift_spacing_result(ta, 16) == (True, (2, 0))
    tc = ops.shift_structure_begin(a)
    assert tc is ta or tc is tb                                     # back from the free list
    assert ops.shift_spacing_result(tc, 16) == (True, (2, 0))
    inf = torch.full((1, 16), float("inf"), device=dev())
    nonneg, spacing = ops.shift_spacing_result(ops.shift_structure_begin(inf), 16)
    assert spacing is None


def test_first_conv_shapes_outside_the_special_kernels_take_the_general_path():
    """rows wider than the sheared / warp-after-convolution kernels cover (W / 4 > 512) must not abort the step:
    forward_pair lands on the built-right-half path and returns the oracle's answer."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(5)
    C, H, W, D = 32, 4, 2052, 4
    L = r.standard_normal((1, C, H, W)).astype(np.float32)
    R = r.standard_normal((1, C, H, W)).astype(np.float32)
    ref = seeded(T.GlobalStack(C), 7)
    ours = seeded(GlobalStack(C), 7).to(dev())
    for s in (np.arange(D, dtype=np.float32)[None] / 2, np.array([[0.0, 0.7, 3.0, 4.25]], dtype=np.float32)):
        with torch.no_grad():
            exp = ref(torch.from_numpy(O.cost_volume_forward(L, R, s, 1))).numpy()
            before = (S._ROUTES["sheared_first_conv"], S._ROUTES["commuted_first_conv"])
            got = ours.forward_pair(*(torch.from_numpy(a).to(dev()) for a in (L, R, s)), 1).cpu().numpy()
            assert (S._ROUTES["sheared_first_conv"], S._ROUTES["commuted_first_conv"]) == before
        check(got, exp, 1e-4, "pair, W = 2052")


def test_hourglass_training_twice_over_a_retained_graph():
    """the skip-connection taps (_SkipTap / _GradBox) survive a second backward over a retained graph."""
    from snvc_amd.models.submodule import hourglass
    torch.manual_seed(3)
    hg = hourglass(32).to(dev()).train()
    x = torch.randn(1, 32, 8, 8, 32, device=dev(), requires_grad=True)
    out = hg(x, None, None, residual=x)[0]
    loss = out.pow(2).mean()
    g1 = torch.autograd.grad(loss, [x] + list(hg.parameters()), retain_graph=True)
    g2 = torch.autograd.grad(loss, [x] + list(hg.parameters()))
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("q,m0", [(2, 0), (2, 3), (1, 0), (1, 2)])
def test_sheared_first_conv_vs_oracle_and_general_path(q, m0):
    """Uniformly spaced disparity planes, shift[d] = (m0 + d) / q: forward_pair takes the sheared first convolution
    (csrc/sheared_conv.hip: no warped volume, conv1 as a 2D convolution along the shear) -- against the C oracle's cost
    volume + the torch-CPU stack, and against the general factored path on the same inputs; every border (d = 0, D-1,
    w = 0, W-1, x < 0 gate, planes of the left half) is inside these small shapes.  Any other shift array keeps the
    general path (route counter)."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(141 + 10 * q + m0)
    C, H, W, D = 32, 8, 40, 12
    L = r.standard_normal((2, C, H, W)).astype(np.float32)
    R = r.standard_normal((2, C, H, W)).astype(np.float32)
    s = np.tile(((m0 + np.arange(D)) / q).astype(np.float32)[None], (2, 1))
    ref = seeded(T.GlobalStack(C), 142)
    ours = seeded(GlobalStack(C), 142).to(dev())
    dl, dr, dsh = torch.from_numpy(L).to(dev()), torch.from_numpy(R).to(dev()), torch.from_numpy(s).to(dev())
    with torch.no_grad():
        exp = ref(torch.from_numpy(O.cost_volume_forward(L, R, s, 1))).numpy()
        before = S._ROUTES["sheared_first_conv"]
        got = ours.forward_pair(dl, dr, dsh, 1).cpu().numpy()
        assert S._ROUTES["sheared_first_conv"] == before + 1
        general = ours.forward_pair(dl, dr, dsh, 1, sheared=False, commuted=False).cpu().numpy()      # right half built
        assert S._ROUTES["sheared_first_conv"] == before + 1
        # first layer alone (before conv2 / the hourglass smooth anything over): the sheared planes against the general ones
        v_sheared = ours.__dict__["_snvc_ws"]
        ours.forward_pair(dl, dr, dsh, 1)
        v1s = ours.last_first_layer().clone()
        ours.forward_pair(dl, dr, dsh, 1, sheared=False, commuted=False)
        v1g = ours.last_first_layer().clone()
        # a shift array that is not uniformly spaced: general path
        dsh2 = dsh.clone()
        dsh2[0, 5] += 0.25
        ours.forward_pair(dl, dr, dsh2, 1)
        assert S._ROUTES["sheared_first_conv"] == before + 2
        # the spacing changes between calls: the launches queued for the previous call's spacing are dropped, not used
        q3, m3 = (1, 1) if q == 2 else (2, 1)
        s3 = torch.from_numpy(np.tile(((m3 + np.arange(D)) / q3).astype(np.float32)[None], (2, 1))).to(dev())
        ours.forward_pair(dl, dr, dsh, 1)                                   # spacing (q, m0) is now the guess
        other = ours.forward_pair(dl, dr, s3, 1).cpu().numpy()
        other_general = ours.forward_pair(dl, dr, s3, 1, sheared=False, commuted=False).cpu().numpy()
        back = ours.forward_pair(dl, dr, dsh, 1).cpu().numpy()              # and back again
        check(other, other_general, 2e-5, "spacing changed between calls")
        assert np.array_equal(back, got)
    check(v1s.cpu().numpy(), v1g.cpu().numpy(), TIGHT, f"first layer, sheared vs general q={q} m0={m0}")
    check(got, exp, 1e-4, f"pair (sheared) vs oracle q={q} m0={m0}")
    check(got, general, 2e-5, f"sheared vs general path q={q} m0={m0}")


@pytest.mark.parametrize("case", ["k3s1_32", "k3s1_64_ragged", "k3s2_32_64", "k3s2_ragged", "deconv_64_32", "deconv_ragged", "unsupported_w78"])
def test_conv_statistics_epilogue_vs_separate_pass(case):
    """snvc_conv3d_forward_stats: the convolution result is bit-identical to the plain launch and the batch statistics taken in
    its epilogue equal snvc_norm_stats' over that tensor (fp64 sums in a different order: 1e-6), for tile-ragged extents, two
    samples and two channel groups; a layer whose rows do not allow the carrying kernel forms reports that it did nothing."""
    from snvc_amd import ops
    cin, cout, stride, shape = {"k3s1_32": (32, 32, 1, (8, 8, 64)), "k3s1_64_ragged": (6, 64, 1, (5, 7, 72)),
                                "k3s2_32_64": (32, 64, 2, (8, 16, 128)), "k3s2_ragged": (4, 32, 2, (10, 14, 72)),
                                "deconv_64_32": (64, 32, 2, (4, 8, 64)), "deconv_ragged": (6, 64, 2, (3, 5, 36)),
                                "unsupported_w78": (8, 32, 1, (4, 4, 78))}[case]
    transposed = case.startswith("deconv")
    r = np.random.default_rng(231)
    wshape = (cin, cout, 3, 3, 3) if transposed else (cout, cin, 3, 3, 3)
    w = torch.from_numpy((0.1 * r.standard_normal(wshape)).astype(np.float32)).to(dev())
    x = torch.from_numpy(r.standard_normal((2, cin) + shape).astype(np.float32)).to(dev())
    gamma = torch.from_numpy(r.uniform(0.5, 1.5, cout).astype(np.float32)).to(dev())
    beta = torch.from_numpy(r.standard_normal(cout).astype(np.float32)).to(dev())
    # the same comparison on a result whose per-channel mean is 50 .. 400 x its spread (tests/stats_cases.py, where the float64 bound is)
    import stats_cases as SC
    assert SC.layer_of("fp32", case)[:5] == (cin, cout, shape, stride, transposed)
    x_off, w_off = (torch.from_numpy(a).to(dev()) for a in SC.conv_inputs("fp32", case, "offset"))
    for data, x, w in (("ordinary", x, w), ("offset", x_off, w_off)):
        layer = ops.Conv3dLayer(w, 3, stride, 1, 1, transposed)
        got = layer.forward_stats(x, gamma, beta, 1e-5)
        if case.startswith("unsupported"):
            assert got is None
            continue
        raw, scale, shift, mean, var = got
        ref = layer(x)
        assert torch.equal(raw, ref)
        s2, h2, m2, v2 = ops.norm_stats(ref, gamma, beta, cout, False, 1e-5)
        for a_, b_, what in ((scale, s2, "scale"), (shift, h2, "shift"), (mean, m2, "mean"), (var, v2, "var")):
            np.testing.assert_allclose(a_.cpu().numpy(), b_.cpu().numpy(), rtol=2e-6, atol=2e-7, err_msg=f"{what}, {data} data")


@pytest.mark.parametrize("fused_bn", [True, False])
@pytest.mark.parametrize("q,m0", [(2, 0), (2, 3), (1, 0), (1, 2)])
def test_training_step_sheared_first_conv_vs_torch_autograd(q, m0, fused_bn):
    """Training (cfg4) with uniformly spaced disparity planes: the first layer runs sheared in BOTH directions
    (_ShearedFirstConvFn: snvc_sheared_reduce / snvc_sheared_wgrad / the 3 x 7 dgrad / snvc_sheared_upsample_backward).
    Every parameter gradient and the feature gradients against the C oracle's cost volume + torch-CPU autograd, and
    against the general factored function on the same inputs.  ``fused_bn``: the train-mode BatchNorm + ReLU folded around the
    layer (_ShearedFirstConvBNFn: snvc_sheared_expand_stats / snvc_sheared_backward_reduce, no raw result, no raw gradient)."""
    from oracle import native as O
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(181 + 10 * q + m0)
    C, H, W, D = 32, 8, 40, 12
    L = r.standard_normal((2, C, H, W)).astype(np.float32)
    R = r.standard_normal((2, C, H, W)).astype(np.float32)
    s = np.tile(((m0 + np.arange(D)) / q).astype(np.float32)[None], (2, 1))
    ref, ours = T.GlobalStack(C), GlobalStack(C)
    sd = T.seeded_state_dict(ref, 182)
    ref.load_state_dict(sd); ours.load_state_dict(sd)
    ref.train(); ours.train()
    ours = ours.to(dev())

    class CV(torch.autograd.Function):
        @staticmethod
        def forward(ctx, l, rr):
            return torch.from_numpy(O.cost_volume_forward(l.detach().numpy(), rr.detach().numpy(), s, 1))

        @staticmethod
        def backward(ctx, g):
            gl, gr = O.cost_volume_backward(g.contiguous().numpy(), s, 1)
            return torch.from_numpy(gl), torch.from_numpy(gr)

    lr, rr = torch.from_numpy(L).requires_grad_(), torch.from_numpy(R).requires_grad_()
    (gl_r, gr_r), gp_r = _grads(ref, [lr, rr], lambda: ref(CV.apply(lr, rr)).pow(2).mean())
    lo, ro = torch.from_numpy(L).to(dev()).requires_grad_(), torch.from_numpy(R).to(dev()).requires_grad_()
    sh = torch.from_numpy(s).to(dev())
    before, before_bn = S._ROUTES["sheared_first_conv_train"], S._ROUTES["sheared_first_conv_train_fused_bn"]
    before_stats, before_x3 = S._ROUTES["conv_stats_epilogue"], S._ROUTES["x3_train_dgrad"]
    (gl_o, gr_o), gp_o = _grads(ours, [lo, ro], lambda: ours.forward_pair(lo, ro, sh, 1, fused_bn=fused_bn).pow(2).mean())
    assert S._ROUTES["conv_stats_epilogue"] >= before_stats + 1      # conv2 (fp32 Winograd, statistics in its epilogue)
    assert S._ROUTES["x3_train_dgrad"] == before_x3 + 7              # r6: conv2 and the hourglass's six layers on the split kernels, both directions
    assert S._ROUTES["sheared_first_conv_train"] == before + 1
    assert S._ROUTES["sheared_first_conv_train_fused_bn"] == before_bn + (1 if fused_bn else 0)
    for (k, a), (_, b) in zip(ours.state_dict().items(), ref.state_dict().items()):     # BatchNorm bookkeeping after ONE step
        if "running" in k:
            check(a.cpu().numpy(), b.numpy(), 1e-4, k)
    # the same step on the general factored function (the running statistics move a second time: gradients only)
    lg, rg = torch.from_numpy(L).to(dev()).requires_grad_(), torch.from_numpy(R).to(dev()).requires_grad_()
    (gl_g, gr_g), gp_g = _grads(ours, [lg, rg], lambda: ours.forward_pair(lg, rg, sh, 1, sheared=False, commuted=False).pow(2).mean())
    assert S._ROUTES["sheared_first_conv_train"] == before + 1

    def l2(a, b):
        return float(np.linalg.norm(a - b) / np.linalg.norm(b))
    assert l2(gl_o.numpy(), gl_r.numpy()) < 1e-3 and l2(gr_o.numpy(), gr_r.numpy()) < 1e-3
    assert l2(gl_o.numpy(), gl_g.numpy()) < 1e-3 and l2(gr_o.numpy(), gr_g.numpy()) < 1e-3
    assert set(gp_o) == set(gp_r)
    for k in gp_r:
        check(gp_o[k].numpy(), gp_r[k].numpy(), 1e-3, f"d {k} (vs torch)")
        check(gp_o[k].numpy(), gp_g[k].numpy(), 1e-3, f"d {k} (vs general)")


@pytest.mark.parametrize("fused_bn", [True, False])
def test_first_layer_backward_runs_on_the_layers_of_its_own_forward(fused_bn):
    """Another forward with updated first-layer weights (and another plane spacing) between a graph's forward and its backward replaces
    the layer's training cache (_first_conv_train_cache).  The first graph's backward still runs on the layers its own forward built:
    the gradients of the undisturbed step, bit for bit (the same launches on the same tensors; the weight is no saved tensor, so
    autograd's version check does not see the update)."""
    from snvc_amd.models.stereo_volume import GlobalStack
    r = np.random.default_rng(191)
    C, H, W, D = 32, 8, 40, 12
    model = seeded(GlobalStack(C), 182).to(dev()).train()
    L, R = (torch.from_numpy(r.standard_normal((2, C, H, W)).astype(np.float32)).to(dev()).requires_grad_() for _ in range(2))
    half = torch.from_numpy(np.tile((np.arange(D) / 2).astype(np.float32)[None], (2, 1))).to(dev())
    whole = torch.from_numpy(np.tile(np.arange(D).astype(np.float32)[None], (2, 1))).to(dev())
    w1 = model.conv1[0][0].weight

    def step(disturb):
        for t in list(model.parameters()) + [L, R]:
            t.grad = None
        loss = model.forward_pair(L, R, half, 1, fused_bn=fused_bn).pow(2).mean()
        if disturb:
            with torch.no_grad():
                w1.mul_(1.25)
            model.forward_pair(L, R, whole, 1, fused_bn=fused_bn)            # under autograd: rebuilds the cache for the new weight, q = 1
        loss.backward()
        return [L.grad.clone(), R.grad.clone()] + [p.grad.clone() for p in model.conv1.parameters()]
    step(False)                                                                 # from the second step on the layers' operands come as twins
    want, got = step(False), step(True)
    assert len(want) == len(got) == 5
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("q,m0", [(2, 0), (2, 5), (1, 1)])
def test_sheared_fused_batchnorm_entry_points_vs_numpy(q, m0):
    """snvc_sheared_expand_stats against the statistics of the expanded tensor, and snvc_sheared_backward_reduce against the
    same sums formed in numpy from the expanded tensor and a random gy: per-channel fp64 sums, shear-line sums, last-column
    slots and depth-class sums of both the masked gradient and raw.  Two samples, W = 24.  With C = 3 and H = 6 the forward kernels run
    one row per workgroup (RB = 1; tests/test_gpu_first_layer_forms.py has the larger row blocks and their short last block); the
    backward kernel's four-row blocks leave a last block of two rows."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    r = np.random.default_rng(211 + q + m0)
    N, C, D, H, W = 2, 3, 10, 6, 24
    off, wu, off_col, wu_col = sheared_geometry(q, m0, D, W)
    g = torch.from_numpy(r.standard_normal((N, 3 * C, H, wu)).astype(np.float32)).to(dev())
    gcol = torch.from_numpy(r.standard_normal((N, 3 * C, H, wu_col)).astype(np.float32)).to(dev())
    planes = torch.from_numpy(r.standard_normal((N, C, 3, H, W)).astype(np.float32)).to(dev())
    gamma = torch.from_numpy(r.uniform(0.5, 1.5, C).astype(np.float32)).to(dev())
    beta = torch.from_numpy(r.standard_normal(C).astype(np.float32)).to(dev())
    raw_t = torch.empty((N, C, D, H, W), device=dev())
    ops.sheared_expand(g, gcol, planes, None, None, raw_t, q, m0, off, off_col, 0)
    raw = raw_t.cpu().numpy().astype(np.float64)
    scale, shift, mean, var = ops.sheared_expand_stats(g, gcol, planes, gamma, beta, (N, C, D, H, W), q, m0, off, off_col, 1e-5)
    mu, vr = raw.mean((0, 2, 3, 4)), raw.var((0, 2, 3, 4))
    np.testing.assert_allclose(mean.cpu().numpy()[0], mu, rtol=0, atol=1e-6)
    np.testing.assert_allclose(var.cpu().numpy()[0], vr, rtol=1e-6)
    sc = gamma.cpu().numpy() / np.sqrt(vr + 1e-5)
    np.testing.assert_allclose(scale.cpu().numpy()[0], sc, rtol=2e-6)
    np.testing.assert_allclose(shift.cpu().numpy()[0], beta.cpu().numpy() - mu * sc, rtol=0, atol=2e-6)

    gy = r.standard_normal((N, C, D, H, W)).astype(np.float32)
    line, colsum, lastc, sums = ops.sheared_backward_reduce(g, gcol, planes, scale, shift, torch.from_numpy(gy).to(dev()), q, m0, off, off_col)
    rawf = raw_t.cpu().numpy()
    v = rawf * scale.cpu().numpy()[0][None, :, None, None, None] + shift.cpu().numpy()[0][None, :, None, None, None]
    gm = np.where(v > 0, gy, 0).astype(np.float64)
    exp_sums = np.stack([gm.sum((2, 3, 4)), (gm * raw).sum((2, 3, 4))], -1)
    np.testing.assert_allclose(sums.cpu().numpy(), exp_sums, rtol=2e-6, atol=2e-5)
    cls_of = lambda d: 0 if d == 0 else (2 if d == D - 1 else 1)          # noqa: E731
    e_line, e_last, e_col = np.zeros((2, N, 3, C, H, wu)), np.zeros((2, N, 3, C, H, wu_col)), np.zeros((2, N, C, 3, H, W))
    for qi, src in enumerate((gm, raw)):
        for d in range(D):
            cls = cls_of(d)
            e_col[qi, :, :, cls] += src[:, :, d]
            for w in range(W - 1):
                i = q * w - d - m0 + off
                if 0 <= i < wu:
                    e_line[qi, :, cls, :, :, i] += src[:, :, d, :, w]
            e_last[qi, :, cls, :, :, q * (W - 1) - d - m0 + off_col] += src[:, :, d, :, W - 1]
    check(line.cpu().numpy().reshape(e_line.shape), e_line.astype(np.float32), 1e-5, "line sums")
    check(lastc.cpu().numpy().reshape(e_last.shape), e_last.astype(np.float32), 0, "last-column slots")
    check(colsum.cpu().numpy(), e_col.astype(np.float32), 1e-5, "depth-class sums")


@pytest.mark.parametrize("q,m0", [(2, 0), (2, 5), (1, 1)])
def test_sheared_backward_entry_points_vs_numpy(q, m0):
    """snvc_sheared_reduce is the exact adjoint of snvc_sheared_expand (bit-exact against a numpy scatter in the same order
    for the one-term slots, 1e-5 for the sums), snvc_sheared_wgrad against an fp64 correlation, snvc_sheared_upsample_backward
    against the transpose of the interpolation matrix."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    r = np.random.default_rng(191 + q + m0)
    N, C, D, H, W = 2, 5, 9, 3, 21
    off, wu, off_col, wu_col = sheared_geometry(q, m0, D, W)
    dy = r.standard_normal((N, C, D, H, W)).astype(np.float32)
    dg, dgc = ops.sheared_reduce(torch.from_numpy(dy).to(dev()), q, m0, wu, off, wu_col, off_col)
    exp_g = np.zeros((N, 3, C, H, wu), np.float64)
    exp_c = np.zeros((N, 3, C, H, wu_col), np.float64)
    for d in range(D):
        cls = 0 if d == 0 else (2 if d == D - 1 else 1)
        for w in range(W - 1):
            if 0 <= q * w - d - m0 + off < wu:           # further left than the kernel's reach: G is zero there, nothing to sum
                exp_g[:, cls, :, :, q * w - d - m0 + off] += dy[:, :, d, :, w]
        exp_c[:, cls, :, :, q * (W - 1) - d - m0 + off_col] += dy[:, :, d, :, W - 1]
    check(dg.cpu().numpy().reshape(exp_g.shape), exp_g.astype(np.float32), 1e-5, "dG")
    check(dgc.cpu().numpy().reshape(exp_c.shape), exp_c.astype(np.float32), 0, "dG'")

    # 3 x 7 weight gradient (CO = 40: one full and one ragged channel group; C < 32)
    CO, WU = 40, 2 * 64 + 20
    x = r.standard_normal((N, C, H, WU)).astype(np.float32)
    gy = r.standard_normal((N, CO, H, WU)).astype(np.float32)
    dk = ops.sheared_wgrad(torch.from_numpy(x).to(dev()), torch.from_numpy(gy).to(dev())).cpu().numpy()
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (3, 3)))
    exp = np.zeros((CO, C, 3, 7))
    for kh in range(3):
        for t in range(7):
            exp[:, :, kh, t] = np.einsum("nohi,nchi->oc", gy.astype(np.float64), xp[:, :, kh:kh + H, t:t + WU])
    check(dk, exp.astype(np.float32), 1e-5, "dK")

    # adjoint of the upsampling: <upsample(R), G> == <R, upsample_backward(G)> and against the dense transpose
    R = r.standard_normal((N, C, H, W)).astype(np.float32)
    G = r.standard_normal((N, C, H, wu)).astype(np.float32)
    up = ops.sheared_upsample(torch.from_numpy(R).to(dev()), q, wu, off).cpu().numpy().astype(np.float64)
    M = np.zeros((wu, W))                                    # up[i] = sum_j M[i][j] R[j]
    for j in range(W):
        e = np.zeros((1, 1, 1, W), np.float32); e[..., j] = 1
        M[:, j] = ops.sheared_upsample(torch.from_numpy(e).to(dev()), q, wu, off).cpu().numpy().reshape(-1)
    back = ops.sheared_upsample_backward(torch.from_numpy(G).to(dev()), q, W, off).cpu().numpy()
    check(back, (G.astype(np.float64) @ M).astype(np.float32), 1e-6, "upsample backward")
    assert abs((up * G).sum() - (back.astype(np.float64) * R).sum()) < 1e-3


@pytest.mark.parametrize("gn,exact_k57", [(False, False), (True, False), (False, True)])
def test_training_step_vernier_trunk_vs_torch_autograd(gn, exact_k57, request):
    """Local (V-A) model: gather + 3D trunk (7^3, 5^3, dilated 5^3 convs, hourglass, heads' inputs)
    forward+backward in train mode against torch-CPU autograd: every 3D-trunk parameter gradient and
    the gradients w.r.t. the two feature maps.  The k5 / k7 layers on their Winograd forms (the default under autograd since
    r4) and on the direct kernels (TRAIN_EXACT_K57)."""
    from oracle import torch_ref as T
    from snvc_amd.models import submodule as S_
    from snvc_amd.models.vernier import VernierScale
    S_.TRAIN_EXACT_K57[0] = exact_k57
    request.addfinalizer(lambda: S_.TRAIN_EXACT_K57.__setitem__(0, False))
    grid = (16, 16, 24)
    ref = T.VernierTrunk(32, grid, gn)
    ours = VernierScale(_cfg(grid, gn))
    sd = T.seeded_state_dict(ref, 91)
    ref.load_state_dict(sd); ours.load_state_dict(sd)
    ref.train(); ours.train()
    ours = ours.to(dev())
    lf, rf, gpl, gpr = GC.trunk_inputs(2, 32, 16, 16, grid, 92)
    w_occ = GC.randn((2, 1) + grid, 93)

    def loss_ref(l, r):
        bev, occ, _ = ref.trunk_3d(T.sample_2d_feat(l, r, gpl, gpr, GC.RESOLUTION, grid))
        return bev.pow(2).mean() + (occ * w_occ).mean()

    def loss_ours(l, r):
        bev, occ, _ = ours.trunk_3d(ours.construct_voxel(l, r, gpl.to(dev()), gpr.to(dev())))
        return bev.pow(2).mean() + (occ * w_occ.to(dev())).mean()

    lr_, rr_ = lf.clone().requires_grad_(), rf.clone().requires_grad_()
    (gl_r, gr_r), gp_r = _grads(ref, [lr_, rr_], lambda: loss_ref(lr_, rr_))
    lo, ro = lf.to(dev()).requires_grad_(), rf.to(dev()).requires_grad_()
    (gl_o, gr_o), gp_o = _grads(ours, [lo, ro], lambda: loss_ours(lo, ro))

    def l2(a, b):
        return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))
    # direct kernels: 2e-3.  Winograd F(4,5) / F(4,7) forward (1e-4 of the range off, inside the 1e-3 contract): a handful of
    # ReLU masks differ from torch's, each an isolated O(1) difference in the gradient behind it -- bounded, not matched
    tol = 2e-3 if exact_k57 else 2e-2
    errs = {"left": l2(gl_o.numpy(), gl_r.numpy()), "right": l2(gr_o.numpy(), gr_r.numpy())}
    trunk = [k for k in gp_r if gp_r[k] is not None and k.split(".")[0] in
             ("vimg_feat", "conv1", "conv2", "conv3", "conv4", "hg_conv3d", "fg_cls_head")]
    assert len(trunk) >= 30
    errs.update({k: l2(gp_o[k].numpy(), gp_r[k].numpy()) for k in trunk})
    worst = max(errs, key=errs.get)
    print(f"gn={gn} exact={exact_k57}: worst l2 {errs[worst]:.2e} ({worst}), left {errs['left']:.2e}, right {errs['right']:.2e}")
    assert errs[worst] < tol, (worst, errs[worst])


def test_empty_and_ragged_inputs():
    """Edge cases: empty batches / zero voxels / zero points, W not a multiple of the 32-voxel tile
    or of 4, single-plane depth, and a conv whose last channel chunk is partial on the LAST sample
    of the allocation (no read may leave the tensor)."""
    import torch.nn.functional as F
    from snvc_amd import ops
    from snvc_amd.extension.roiaware_pool3d import roiaware_pool3d_utils as U
    from snvc_amd.models import submodule as S
    d = dev()
    with torch.no_grad():
        conv = S.HipConv3d(5, 32, 3, 1, 1, bias=False).to(d)
        assert conv(torch.zeros(0, 5, 4, 4, 8, device=d)).shape == (0, 32, 4, 4, 8)
        for shape in ((1, 5, 1, 1, 1), (1, 5, 2, 3, 33), (2, 5, 3, 5, 7)):
            x = torch.randn(shape, device=d)
            ref = F.conv3d(x.cpu(), conv.weight.cpu(), None, 1, 1)
            check(conv(x).cpu().numpy(), ref.numpy(), TIGHT, f"ragged conv {shape}")
        # channel count 1 (dgrad of the classifier): Cin smaller than every staging chunk
        c1 = S.HipConv3d(1, 32, 1, 1, 0, bias=False).to(d)
        x = torch.randn(3, 1, 4, 4, 32, device=d)
        check(c1(x).cpu().numpy(), F.conv3d(x.cpu(), c1.weight.cpu()).numpy(), TIGHT, "Cin=1")
        assert ops.voxel_gather_forward(torch.zeros(2, 4, 5, 5, device=d), torch.zeros(2, 4, 5, 5, device=d),
                                        torch.zeros(2, 2, 0, device=d), torch.zeros(2, 2, 0, device=d), (8, 8)).shape == (2, 8, 0)
        assert ops.avgpool_depth4(torch.zeros(1, 2, 3, 4, 4, device=d)).shape == (1, 2, 0, 4, 4)
        idx, val = ops.argmax_rows(torch.zeros(0, 7, device=d))
        assert idx.shape == (0,)
        with pytest.raises(RuntimeError, match="empty sequence"):
            ops.argmax_rows(torch.zeros(3, 0, device=d))
    pool = U.RoIAwarePool3d((2, 2, 2), 8)
    rois = torch.tensor([[0, 0, 0, 2, 2, 2, 0.0]], device=d)
    out = pool(rois, torch.zeros(0, 3, device=d), torch.zeros(0, 4, device=d), "max")     # no points
    assert out.shape == (1, 2, 2, 2, 4) and float(out.abs().sum()) == 0.0
    out = pool(rois[:0], torch.zeros(5, 3, device=d), torch.zeros(5, 4, device=d), "avg")  # no boxes
    assert out.shape == (0, 2, 2, 2, 4)
    assert U.points_in_boxes_gpu(torch.zeros(1, 0, 3, device=d), torch.zeros(1, 2, 7, device=d)).shape == (1, 0)


# =============================================================================== a9 + glue
def test_small_ops():
    from snvc_amd import ops
    from snvc_amd.models.submodule import disparityregression
    r = np.random.default_rng(51)
    x = torch.from_numpy(r.standard_normal((2, 12, 5, 7)).astype(np.float32))
    depth = torch.from_numpy(np.linspace(2.0, 40.0, 12).astype(np.float32))
    G = GC.load_golden()
    got = disparityregression(12, None)(GC.randn((2, 12, 5, 7), 901).to(dev()), depth.to(dev()))
    check(got.cpu().numpy(), G["disparityregression"], 1e-6, "disparityregression")
    for shape in ((2, 3, 8, 5, 12), (1, 2, 4, 3, 7), (1, 1, 9, 2, 2)):
        v = torch.from_numpy(r.standard_normal(shape).astype(np.float32))
        exp = torch.nn.AvgPool3d((4, 1, 1), stride=(4, 1, 1))(v)
        check(ops.avgpool_depth4(v.to(dev())).cpu().numpy(), exp.numpy(), 1e-6, "avgpool")
        occ = torch.from_numpy(r.random((shape[0], 1) + shape[2:]).astype(np.float32))
        assert torch.equal(ops.mul_broadcast(v.to(dev()), occ.to(dev())).cpu(), v * occ)
    h = torch.from_numpy(r.standard_normal((7, 1000)).astype(np.float32))
    h[2, 17] = h[2, 900] = 50.0          # tie -> first index
    h[3, 5] = float("nan")               # numpy: NaN wins
    idx, val = ops.argmax_rows(h.to(dev()))
    assert np.array_equal(idx.cpu().numpy(), np.argmax(h.numpy(), axis=1))
    assert idx[2].item() == 17 and idx[3].item() == 5


# =============================================================================== a10
def _roi_scene(seed, B=5, P=3000, C=6):
    r = np.random.default_rng(seed)
    rois = np.zeros((B, 7), np.float32)
    rois[:, :3] = r.uniform(-4, 4, (B, 3))
    rois[:, 3:6] = r.uniform(1.5, 5.0, (B, 3))
    rois[:, 6] = r.uniform(-np.pi, np.pi, B)
    rois[0, 6] = 0.0
    rois[1, 6] = np.pi / 2
    pts = r.uniform(-7, 7, (P, 3)).astype(np.float32)
    # >127 points inside ONE voxel of box 0 (heading 0): centre + 1/8 of the extents, tiny jitter
    pts[:200] = rois[0, :3] + 0.125 * rois[0, 3:6] + r.uniform(-0.01, 0.01, (200, 3)).astype(np.float32)
    feat = r.standard_normal((P, C)).astype(np.float32)
    feat[10:20] = feat[10]                                                          # argmax ties
    return rois, pts, feat


@pytest.mark.parametrize("method", ["max", "avg"])
@pytest.mark.parametrize("out_size", [(4, 4, 4), (3, 5, 2)])
def test_roiaware_pool3d_bit_exact(method, out_size):
    from oracle import native as O
    from snvc_amd.extension.roiaware_pool3d import roiaware_pool3d_utils as U
    rois, pts, feat = _roi_scene(61)
    e_pool, e_arg, e_lists = O.roiaware_pool3d_forward(rois, pts, feat, out_size, 128, method)
    assert e_lists[..., 0].max() == 127          # truncation is exercised
    pool = U.RoIAwarePool3d(out_size, 128)
    t_feat = torch.from_numpy(feat).to(dev()).requires_grad_()
    got = pool(torch.from_numpy(rois).to(dev()), torch.from_numpy(pts).to(dev()), t_feat, method)
    assert np.array_equal(got.detach().cpu().numpy(), e_pool)
    # the integer side outputs, bit-exact ("bit-exact voxel indices")
    lists, argmax, _, _, _ = got.grad_fn.roiaware_pool3d_for_backward
    assert np.array_equal(lists.cpu().numpy(), e_lists)
    if method == "max":
        assert np.array_equal(argmax.cpu().numpy(), e_arg)
    g = np.random.default_rng(62).standard_normal(e_pool.shape).astype(np.float32)
    got.backward(torch.from_numpy(g).to(dev()))
    e_grad = O.roiaware_pool3d_backward(e_lists, e_arg, g, pts.shape[0], method)
    np.testing.assert_allclose(t_feat.grad.cpu().numpy(), e_grad, rtol=1e-5, atol=1e-5)  # atomics: order differs


def test_roiaware_mask_codes_bit_exact():
    import ctypes
    from oracle import native as O
    from snvc_amd import _lib
    rois, pts, _ = _roi_scene(63, B=7, P=5000)
    exp = O.roiaware_mask(rois, pts, (6, 7, 5))
    # the mask lives in the op's workspace: run forward and read the workspace back
    d_rois, d_pts = torch.from_numpy(rois).to(dev()), torch.from_numpy(pts).to(dev())
    feat = torch.zeros(5000, 1, device=dev())
    ws = torch.empty(7 * 5000, dtype=torch.int32, device=dev())
    lists = torch.zeros(7, 6, 7, 5, 128, dtype=torch.int32, device=dev())
    pooled = torch.zeros(7, 6, 7, 5, 1, device=dev())
    arg = torch.zeros(7, 6, 7, 5, 1, dtype=torch.int32, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = _lib.lib().snvc_roiaware_pool3d_forward(p(d_rois), p(d_pts), p(feat), p(arg), p(lists), p(pooled), p(ws),
                                                 7, 5000, 1, 128, 6, 7, 5, 0, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(ws.cpu().numpy().reshape(7, 5000), exp)
    assert (exp >= 0).sum() > 100


def test_points_in_boxes():
    from oracle import native as O
    from snvc_amd.extension.roiaware_pool3d import roiaware_pool3d_utils as U
    rois, pts, _ = _roi_scene(64, B=6, P=4000)
    boxes = np.stack([rois, rois[::-1]])          # [2, 6, 7]
    points = np.stack([pts, pts[::-1]])           # [2, 4000, 3]
    exp = O.points_in_boxes_gpu(points, boxes)
    got = U.points_in_boxes_gpu(torch.from_numpy(points.copy()).to(dev()), torch.from_numpy(boxes.copy()).to(dev()))
    assert np.array_equal(got.cpu().numpy(), exp) and (exp >= 0).sum() > 50
    exp_cpu = O.points_in_boxes_cpu(pts, rois)
    assert np.array_equal(U.points_in_boxes_cpu(pts, rois), exp_cpu)


# =============================================================================== N3 (parity unpinned by the reference)
@pytest.mark.parametrize("align", [False, True])
def test_volume_resample_vs_grid_sample(align):
    """PSV -> 3D grid resampling: defined against 5-D F.grid_sample (trilinear, zeros padding); the
    reference ships only the helper math (snvc/utils/torch_utils.py:5-45), so torch's operator is the oracle."""
    import torch.nn.functional as F
    from snvc_amd import ops
    r = np.random.default_rng(61)
    x = torch.from_numpy(r.standard_normal((2, 5, 6, 7, 9)).astype(np.float32))
    grid = r.uniform(-1.15, 1.15, (2, 3, 4, 11, 3)).astype(np.float32)
    grid[0, 0, 0, :4] = [[-1, -1, -1], [1, 1, 1], [0, 0, 0], [1e9, 0, 0]]     # exact corners, centre, far outside
    g = torch.from_numpy(grid)
    exp = F.grid_sample(x, g, mode="bilinear", padding_mode="zeros", align_corners=align)
    got = ops.volume_resample(x.to(dev()), g.to(dev()), align_corners=align).cpu()
    assert got.shape == exp.shape == (2, 5, 3, 4, 11)
    check(got.numpy(), exp.numpy(), 1e-6, f"volume_resample align_corners={align}")
    # channel-sliced input (a view of a wider buffer) and a flat [N,V,3] grid
    big = torch.zeros(2, 8, 6, 7, 9, device=dev())
    big[:, 2:7] = x.to(dev())
    got2 = ops.volume_resample(big[:, 2:7], g.reshape(2, -1, 3).to(dev()), align_corners=align).cpu()
    assert torch.equal(got2.view_as(got), got)


def test_psv_to_grid_chain_vs_torch():
    """project_rect_to_image (torch_utils.py:37-45) + normalisation on the device, then the resampler, then
    disparityregression (submodule.py:76-83) on the same volume: the global model's read-out steps chained."""
    import torch.nn.functional as F
    from snvc_amd import ops
    r = np.random.default_rng(62)
    P = np.array([7.215377e+02, 0.0, 6.095593e+02, 4.485728e+01, 0.0, 7.215377e+02, 1.728540e+02, 2.163791e-01,
                  0.0, 0.0, 1.0, 2.745884e-03], dtype=np.float32).reshape(3, 4)
    pts = np.stack([r.uniform(-20, 20, 500), r.uniform(-1, 3, 500), r.uniform(2, 60, 500)], 1).astype(np.float32)
    origin, span = (0.0, 0.0, 2.0), (1247.0, 383.0, 58.0)
    # the reference's helper, expression by expression
    ph = torch.cat([torch.from_numpy(pts), torch.ones(500, 1)], dim=1)
    p2 = torch.mm(ph, torch.from_numpy(P).t())
    uv = torch.stack([p2[:, 0] / p2[:, 2], p2[:, 1] / p2[:, 2]], 1)
    exp = torch.stack([(uv[:, 0] - origin[0]) / span[0] * 2 - 1, (uv[:, 1] - origin[1]) / span[1] * 2 - 1,
                       (torch.from_numpy(pts)[:, 2] - origin[2]) / span[2] * 2 - 1], 1)
    grid = ops.rect_to_psv_grid(torch.from_numpy(pts).to(dev()), P, origin, span)
    assert np.abs(grid.cpu().numpy() - exp.numpy()).max() < 2e-6
    cost = torch.from_numpy(r.standard_normal((1, 1, 12, 10, 14)).astype(np.float32))
    feat = torch.from_numpy(r.standard_normal((1, 4, 12, 10, 14)).astype(np.float32))
    vox = ops.volume_resample(feat.to(dev()), grid.view(1, -1, 3), align_corners=True).cpu()
    ref = F.grid_sample(feat, grid.cpu().view(1, 1, 1, -1, 3), mode="bilinear", padding_mode="zeros", align_corners=True)
    check(vox.numpy(), ref[:, :, 0, 0].numpy(), 1e-6, "psv -> grid")
    depth = torch.linspace(2.0, 60.0, 12)
    prob = torch.softmax(cost[:, 0], dim=1)
    dm = ops.disparity_regression(prob.to(dev()), depth.to(dev())).cpu()
    check(dm.numpy(), (prob * depth.view(1, -1, 1, 1)).sum(1).numpy(), 1e-6, "disparityregression")


def test_sample_2d_feat_concat_atten_vs_torch():
    """aggregate="concat-atten" (vernier.py:341-344): concat * clamp(cosine_similarity(left, right, dim=1), 0)."""
    import torch.nn.functional as F
    from snvc_amd.models.vernier import VernierScale
    grid, gn, n, fh, fw, seed = GC.TRUNK_CASES["G1"]
    m = VernierScale(_cfg(grid, gn)).to(dev())
    lf, rf, gpl, gpr = GC.trunk_inputs(n, 32, fh, fw, grid, seed + 1)
    with torch.no_grad():
        plain = m._sample_2d_feat(lf.to(dev()), rf.to(dev()), gpl.to(dev()), gpr.to(dev())).cpu()
        got = m._sample_2d_feat(lf.to(dev()), rf.to(dev()), gpl.to(dev()), gpr.to(dev()), aggregate="concat-atten").cpu()
    att = F.cosine_similarity(plain[:, :32], plain[:, 32:], dim=1).unsqueeze(1)
    check(got.numpy(), (plain * torch.clamp(att, 0.0)).numpy(), 2e-6, "concat-atten")


@pytest.mark.parametrize("shape", [(2, 5, 8, 3, 7), (1, 32, 32, 16, 24), (1, 3, 10, 4, 4), (2, 2, 3, 5, 6)])
def test_avgpool_depth4_autograd_vs_torch(shape):
    """r5: the pool in front of the BEV reshape under autograd (reference vernier.py:289,436) on the HIP kernels in both
    directions -- forward bit-equal to F.avg_pool3d's fp32 sum order, backward = grad / 4 on the pooled planes and zero on the
    planes the floor drops (depth 10 -> 2 windows, depth 3 -> none)."""
    from snvc_amd import ops
    torch.manual_seed(sum(shape))
    x = torch.randn(*shape, device=dev(), requires_grad=True)
    xr = x.detach().clone().requires_grad_()
    y = ops.AvgPoolDepth4Fn.apply(x)
    import torch.nn.functional as F
    yr = F.avg_pool3d(xr, (4, 1, 1), (4, 1, 1)) if shape[2] >= 4 else xr.new_zeros(shape[:2] + (0,) + shape[3:]) + 0.0 * xr.sum()
    assert y.shape == yr.shape
    g = torch.randn_like(y)
    y.backward(g)
    yr.backward(g)
    assert torch.allclose(y, yr, rtol=0, atol=1e-6)
    assert torch.equal(x.grad, xr.grad)
