"""The fused sheared first layer (GlobalStack.fused_first; csrc/conv3d_f16.hip, conv3d_x3q_kernel<EPI, 1>): conv2's launch forms the
first layer's split pair itself instead of reading what the expand pass stored.  The two routes must agree BIT FOR BIT -- the
production is the expand kernel's arithmetic, operation for operation -- so every comparison here is torch.equal.

Shapes.  Through ``ops`` (conv2's pair and side head on both routes): features [2, 32, 6, 40], 10 planes: tile rows 4 + 2; two W
tiles, the last column in a partial tile and columns past the tensor; three depth tiles (d = 0, d = D - 1, and one with neither).
Through ``forward_pair`` the hourglass behind conv2 halves depth and height twice and doubles them back, so both must be multiples
of 4 there (6 rows or 10 planes fail in the hourglass on either route): 8 rows and 12 planes -- three depth tiles again, two W
tiles, the partial tiles left to the ``ops`` cases.  The 16x16x32 form is forced through its job threshold (as
test_gpu_epilogue_paths.py does) and the threshold restored.
"""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H, W, D = 2, 32, 6, 40, 10
HM, DM = 8, 12      # forward_pair: multiples of 4 (the hourglass)


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def q16_everywhere():
    from snvc_amd import ops
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    yield
    ops.X3_Q16_MIN_JOBS[0] = old


@pytest.fixture(scope="module")
def stack():
    import bench
    from snvc_amd.models.stereo_volume import GlobalStack
    m = GlobalStack(C)
    m.load_state_dict(bench.seeded_state(m, 11))
    return m.eval().to(dev())


def _pair(q, m0, d=DM, seed=5, mul=1.0):
    g = np.random.default_rng(seed)
    left = torch.from_numpy(g.standard_normal((N, C, HM, W)).astype(np.float32) * mul).to(dev())
    right = torch.from_numpy(g.standard_normal((N, C, HM, W)).astype(np.float32) * mul).to(dev())
    shift = torch.from_numpy(((m0 + np.arange(d, dtype=np.float32)) / q)[None].repeat(N, 0)).to(dev())
    return left, right, shift


def _both(m, args, **kw):
    """(fused result, unfused result, fused launches counted, expand passes counted)."""
    from snvc_amd.models import submodule as S
    out = []
    with torch.no_grad():
        for on in (True, False):
            m.fused_first = on
            try:
                b = (S._ROUTES["fused_first_conv"], S._ROUTES["sheared_first_conv"])
                y = m.forward_pair(*args, 1, **kw).clone()
                out.append((y, S._ROUTES["fused_first_conv"] - b[0], S._ROUTES["sheared_first_conv"] - b[1]))
            finally:
                m.__dict__.pop("fused_first", None)                 # the class default stays
    return out


@pytest.mark.parametrize("q,m0", [(1, 0), (2, 0), (1, 3), (2, 5)])
def test_forward_pair_is_bit_identical_and_takes_the_fused_launch(stack, q, m0):
    (y1, f1, s1), (y0, f0, s0) = _both(stack, _pair(q, m0))
    assert (f1, s1) == (1, 1) and (f0, s0) == (0, 1)          # both are the sheared route; only the first fuses
    assert torch.isfinite(y1).all() and torch.equal(y1, y0)


def test_last_first_layer_is_still_available(stack):
    """The fused route never stores v1; ``last_first_layer()`` forms it on demand from the operands the call left behind."""
    args = _pair(2, 0)
    with torch.no_grad():
        stack.fused_first = True
        try:
            stack.forward_pair(*args, 1)
            v1f = stack.last_first_layer().clone()
            stack.fused_first = False
            stack.forward_pair(*args, 1)
            v1u = stack.last_first_layer().clone()
        finally:
            stack.__dict__.pop("fused_first", None)
    assert torch.equal(v1f, v1u)


def _ops_case(q, m0, d, relu=True, mul=1.0, seed=9, narrow=0):
    """conv2 + side head through ``ops`` on both routes, from the same prep launches.  Returns a dict of tensors.  ``narrow``: G is
    computed ``narrow`` columns narrower than the geometry asks for, so that the last columns' indices run past its rows."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    torch.manual_seed(seed)
    left = torch.randn(N, C, H, W, device=dev())
    right = torch.randn(N, C, H, W, device=dev())
    lay_p = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 3, device=dev()) * 0.06)
    lay_g = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04)
    lay_c = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04)
    conv2 = ops.Conv3dLayerX3(torch.randn(C, C, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (C * 27)))
    v_sc = ((torch.rand(C, device=dev()) + 0.5) * mul).contiguous()
    v_bi = (torch.randn(C, device=dev()) * 0.3 * mul).contiguous()
    sc2, bi2 = torch.rand(C, device=dev()) + 0.5, torch.randn(C, device=dev()) * 0.3
    head = torch.randn(C, device=dev()) * 0.2
    off, wu, off_col, wu_col = sheared_geometry(q, m0, d, W)
    wu -= narrow
    pitch, lp = ops.fused_il_geometry(q, m0, d, W, wu, off, wu_col, off_col)
    planes, p_il = ops.planes_x3_il(left, lay_p, {})
    g, gcol, gi = ops.sheared_prep_x3_il(right, q, wu, off, wu_col, off_col, lay_g, lay_c, {}, pitch, lp)
    flags = ops.EPI_RELU if relu else 0
    e1, e2 = 2, 1
    f_u = torch.zeros(1, dtype=torch.int32, device=dev())
    f_f = torch.zeros(1, dtype=torch.int32, device=dev())
    v1s = torch.empty((N, 2, C // 8, d, H, W, 8), dtype=torch.float16, device=dev())
    ops.sheared_expand_split(g, gcol, planes.view(N, C, 3, H, W), v_sc, v_bi, v1s, q, m0, off, off_col, flags, f_u)
    y_u, h_u = conv2(v1s, e1, sc2, bi2, flags=ops.EPI_RELU, out_exp=e2, head=head, overflow=f_u)
    y_f, h_f = conv2.forward_fused_first(gi, pitch, lp, p_il, v_sc, v_bi, q, m0, off, off_col, flags, N, (d, H, W), x_exp=e1, scale=sc2, bias=bi2,
                                         flags=ops.EPI_RELU, out_exp=e2, head=head, overflow=f_f)
    return dict(g=g, gcol=gcol, gi=gi, planes=planes, p_il=p_il, lp=lp, wu=wu, wu_col=wu_col, y_u=y_u, y_f=y_f, h_u=h_u, h_f=h_f,
                f_u=f_u, f_f=f_f, v1s=v1s, i_lo=-(d - 1) - m0 + off, i_hi=q * (W - 2) - m0 + off)


@pytest.mark.parametrize("q,m0,relu,narrow", [(1, 0, True, 0), (2, 1, True, 0), (1, 0, True, 8), (2, 0, False, 0)])
def test_conv2_pair_and_side_head_through_ops(q, m0, relu, narrow):
    """narrow = 8: G has 40 columns and its index runs from -5 (w = 0, d = 9) to 42 (w = W - 2, d = 0): out of the row on both sides
    (both routes then read 0)."""
    r = _ops_case(q, m0, D, relu, narrow=narrow)
    assert r["i_lo"] < 0
    if narrow:
        assert r["i_hi"] >= r["wu"]
    # the interleaved operands are the fp32 ones, regrouped; zero around the rows
    lp, wu, wu_col = r["lp"], r["wu"], r["wu_col"]
    gi = r["gi"]
    assert torch.equal(gi[:, :3, :, :, lp:lp + wu], r["g"].view(N, 3, C // 8, 8, H, wu).permute(0, 1, 2, 4, 5, 3))
    assert torch.equal(gi[:, 3:, :, :, lp:lp + wu_col], r["gcol"].view(N, 3, C // 8, 8, H, wu_col).permute(0, 1, 2, 4, 5, 3))
    assert not gi[:, :, :, :, :lp].any() and not gi[:, :3, :, :, lp + wu:].any() and not gi[:, 3:, :, :, lp + wu_col:].any()
    assert torch.equal(r["p_il"], r["planes"].view(N, C // 8, 8, 3, H, W).permute(0, 3, 1, 4, 5, 2))
    assert int(r["f_u"].item()) == 0 and int(r["f_f"].item()) == 0
    assert r["v1s"].float().abs().max() > 0
    assert torch.equal(r["y_f"], r["y_u"]) and torch.equal(r["h_f"], r["h_u"])


def test_clamped_first_layer_raises_the_flag_and_stores_the_same_bits():
    """An affine 2^14 times too large: v1 clamps at 65504 in the expand pass and in the fused production alike."""
    r = _ops_case(1, 0, D, mul=16384.0)
    assert r["v1s"][:, 0].float().abs().max() == 65504.0
    assert int(r["f_u"].item()) == 1 and int(r["f_f"].item()) == 1
    assert torch.equal(r["y_f"], r["y_u"]) and torch.equal(r["h_f"], r["h_u"])


@pytest.mark.parametrize("check", ["call", "deferred"])
def test_overflowing_features_return_what_the_unfused_route_returns(check):
    """Features 4096 times what the first layer's statistics promise: v1 clamps.  ``"call"`` (arithmetic="auto"): both routes are
    flagged inside the call and redone on the fp32 kernels (tests/test_gpu_overflow.py); ``"deferred"``: both return the clamped
    split-mode result -- the same bits."""
    import bench
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    args = _pair(2, 0, mul=4096.0)
    got = []
    for on in (True, False):
        m = GlobalStack(C)
        m.load_state_dict(bench.seeded_state(m, 11))
        m = m.eval().to(dev())
        m.fused_first = on
        m.overflow_check = check
        redo, fused = S._ROUTES["x3_overflow_redo"], S._ROUTES["fused_first_conv"]
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got.append(m.forward_pair(*args, 1).clone())
            assert S._ROUTES["fused_first_conv"] == fused + int(on)
            if check == "call":
                assert S._ROUTES["x3_overflow_redo"] == redo + 1 and m.__dict__.get("_snvc_x3_off")
            else:
                assert m.check_overflow() is True          # the flag this call raised
    assert torch.isfinite(got[0]).all() and torch.equal(got[0], got[1])


def test_routes_that_keep_the_expand_pass(stack):
    """GroupNorm, quarter-pixel spacing (q = 4), arithmetic="fp32" and the any-shift path never take the fused launch."""
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    before = S._ROUTES["fused_first_conv"]
    with torch.no_grad():
        assert stack.fused_first                                     # the default under test
        stack.forward_pair(*_pair(4, 0), 1)                          # q = 4
        stack.forward_pair(*_pair(2, 0), 1, arithmetic="fp32")
        l, r, s = _pair(2, 0)
        stack.forward_pair(l, r, s * 0.73 + 0.1, 1)                  # no uniform spacing: the commuted path
        stack.forward_pair(l, r, s, 1, sheared=False)
        gn = GlobalStack(C, gn=True).eval().to(dev())
        gn.forward_pair(l, r, s, 1)
        assert S._ROUTES["fused_first_conv"] == before
        stack.forward_pair(l, r, s, 1)
        assert S._ROUTES["fused_first_conv"] == before + 1
