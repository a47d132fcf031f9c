"""The wedge deduplication of the fused first layer (GlobalStack.dedup_wedge; include/snvc_dedup.h; csrc/conv3d_f16.hip,
conv3d_x3q_kernel<EPI, 1> with SRC_DEDUP + wedge_copy_kernel): conv2's tiles whose whole input image lies left of the image's first
column on interior planes are computed once per (n, th, tw) and copied to their duplicates.  The deduplicated launch must store the
bits of the plain fused launch -- the pair, the side head and the overflow word -- so every comparison here is torch.equal.

Shapes (N 2, C 32, H 6: tile rows 4 + 2): the smallest at which a tile column has duplicates -- the rule needs
q * (w0 + 32) - (d0 - 1) - m0 + 4 < 0, i.e. more than 36 planes in front of the first duplicate at m0 = 0 -- and every way a column can
lose them: (a) one full column with 12 duplicates beside the partial last column; (b) m0 = 60: duplicates in two columns, of
different length, the third excluded; (c) half-pixel planes; (d) no ReLU in the first layer; (e) too few planes for any (the launcher
walks the same rule as the query: zero duplicates there is no copy launch).  The 16x16x32 form is forced through its job threshold as tests/test_gpu_fused_first_layer.py does.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H = 2, 32, 6
# name -> (D, W, q, m0, relu, duplicates per (n, th))
CASES = {
    "a_one_column": (96, 40, 1, 0, True, 12),
    "b_two_columns_m60": (40, 72, 1, 60, True, None),
    "c_half_pixel": (80, 72, 2, 5, True, None),
    "d_no_relu": (96, 40, 1, 0, False, 12),
    "e_no_duplicates": (10, 40, 1, 0, True, 0),
}


def dev():
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def q16_everywhere():
    from snvc_amd import ops
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    yield
    ops.X3_Q16_MIN_JOBS[0] = old


def wedge_case(d, w, q, m0, relu=True, mul=1.0, seed=9):
    """conv2 + side head through ``ops`` from one set of prep launches, ``dedup=True`` against ``dedup=False``, built like
    test_gpu_fused_first_layer._ops_case.  Returns a dict of tensors and the host query's answer."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    torch.manual_seed(seed)
    left = torch.randn(N, C, H, w, device=dev())
    right = torch.randn(N, C, H, w, device=dev())
    lay_p = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 3, device=dev()) * 0.06)
    lay_g = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04)
    lay_c = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04)
    conv2 = ops.Conv3dLayerX3(torch.randn(C, C, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (C * 27)))
    v_sc = ((torch.rand(C, device=dev()) + 0.5) * mul).contiguous()
    v_bi = (torch.randn(C, device=dev()) * 0.3 * mul).contiguous()
    sc2, bi2 = torch.rand(C, device=dev()) + 0.5, torch.randn(C, device=dev()) * 0.3
    head = torch.randn(C, device=dev()) * 0.2
    off, wu, off_col, wu_col = sheared_geometry(q, m0, d, w)
    pitch, lp = ops.fused_il_geometry(q, m0, d, w, wu, off, wu_col, off_col)
    _, p_il = ops.planes_x3_il(left, lay_p, {})
    _, _, gi = ops.sheared_prep_x3_il(right, q, wu, off, wu_col, off_col, lay_g, lay_c, {}, pitch, lp)
    flags = ops.EPI_RELU if relu else 0
    out = {}
    for on in (False, True):
        f = torch.zeros(1, dtype=torch.int32, device=dev())
        y, h = conv2.forward_fused_first(gi, pitch, lp, p_il, v_sc, v_bi, q, m0, off, off_col, flags, N, (d, H, w), x_exp=2, scale=sc2, bias=bi2,
                                         flags=ops.EPI_RELU, out_exp=1, head=head, overflow=f, dedup=on)
        out[on] = (y, h, f)
    return dict(plain=out[False], dedup=out[True], tiles=ops.fused_first_wedge_tiles(d, w, q, m0, off))


def wedge_check(name, mul=1.0):
    """One case of CASES: the duplicate count the host query gives, then the pair, the side head and the overflow word bit for bit.
    Also what tests/test_gpu_guard_wedge_dedup.py runs between guard bands."""
    d, w, q, m0, relu, want = CASES[name]
    r = wedge_case(d, w, q, m0, relu, mul)
    dups, first, last = r["tiles"]
    if want is not None:
        assert dups == want
    if want != 0:
        assert dups > 0 and first[0] >= 0 and last[0] > first[0]          # the comparison below is not vacuous
    (y0, h0, f0), (y1, h1, f1) = r["plain"], r["dedup"]
    assert torch.isfinite(y0.float()).all() and y0.float().abs().max() > 0
    if dups:      # the wedge is not a region of zeros: a duplicate row holds values, and they are the representative's
        row = y0[:, :, :, 4 * last[0], :, :32]
        assert row.float().abs().max() > 0 and torch.equal(row, y0[:, :, :, 4 * first[0], :, :32])
    assert torch.equal(y1, y0) and torch.equal(h1, h0)
    assert int(f1.item()) == int(f0.item()) == (1 if mul > 1.0 else 0)
    return r


@pytest.mark.parametrize("name", list(CASES))
def test_deduplicated_launch_stores_the_plain_launch_s_bits(name):
    r = wedge_check(name)
    dups, first, last = r["tiles"]
    if name == "b_two_columns_m60":
        assert first[1] >= 0 and last[1] - first[1] != last[0] - first[0] and first[2] == last[2] == -1
    if name == "a_one_column":
        assert (first, last) == ([10, -1], [22, -1])


def test_clamped_first_layer_raises_the_flag_on_both_sides():
    """An affine 2^14 times too large (test_clamped_first_layer_raises_the_flag_and_stores_the_same_bits): v1 clamps at 65504 inside
    the skipped tiles' images too -- their representative raises the same flag."""
    wedge_check("a_one_column", mul=16384.0)


@pytest.fixture(scope="module")
def stack():
    import bench
    from snvc_amd.models.stereo_volume import GlobalStack
    m = GlobalStack(C)
    m.load_state_dict(bench.seeded_state(m, 11))
    return m.eval().to(dev())


@pytest.mark.parametrize("q,m0", [(1, 0), (2, 0)])
def test_forward_pair_with_and_without_the_wedge_and_unfused(stack, q, m0):
    """H 8, W 40, D 96 (multiples of 4: the hourglass): dedup_wedge True against False against the unfused route."""
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    hm, w, d = 8, 40, 96
    assert stack.dedup_wedge and stack.fused_first                      # the defaults under test
    assert ops.fused_first_wedge_tiles(d, w, q, m0, 4)[0] > 0
    g = np.random.default_rng(5)
    left = torch.from_numpy(g.standard_normal((N, C, hm, w)).astype(np.float32)).to(dev())
    right = torch.from_numpy(g.standard_normal((N, C, hm, w)).astype(np.float32)).to(dev())
    shift = torch.from_numpy(((m0 + np.arange(d, dtype=np.float32)) / q)[None].repeat(N, 0)).to(dev())
    got = {}
    with torch.no_grad():
        for key, attrs in (("dedup", {}), ("plain", {"dedup_wedge": False}), ("unfused", {"fused_first": False})):
            for k, v in attrs.items():
                setattr(stack, k, v)
            try:
                before = S._ROUTES["fused_first_conv"]
                got[key] = stack.forward_pair(left, right, shift, 1).clone()
                assert S._ROUTES["fused_first_conv"] - before == (0 if key == "unfused" else 1)
            finally:
                for k in attrs:
                    stack.__dict__.pop(k, None)                         # the class defaults stay
    assert torch.isfinite(got["dedup"]).all()
    assert torch.equal(got["dedup"], got["plain"]) and torch.equal(got["dedup"], got["unfused"])
