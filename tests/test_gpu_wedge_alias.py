"""The aliased wedge duplicates (GlobalStack.alias_wedge; include/snvc_alias.h): conv2's fused launch neither computes nor copies its
duplicate tiles, and the one reader of each result -- the hourglass's first stride-2 layer (conv3d_x3s2q_kernel<1>) for the pair, the
tail's gather (deconv_tail_gather_alias_kernel) for the side head -- reads the representative's row where a duplicate's would be.

Every comparison is torch.equal against the plain launches.  The aliased conv2 writes into buffers pre-filled with NaN (0x7E00 in the
pair, a float NaN in the side head): a duplicate row that still holds the poison was written by nobody, and a reader that looked at
one would return NaN where the plain launch returns a number.

Shapes (N 2, C 32, H 8, all multiples of 4 where the gather runs): q 1, D 96, W 72 -- duplicates in two tile columns of different
length beside a partial third; q 2, D 148, W 72 -- half-pixel planes, one long and one two-tile column; q 1, D 96, W 40 -- one
column; D 10 -- no duplicate, the aliased readers are the plain ones.  The 16x16x32 forms are forced through their job threshold as
tests/test_gpu_wedge_dedup.py does.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H = 2, 32, 8
# name -> (D, W, q, m0, has duplicates)
CASES = {
    "q1_two_columns": (96, 72, 1, 0, True),
    "q2_half_pixel": (148, 72, 2, 0, True),
    "q1_one_column": (96, 40, 1, 0, True),
    "no_duplicates": (10, 40, 1, 0, False),
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


def duplicate_mask(d, w, q, m0, off):
    """[D, W] bool on the device: the voxels of the duplicate tiles, from the host query."""
    from snvc_amd import ops
    dups, first, last = ops.fused_first_wedge_tiles(d, w, q, m0, off)
    m = torch.zeros(d, w, dtype=torch.bool)
    for tw, (f, l) in enumerate(zip(first, last)):
        if f >= 0:
            m[4 * (f + 1):4 * l + 4, 32 * tw:32 * tw + 32] = True
    assert int(m.sum()) == dups * 4 * 32
    return dups, m.to(dev())


def alias_case(name, mul=1.0, seed=9):
    """One shape end to end, per operator: conv2 plain and aliased (into poisoned buffers), the stride-2 layer plain on the plain pair and
    aliased on the poisoned one, the gather plain on the plain side head and aliased on the poisoned one.  Asserts (a), (b), (d) of the
    module's text; also what tests/test_gpu_guard_wedge_alias.py runs between guard bands."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    d, w, q, m0, has = CASES[name]
    torch.manual_seed(seed)
    left = torch.randn(N, C, H, w, device=dev())
    right = torch.randn(N, C, H, w, device=dev())
    lay_p = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 3, device=dev()) * 0.06)
    lay_g = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04)
    lay_c = ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04)
    conv2 = ops.Conv3dLayerX3(torch.randn(C, C, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (C * 27)))
    h1 = ops.Conv3dLayerX3(torch.randn(2 * C, C, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (C * 27)), 3, 2, 1, 1, False)
    v_sc = ((torch.rand(C, device=dev()) + 0.5) * mul).contiguous()
    v_bi = (torch.randn(C, device=dev()) * 0.3 * mul).contiguous()
    sc2, bi2 = torch.rand(C, device=dev()) + 0.5, torch.randn(C, device=dev()) * 0.3
    sc3, bi3 = torch.rand(2 * C, device=dev()) + 0.5, torch.randn(2 * C, device=dev()) * 0.3
    head = torch.randn(C, device=dev()) * 0.2
    off, wu, off_col, wu_col = sheared_geometry(q, m0, d, w)
    pitch, lp = ops.fused_il_geometry(q, m0, d, w, wu, off, wu_col, off_col)
    _, p_il = ops.planes_x3_il(left, lay_p, {})
    _, _, gi = ops.sheared_prep_x3_il(right, q, wu, off, wu_col, off_col, lay_g, lay_c, {}, pitch, lp)
    dups, mask = duplicate_mask(d, w, q, m0, off)
    assert (dups > 0) == has
    desc = ops.wedge_desc(d, w, q, m0, off)

    # (a) conv2: the plain launch against the aliased one into poison
    def run_conv2(alias):
        f = torch.zeros(1, dtype=torch.int32, device=dev())
        out = torch.full((N, 2, C // 8, d, H, w, 8), float("nan"), dtype=torch.float16, device=dev())
        hv = torch.full((N, 1, d, H, w), float("nan"), dtype=torch.float32, device=dev())
        y, h = conv2.forward_fused_first(gi, pitch, lp, p_il, v_sc, v_bi, q, m0, off, off_col, ops.EPI_RELU, N, (d, H, w), x_exp=2, scale=sc2,
                                         bias=bi2, flags=ops.EPI_RELU, out_exp=1, head=head, overflow=f, alias=alias, out=out, head_out=hv)
        return y, h, f
    (y0, hv0, f0), (y1, hv1, f1) = run_conv2(False), run_conv2(True)
    assert torch.isfinite(y0.float()).all() and y0.float().abs().max() > 0 and torch.isfinite(hv0).all()
    my, mh = mask[None, None, None, :, None, :, None], mask[None, None, :, None, :]
    assert torch.equal(torch.where(my, y0, y1), y0) and torch.equal(torch.where(mh, hv0, hv1), hv0)      # written rows: the plain launch's
    if has:                                                                                              # duplicate rows: nobody wrote them
        assert bool((y1.view(torch.int16)[my.expand_as(y1)] == 0x7E00).all()) and bool(torch.isnan(hv1[mh.expand_as(hv1)]).all())
    assert int(f1.item()) == int(f0.item()) == (1 if mul > 1.0 else 0)

    # (b) the stride-2 layer: aliased on the poisoned pair against plain on the plain pair
    g0, g1 = (torch.zeros(1, dtype=torch.int32, device=dev()) for _ in range(2))
    o0 = h1(y0, 1, sc3, bi3, flags=ops.EPI_RELU, out_exp=0, overflow=g0)
    o1 = h1.forward_aliased(y1, desc, 1, sc3, bi3, flags=ops.EPI_RELU, out_exp=0, overflow=g1)
    assert h1.algo == ops._lib.ALGO_X3_Q16
    assert torch.isfinite(o0.float()).all() and o0.float().abs().max() > 0
    assert torch.equal(o1, o0) and int(g1.item()) == int(g0.item())

    # (d) the gather: aliased on the poisoned side head against plain on the plain one
    res = {}
    if d % 4 == 0:
        t = torch.randn(N, 27, 8, d // 4, H // 4, w // 4, device=dev())
        b = torch.randn(1, device=dev())
        c0 = ops.deconv_tail_gather(t, b, hv0)
        c1 = ops.deconv_tail_gather(t, b, hv1, res_alias=desc)
        assert torch.isfinite(c0).all() and torch.equal(c1, c0)
        res = dict(cost=c0)
    return dict(y=y0, hv=hv0, o=o0, dups=dups, **res)


@pytest.mark.parametrize("name", list(CASES))
def test_aliased_readers_return_the_plain_launches_bits_and_nobody_writes_a_duplicate(name):
    alias_case(name)


def test_clamped_first_layer_raises_the_flag_on_both_sides():
    """An affine 2^14 times too large: v1 clamps inside the skipped tiles' images too -- their representative raises the same flag."""
    alias_case("q1_one_column", mul=16384.0)


def test_a_form_without_the_aliased_read_is_refused_with_its_message_and_launches_nothing():
    """(e): the stride-2 layer off its persistent form, and a stride-1 layer: Unsupported, the result buffer untouched."""
    from snvc_amd import ops
    d, w = 96, 40
    desc = ops.wedge_desc(d, w, 1, 0, 4)
    x = torch.zeros(N, 2, C // 8, d, H, w, 8, dtype=torch.float16, device=dev())
    h1 = ops.Conv3dLayerX3(torch.randn(2 * C, C, 3, 3, 3, device=dev()) * 0.05, 3, 2, 1, 1, False)
    s1 = ops.Conv3dLayerX3(torch.randn(C, C, 3, 3, 3, device=dev()) * 0.05)
    old = ops.X3_Q16_S2[0]
    ops.X3_Q16_S2[0] = False
    try:
        out = torch.full((N, 2, 2 * C // 8, d // 2, H // 2, w // 2, 8), float("nan"), dtype=torch.float16, device=dev())
        with pytest.raises(ops.Unsupported, match="stride-2 3x3x3 layer on the 16x16x32 form"):
            h1.forward_aliased(x, desc, out=out)
        assert bool((out.view(torch.int16) == 0x7E00).all())
    finally:
        ops.X3_Q16_S2[0] = old
    out = torch.full((N, 2, C // 8, d, H, w, 8), float("nan"), dtype=torch.float16, device=dev())
    with pytest.raises(ops.Unsupported, match="stride-2 3x3x3 layer on the 16x16x32 form"):
        s1.forward_aliased(x, desc, out=out)
    assert bool((out.view(torch.int16) == 0x7E00).all())
    with pytest.raises(RuntimeError, match=r"in_alias describes a \[Din\]"):      # a descriptor of another tensor
        h1.forward_aliased(x, ops.wedge_desc(d + 4, w, 1, 0, 4))
    t = torch.zeros(N, 27, 8, d // 4, H // 4, w // 4, device=dev())
    with pytest.raises(RuntimeError, match="res_alias describes the residual"):
        ops.deconv_tail_gather(t, None, torch.zeros(N, 1, d, H, w, device=dev()), res_alias=ops.wedge_desc(d, w + 4, 1, 0, 4))


@pytest.fixture(scope="module")
def stack():
    import bench
    from snvc_amd.models.stereo_volume import GlobalStack
    m = GlobalStack(C)
    m.load_state_dict(bench.seeded_state(m, 11))
    return m.eval().to(dev())


@pytest.mark.parametrize("d,q", [(96, 1), (148, 2)])
def test_forward_pair_aliased_copied_and_computed(stack, d, q):
    """H 8, W 72: alias_wedge True against False (the copy route) against dedup_wedge False (every tile computed), and the aliased route
    not taken when the stride-2 layer leaves its persistent form (there the copy route's result against the all-computed one)."""
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    hm, w, m0 = 8, 72, 0
    assert stack.alias_wedge and stack.dedup_wedge and stack.fused_first                      # the defaults under test
    assert ops.fused_first_wedge_tiles(d, w, q, m0, 4)[0] > 0
    g = np.random.default_rng(5)
    left = torch.from_numpy(g.standard_normal((N, C, hm, w)).astype(np.float32)).to(dev())
    right = torch.from_numpy(g.standard_normal((N, C, hm, w)).astype(np.float32)).to(dev())
    shift = torch.from_numpy(((m0 + np.arange(d, dtype=np.float32)) / q)[None].repeat(N, 0)).to(dev())
    got = {}
    with torch.no_grad():
        for key, attrs, s2 in (("alias", {}, True), ("copy", {"alias_wedge": False}, True), ("plain", {"dedup_wedge": False}, True),
                               ("no_s2_form", {}, False), ("no_s2_form_plain", {"dedup_wedge": False}, False)):
            for k, v in attrs.items():
                setattr(stack, k, v)
            old = ops.X3_Q16_S2[0]
            ops.X3_Q16_S2[0] = s2
            try:
                before = S._ROUTES["fused_first_conv"], S._ROUTES["wedge_alias"]
                got[key] = stack.forward_pair(left, right, shift, 1).clone()
                assert S._ROUTES["fused_first_conv"] - before[0] == 1
                assert S._ROUTES["wedge_alias"] - before[1] == (1 if key == "alias" else 0)
            finally:
                ops.X3_Q16_S2[0] = old
                for k in attrs:
                    stack.__dict__.pop(k, None)                         # the class defaults stay
    assert torch.isfinite(got["alias"]).all()
    for key in ("copy", "plain"):
        assert torch.equal(got["alias"], got[key]), key
    # the serial-plane form sums in another order than the persistent one (csrc/conv3d_f16.hip): equal among its own routes
    assert torch.isfinite(got["no_s2_form"]).all() and torch.equal(got["no_s2_form"], got["no_s2_form_plain"])
