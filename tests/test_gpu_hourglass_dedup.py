"""The hourglass's duplicate tiles (GlobalStack.dedup_hourglass; include/snvc_hgdedup.h): on the alias route the hourglass's first
stride-2 layer (conv3d_x3s2q_kernel<2>) walks its live tiles only, and hg conv2 -- the one reader of its result
(conv3d_x3q_kernel<0, 2>) -- reads the representative's rows where a duplicate's would be.

Every comparison is torch.equal against the plain launches.  The stride-2 layer writes into a pair pre-filled with NaN (0x7E00): a
duplicate row that still holds the poison was written by nobody, and a reader that looked at one would return NaN where the plain
launch returns a number.

Shapes (N 2, C 32, H 8): q 1, D 96, W 72 -- one tile column with 4 duplicates; q 2, D 148, W 72 -- half-pixel planes, a column of one
duplicate; q 1, D 160, W 132 -- two columns, 20 and 4 duplicates; D 10, W 40 -- none, the new entry points are the plain ones.  The
counts are the host query's (tests/test_hourglass_dedup_host.py walks it against the rule) and are asserted here.  The 16x16x32 forms
are forced through their job threshold as tests/test_gpu_wedge_alias.py does.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, C, H = 2, 32, 8
# name -> (D, W, q, m0, duplicates per (n, th) by tile column)
CASES = {
    "q1_one_column": (96, 72, 1, 0, [4]),
    "q2_half_pixel": (148, 72, 2, 0, [1]),
    "q1_two_columns": (160, 132, 1, 0, [20, 4]),
    "no_duplicates": (10, 40, 1, 0, []),
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


def duplicate_mask(desc, want):
    """[OD, OW] bool on the device: the voxels of the stride-2 result's duplicate tiles, from the host query."""
    from snvc_amd import ops
    od, ow = (desc.D - 1) // 2 + 1, (desc.W - 1) // 2 + 1
    dups, first, last = ops.hg_dedup_tiles(desc)
    assert [l - f for f, l in zip(first, last) if f >= 0] == want and dups == sum(want)       # no case passes vacuously
    m = torch.zeros(od, ow, dtype=torch.bool)
    for tw, (f, l) in enumerate(zip(first, last)):
        if f >= 0:
            m[2 * (f + 1):2 * l + 2, 32 * tw:32 * tw + 32] = True
    assert int(m.sum()) == sum(2 * n * min(32, ow - 32 * tw) for tw, n in enumerate(want))
    return dups, m.to(dev())


def hg_case(name, mul=1.0, seed=9):
    """One shape, per operator: the stride-2 layer plain on a full pair and deduplicated into poison; the stride-1 layer plain on the
    plain result and aliased on the poisoned one.  Also what tests/test_gpu_guard_hourglass_dedup.py runs between guard bands."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    d, w, q, m0, want = CASES[name]
    torch.manual_seed(seed)
    off = sheared_geometry(q, m0, d, w)[0]
    desc = ops.wedge_desc(d, w, q, m0, off)
    dups, mask = duplicate_mask(desc, want)
    od, oh, ow = (d - 1) // 2 + 1, (H - 1) // 2 + 1, (w - 1) // 2 + 1
    # a pair with conv2's property and nothing else: d-invariant where the rule says so.  Voxel (dd, ., ww) is d-invariant when the
    # rule's four bounds hold; there plane dd holds plane (first marked plane of the column) + ((dd - that) & 3)'s bits, like a pair
    # that conv2's 4-plane tiles wrote.
    dd, ww = torch.arange(d)[:, None], torch.arange(w)[None, :]
    marked = (dd >= 2) & (dd <= d - 3) & (ww + 1 < w - 1) & (q * (ww + 1) - (dd - 1) - m0 + off < 0)
    first_marked = torch.where(marked, dd.expand(d, w), torch.full((d, w), d)).min(dim=0).values               # [W]
    src = torch.where(marked, first_marked[None, :] + ((dd - first_marked[None, :]) & 3), dd.expand(d, w))    # [D, W]
    val = torch.randn(N, C, d, H, w).gather(2, src[None, None, :, None, :].expand(N, C, d, H, w))
    x = ops.to_split(val.to(dev()), 1)
    # what snvc_alias.h's conv2 leaves behind: its own duplicate rows unwritten (here: poisoned), read through in_alias
    alias_rows = torch.tensor([[ops.wedge_alias_depth(desc, a, b) != a for b in range(0, w, 32)] for a in range(d)])
    alias_rows = alias_rows.repeat_interleave(32, dim=1)[:, :w].to(dev())
    x_poison = torch.where(alias_rows[None, None, None, :, None, :, None], torch.full_like(x, float("nan")), x)
    h1 = ops.Conv3dLayerX3(torch.randn(2 * C, C, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (C * 27)), 3, 2, 1, 1, False)
    h2 = ops.Conv3dLayerX3(torch.randn(2 * C, 2 * C, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (2 * C * 27)))
    sc1, bi1 = (torch.rand(2 * C, device=dev()) + 0.5) * mul, torch.randn(2 * C, device=dev()) * 0.3
    sc2, bi2 = torch.rand(2 * C, device=dev()) + 0.5, torch.randn(2 * C, device=dev()) * 0.3

    # hg conv1: plain on the full pair; deduplicated on the poisoned pair, into poison
    g0, g1 = (torch.zeros(1, dtype=torch.int32, device=dev()) for _ in range(2))
    o0 = h1(x, 1, sc1, bi1, flags=ops.EPI_RELU, out_exp=0, overflow=g0)
    out = torch.full((N, 2, 2 * C // 8, od, oh, ow, 8), float("nan"), dtype=torch.float16, device=dev())
    o1 = h1.forward_hg_dedup(x_poison, desc, 1, sc1, bi1, flags=ops.EPI_RELU, out_exp=0, overflow=g1, out=out)
    assert h1.algo == ops._lib.ALGO_X3_Q16 and h1.hg_dedup_form(N, (d, H, w), desc) == (dups > 0)
    assert torch.isfinite(o0.float()).all() and o0.float().abs().max() > 0
    my = mask[None, None, None, :, None, :, None]
    assert torch.equal(torch.where(my, o0, o1), o0)                                   # written rows: the plain launch's bits
    if dups:                                                                          # duplicate rows: nobody wrote them
        assert bool((o1.view(torch.int16)[my.expand_as(o1)] == 0x7E00).all())
        # and they would have held their representative's bits: the remap is right about the plain launch's result
        remap = torch.tensor([[ops.hg_alias_depth(desc, a, b) for b in range(ow)] for a in range(od)], device=dev())
        assert torch.equal(o0.gather(3, remap[None, None, None, :, None, :, None].expand_as(o0)), o0)
    assert int(g1.item()) == int(g0.item()) == (1 if mul > 1.0 else 0)                # the overflow word

    # hg conv2: aliased on that pair against plain on the fully populated one
    k0, k1 = (torch.zeros(1, dtype=torch.int32, device=dev()) for _ in range(2))
    p0 = h2(o0, 0, sc2, bi2, flags=ops.EPI_RELU, out_exp=0, overflow=k0)
    p1 = h2.forward_hg_reader(o1, desc, 0, sc2, bi2, flags=ops.EPI_RELU, out_exp=0, overflow=k1)
    assert h2.algo == ops._lib.ALGO_X3_Q16 and h2.hg_reader_form(N, (od, oh, ow))
    assert torch.isfinite(p0.float()).all() and p0.float().abs().max() > 0
    assert torch.equal(p1, p0) and int(k1.item()) == int(k0.item())
    return dict(o=o0, p=p0, dups=dups)


@pytest.mark.parametrize("name", list(CASES))
def test_live_walk_and_aliased_reader_return_the_plain_launches_bits_and_nobody_writes_a_duplicate(name):
    hg_case(name)


def test_clamped_result_raises_the_flag_on_both_sides():
    """An affine 2^14 times too large: the stride-2 layer clamps inside the skipped tiles too -- their representative raises the same
    flag."""
    hg_case("q1_one_column", mul=16384.0)


def test_a_form_without_the_entry_points_is_refused_with_its_message_and_launches_nothing():
    from snvc_amd import ops
    d, w = 96, 72
    desc = ops.wedge_desc(d, w, 1, 0, 4)
    x = torch.zeros(N, 2, C // 8, d, H, w, 8, dtype=torch.float16, device=dev())
    h1 = ops.Conv3dLayerX3(torch.randn(2 * C, C, 3, 3, 3, device=dev()) * 0.05, 3, 2, 1, 1, False)
    s1 = ops.Conv3dLayerX3(torch.randn(C, C, 3, 3, 3, device=dev()) * 0.05)
    old = ops.X3_Q16_S2[0]
    ops.X3_Q16_S2[0] = False
    try:
        out = torch.full((N, 2, 2 * C // 8, d // 2, H // 2, w // 2, 8), float("nan"), dtype=torch.float16, device=dev())
        assert not h1.hg_dedup_form(N, (d, H, w), desc)
        with pytest.raises(ops.Unsupported, match="snvc_hgdedup_f16x3_conv3d_forward: built for the stride-2 3x3x3 layer on the 16x16x32 form"):
            h1.forward_hg_dedup(x, desc, out=out)
        assert bool((out.view(torch.int16) == 0x7E00).all())
        with pytest.raises(ops.Unsupported, match="snvc_hgdedup_reader_f16x3_conv3d_forward: built for the stride-1 3x3x3 layer"):
            h1.forward_hg_reader(x, desc, out=out)                   # a stride-2 layer is no reader
        assert bool((out.view(torch.int16) == 0x7E00).all())
    finally:
        ops.X3_Q16_S2[0] = old
    out = torch.full((N, 2, C // 8, d, H, w, 8), float("nan"), dtype=torch.float16, device=dev())
    with pytest.raises(ops.Unsupported, match="snvc_hgdedup_f16x3_conv3d_forward: built for the stride-2 3x3x3 layer"):
        s1.forward_hg_dedup(x, desc, out=out)                        # a stride-1 layer has no live walk
    assert bool((out.view(torch.int16) == 0x7E00).all())
    old = ops.X3_Q16[0]
    ops.X3_Q16[0] = False                                            # the stride-1 layer off its 16x16x32 form
    try:
        assert not s1.hg_reader_form(N, (d, H, w))
        with pytest.raises(ops.Unsupported, match="snvc_hgdedup_reader_f16x3_conv3d_forward: built for the stride-1 3x3x3 layer"):
            s1.forward_hg_reader(x, ops.wedge_desc(2 * d, 2 * w, 1, 0, 4), out=out)
        assert bool((out.view(torch.int16) == 0x7E00).all())
    finally:
        ops.X3_Q16[0] = old
    with pytest.raises(RuntimeError, match=r"in_alias describes a \[Din\]"):          # a descriptor of another tensor
        h1.forward_hg_dedup(x, ops.wedge_desc(d + 4, w, 1, 0, 4))
    with pytest.raises(RuntimeError, match=r"in_desc describes the \[2 Din\]"):
        s1.forward_hg_reader(x, desc)


@pytest.fixture(scope="module")
def stack():
    import bench
    from snvc_amd.models.stereo_volume import GlobalStack
    m = GlobalStack(C)
    m.load_state_dict(bench.seeded_state(m, 11))
    return m.eval().to(dev())


@pytest.mark.parametrize("d,w,q,counts", [(96, 72, 1, True), (148, 72, 2, True), (160, 132, 1, True), (96, 40, 1, False)])
def test_forward_pair_with_and_without_dedup_hourglass(stack, d, w, q, counts):
    """H 8: dedup_hourglass True against False (the alias route's own calls) against dedup_wedge False (every tile computed); the
    counter moves only where the shape has hourglass duplicates and the alias route is taken, and not when the stride-2 layer
    leaves its form.  The operators' shape without duplicates, D 10, is no shape of the hourglass (its two stride-2 levels want D % 4
    == 0); D 96, W 40 stands in for it here: conv2's wedge has duplicates there (the alias route is taken), the hourglass has none."""
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    hm, m0 = 8, 0
    assert stack.alias_wedge and stack.dedup_wedge and stack.fused_first
    assert ops.fused_first_wedge_tiles(d, w, q, m0, 4)[0] > 0
    assert (ops.hg_dedup_tiles(ops.wedge_desc(d, w, q, m0, 4))[0] > 0) == counts
    g = np.random.default_rng(5)
    left = torch.from_numpy(g.standard_normal((N, C, hm, w)).astype(np.float32)).to(dev())
    right = torch.from_numpy(g.standard_normal((N, C, hm, w)).astype(np.float32)).to(dev())
    shift = torch.from_numpy(((m0 + np.arange(d, dtype=np.float32)) / q)[None].repeat(N, 0)).to(dev())
    got = {}
    with torch.no_grad():
        for key, attrs, s2, moves in (("hg", {"dedup_hourglass": True}, True, counts), ("alias", {"dedup_hourglass": False}, True, False),
                                      ("no_alias", {"dedup_hourglass": True, "alias_wedge": False}, True, False),
                                      ("plain", {"dedup_hourglass": True, "dedup_wedge": False}, True, False),
                                      ("no_s2_form", {"dedup_hourglass": True}, False, False)):
            for k, v in attrs.items():
                setattr(stack, k, v)
            old = ops.X3_Q16_S2[0]
            ops.X3_Q16_S2[0] = s2
            try:
                before = S._ROUTES["hg_dedup"], S._ROUTES["wedge_alias"]
                got[key] = stack.forward_pair(left, right, shift, 1).clone()
                assert S._ROUTES["hg_dedup"] - before[0] == (1 if moves else 0), key
                if moves:
                    assert S._ROUTES["wedge_alias"] - before[1] == 1
            finally:
                ops.X3_Q16_S2[0] = old
                for k in attrs:
                    stack.__dict__.pop(k, None)                         # the class defaults stay
    assert torch.isfinite(got["hg"]).all()
    for key in ("alias", "no_alias", "plain"):
        assert torch.equal(got["hg"], got[key]), key
    assert torch.isfinite(got["no_s2_form"]).all()      # another summation order (csrc/conv3d_f16.hip): finite, and the counter stayed
