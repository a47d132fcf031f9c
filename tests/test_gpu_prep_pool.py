"""The pooled first-layer prep (ops.prep_pooled_x3, include/snvc_prep.h; GlobalStack.pooled_prep): three launches for the eight of
``ops.planes_x3_il`` + ``ops.sheared_prep_x3_il``.  Every pooled block runs the body of the kernel it replaces on the same operands,
so every comparison here is torch.equal -- results, the interleaved buffer with its zero pads, both scales, the three split pairs.

Shapes (C = 32, D = 12; (q, m0) = (2, 0) and (1, 2)):
  N 2, H 8, W 40    the fused first layer's own test shape: one short tile row (8 of 16 rows)
  N 2, H 20, W 72   two tile rows, the second short (4 rows); three tile columns in the 3x3 layer, the last short (8 of 32 columns)
  N 1, H 7, W 44    the stage-B ranges end in partial blocks (asserted below), so a block's tail threads must stay inside their range
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C, D = 32, 12
SHAPES = [(2, 8, 40), (2, 20, 72), (1, 7, 44)]
SPACINGS = [(2, 0), (1, 2)]
NAMES = ("planes", "p_il", "g", "gcol", "gi", "mul_right", "mul_left", "rq", "rq2", "split")


def dev():
    return torch.device("cuda:0")


_LAYERS = {}


def layers():
    """(G, G', left planes) layers, packed once for the module."""
    from snvc_amd import ops
    if not _LAYERS:
        torch.manual_seed(21)
        wp = torch.randn(3 * C, C, 3, 3, device=dev()) * 0.06
        _LAYERS["l"] = (ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04),
                        ops.Conv2dLayerX3(torch.randn(3 * C, C, 3, 7, device=dev()) * 0.04),
                        ops.Conv2dLayerX3(wp))
        # the same 3x3 kernels with their rows in class-major order (part 2: prep_pooled_x3(left_rows=1))
        _LAYERS["cm"] = ops.Conv2dLayerX3(wp[torch.tensor(ops.class_major_rows(C), device=dev())].contiguous())
    return _LAYERS["l"]


def features(n, h, w, lmul=1.0, rmul=1.0, seed=7):
    g = np.random.default_rng(seed)
    left = torch.from_numpy(g.standard_normal((n, C, h, w)).astype(np.float32) * np.float32(lmul)).to(dev())
    right = torch.from_numpy(g.standard_normal((n, C, h, w)).astype(np.float32) * np.float32(rmul)).to(dev())
    return left, right


def geometry(q, m0, w):
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    off, wu, off_col, wu_col = sheared_geometry(q, m0, D, w)
    pitch, lp = ops.fused_il_geometry(q, m0, D, w, wu, off, wu_col, off_col)
    return off, wu, off_col, wu_col, pitch, lp


def single(left, right, q, m0):
    """The two calls the pooled one replaces: every tensor they leave, by name."""
    from snvc_amd import ops
    lay_g, lay_c, lay_p = layers()
    off, wu, off_col, wu_col, pitch, lp = geometry(q, m0, left.size(3))
    ws_p, ws_s = {}, {}
    planes, p_il = ops.planes_x3_il(left, lay_p, ws_p)
    g, gcol, gi = ops.sheared_prep_x3_il(right, q, wu, off, wu_col, off_col, lay_g, lay_c, ws_s, pitch, lp)
    return dict(planes=planes, p_il=p_il, g=g, gcol=gcol, gi=gi, mul_right=ws_s["mul"], mul_left=ws_p["mul"], rq=ws_s["rq"], rq2=ws_s["rq2"],
                split=ws_p["split"])


def pooled(left, right, q, m0, ws=None, cm=0):
    from snvc_amd import ops
    lay_g, lay_c, lay_p = layers()
    if cm:
        lay_p = _LAYERS["cm"]
    off, wu, off_col, wu_col, pitch, lp = geometry(q, m0, left.size(3))
    ws = {} if ws is None else ws
    planes, p_il, g, gcol, gi = ops.prep_pooled_x3(left, right, q, wu, off, wu_col, off_col, lay_g, lay_c, lay_p, ws, pitch, lp, cm)
    return dict(planes=planes, p_il=p_il, g=g, gcol=gcol, gi=gi, mul_right=ws["mul"], mul_left=ws["mul_left"], rq=ws["rq"], rq2=ws["rq2"],
                split=ws["split"])


def same(got, want):
    for k in NAMES:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        assert torch.equal(got[k], want[k]), k
    assert torch.isfinite(got["planes"]).all() and torch.isfinite(got["g"]).all() and torch.isfinite(got["gi"]).all()


def pool_case(n, h, w, q, m0, lmul=1.0, rmul=1.0, zero_left=False, stages=None, cm=0):
    """One comparison (also what the guard-band test runs between guard zones)."""
    from snvc_amd import ops
    left, right = features(n, h, w, lmul, rmul)
    if zero_left:
        left = torch.zeros_like(left)
    want = single(left, right, q, m0)
    old = ops.PREP_POOL_STAGES[0]
    if stages is not None:
        ops.PREP_POOL_STAGES[0] = stages
    try:
        got = pooled(left, right, q, m0, cm=cm)
    finally:
        ops.PREP_POOL_STAGES[0] = old
    same(got, want)
    return got


@pytest.mark.parametrize("cm", [0, 1], ids=["class_minor", "class_major"])
@pytest.mark.parametrize("q,m0", SPACINGS)
@pytest.mark.parametrize("n,h,w", SHAPES)
def test_pooled_equals_the_two_calls(n, h, w, q, m0, cm):
    """cm 1: the left planes' layer packed with class-major rows -- planes and p_il must still hold the single calls' bytes."""
    pool_case(n, h, w, q, m0, cm=cm)


def test_partial_blocks_shape_has_partial_ranges():
    from snvc_amd import ops
    n, h, w = SHAPES[2]
    _, wu, _, wu_col, _, _ = geometry(2, 0, w)
    plan = ops.prep_pool_plan(n, C, h, w, wu, wu_col)
    assert any(t % 256 for t in plan.b_items)              # at least one stage-B range ends inside a block
    assert (h * w) % 256                                    # ... and so does every row of the left pair's range


@pytest.mark.parametrize("stages", [0, 1, 2])
def test_each_stage_alone(stages):
    """Stages A + B and stage C are separable in the host call: any mix of pooled and single launches leaves the same bits."""
    n, h, w = SHAPES[1]
    pool_case(n, h, w, 2, 0, stages=stages, cm=stages & 1)


def test_scales_do_not_mix():
    """left * 1e-3, right * 1e3: the two scales differ by 2^20 -- a swap of scratch words or of the scale pointers shows in every tensor."""
    n, h, w = SHAPES[0]
    got = pool_case(n, h, w, 2, 0, lmul=1e-3, rmul=1e3, cm=1)
    assert float(got["mul_left"]) > 1e5 * float(got["mul_right"])


def test_all_zero_left_takes_scale_one():
    n, h, w = SHAPES[0]
    got = pool_case(n, h, w, 1, 2, zero_left=True)
    assert float(got["mul_left"]) == 1.0 and not got["planes"].any() and not got["p_il"].any()


def test_two_calls_in_a_row_and_the_scratch_is_left_zero():
    from snvc_amd import ops
    n, h, w = SHAPES[0]
    left, right = features(n, h, w, 1e-3, 1e3)
    want = single(left, right, 2, 0)
    want_scale = ops.split_scale_of(right).clone()
    ws = {}
    first = {k: v.clone() for k, v in pooled(left, right, 2, 0, ws).items()}
    second = pooled(left, right, 2, 0, ws)
    same(first, want)
    same(second, want)
    assert second["gi"].data_ptr() == ws["gi"].data_ptr() and len(ws["layers"]) == 1                # the keyed workspace, reused
    assert not ops._pool_scratch(dev()).any()                                      # all four words back to zero
    assert torch.equal(ops.split_scale_of(right), want_scale) and not ops._scale_scratch(dev()).any()
    assert torch.equal(want_scale, want["mul_right"])


@pytest.fixture()
def q16_everywhere():
    from snvc_amd import ops
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    yield
    ops.X3_Q16_MIN_JOBS[0] = old


def test_forward_pair_pooled_against_single(q16_everywhere):
    """At test_gpu_pair_routes.py's shape with the 16x16x32 form forced (its row half_pixel_fused_q16): a fresh model's first call has no
    guess and pools nothing; the second call pools once, counts the routes of that row, and gives the bits of pooled_prep = False."""
    from collections import Counter

    import test_gpu_pair_routes as R
    from snvc_amd.models import stereo_volume as SV
    from snvc_amd.models import submodule as S
    left, right = R._features()
    shift = R._planes(2, 0)
    out = {}
    with torch.no_grad():
        for on in (True, False):
            m = R._model()
            m.pooled_prep = on
            c0 = SV.POOLED_PREP_CALLS
            first = m.forward_pair(left, right, shift, 1).clone()
            assert SV.POOLED_PREP_CALLS == c0                        # no guess yet: the code path is the parent's
            before = Counter(S._ROUTES)
            cost = m.forward_pair(left, right, shift, 1).clone()
            delta = dict(Counter(S._ROUTES) - before)
            assert SV.POOLED_PREP_CALLS - c0 == (1 if on else 0)
            assert delta == R.ROWS["half_pixel_fused_q16"][1]
            assert torch.equal(first, cost)
            out[on] = (cost, m.last_first_layer().clone())
            known = m.forward_pair(left, right, shift, 1, shift_checked=True, spacing=(2, 0))      # the spacing known: pooled as well
            assert SV.POOLED_PREP_CALLS - c0 == (2 if on else 0) and torch.equal(known, cost)
    assert torch.isfinite(out[True][0]).all()
    assert torch.equal(out[True][0], out[False][0]) and torch.equal(out[True][1], out[False][1])


def test_a_wrong_guess_keeps_the_planes(q16_everywhere):
    """The guess (q 2) is wrong for the second call's planes (q 1): the sheared inputs are queued again on their own, the planes of the
    pooled call stay, and the result is that of a model that never guessed."""
    import test_gpu_pair_routes as R
    from snvc_amd.models import stereo_volume as SV
    left, right = R._features()
    with torch.no_grad():
        want = R._model().forward_pair(left, right, R._planes(1, 2), 1).clone()
        m = R._model()
        m.forward_pair(left, right, R._planes(2, 0), 1)
        c0 = SV.POOLED_PREP_CALLS
        got = m.forward_pair(left, right, R._planes(1, 2), 1)
        assert SV.POOLED_PREP_CALLS - c0 == 1
    assert torch.equal(got, want)
