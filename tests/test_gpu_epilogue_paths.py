"""The epilogues and tile hand-overs of the three split-mode kernels that carry the headline step, on shapes that reach every path
of theirs: conv3d_x3q_kernel (stride-1 3x3x3, 16x16x32 form; with and without the side head), conv3d_f16_kernel's tail-projection
epilogue (the transposed layer in front of the folded one-channel layer) and the persistent stride-2 kernel conv3d_x3s2q_kernel
(one workgroup walking several tiles; a single job).

Every case is a function returning its tensors, so that a script can save them from two builds of the library and compare bits.
References: float64 convolutions on the CPU at test_gpu_tail.py's tolerance (TIGHT, 2e-5).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_parity import TIGHT, check  # noqa: E402

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _aff(c, affine):
    if not affine:
        return None, None
    return torch.rand(c, device=dev()) + 0.5, torch.randn(c, device=dev()) * 0.3


def _aff64(y, scale, bias):
    if scale is None:
        return y
    return y * scale.double().cpu().view(1, -1, 1, 1, 1) + bias.double().cpu().view(1, -1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ conv3d_x3q_kernel
X3Q_CASES = [("32_32_head", True), ("32_32_head", False), ("64_64", True), ("64_64", False)]


def x3q_case(case, affine):
    """Grid 6 x 6 x 40 on 4 x 4 x 32 tiles: a partial tile in depth, height and width, and a second tile along W whose right
    16-column half lies wholly outside the tensor.  The form is forced through the job threshold and the threshold restored."""
    from snvc_amd import _lib as L_
    from snvc_amd import ops
    torch.manual_seed(7 + len(case) + int(affine))
    c, with_head = {"32_32_head": (32, True), "64_64": (64, False)}[case]
    n, sp = 2, (6, 6, 40)
    x = torch.randn(n, c, *sp, device=dev()) * 1.5
    w = torch.randn(c, c, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (c * 27))
    scale, bias = _aff(c, affine)
    head = torch.randn(c, device=dev()) * 0.2 if with_head else None
    x_exp, e_y = 3, 2
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    layer = ops.Conv3dLayerX3(w)
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    try:
        got = layer(ops.to_split(x, x_exp), x_exp, scale, bias, flags=ops.EPI_RELU, out_exp=e_y, head=head, overflow=flag)
        assert layer.algo == L_.ALGO_X3_Q16, layer.algo
    finally:
        ops.X3_Q16_MIN_JOBS[0] = old
    y, y_head = got if with_head else (got, None)
    ref = torch.relu(_aff64(F.conv3d(x.double().cpu(), w.double().cpu(), None, 1, 1), scale, bias))
    out = {"y": y, "y_f32": ops.from_split(y, e_y, c), "flag": flag, "ref": ref}
    if with_head:
        out["y_head"] = y_head
        out["ref_head"] = (ref * head.double().cpu().view(1, -1, 1, 1, 1)).sum(1, keepdim=True)
    return out


@pytest.mark.parametrize("case,affine", X3Q_CASES)
def test_x3q_partial_tiles_affine_and_side_head_vs_float64(case, affine):
    r = x3q_case(case, affine)
    assert int(r["flag"].item()) == 0
    assert torch.isfinite(r["y"].float()).all()
    check(r["y_f32"].cpu().numpy(), r["ref"].numpy(), TIGHT, f"x3q {case} affine={affine}")
    if "y_head" in r:
        check(r["y_head"].cpu().numpy(), r["ref_head"].numpy(), TIGHT, f"x3q {case} affine={affine}: side head")


# ------------------------------------------------------------------------------------------- conv3d_f16_kernel, tail projection (EPI 4)
TAIL_FORMS = ["full", "small"]


def tail_case(form):
    """A coarse input (1, 64, 3, 5, 40) -> the layer's 6 x 10 x 80 result: all eight parity classes, odd extents in depth and
    height (a tile row past the class's extent), a second W tile with 8 of its 32 columns inside; residual before the ReLU."""
    from snvc_amd import _lib as L_
    from snvc_amd import ops
    torch.manual_seed(11 + len(form))
    n, c, shape = 1, 64, (3, 5, 40)
    x = torch.relu(torch.randn(n, c, *shape, device=dev())) * 1.5
    w = torch.randn(c, c, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (c * 27 / 8))
    scale, bias = _aff(c, True)
    pre = torch.relu(torch.randn(n, c, *(2 * s for s in shape), device=dev()))
    wt = torch.randn(c, 1, 3, 3, 3, device=dev()) * 0.2
    layer = ops.Conv3dLayerX3(w, 3, 2, 1, 1, True, algo=L_.ALGO_X3_SMALL if form == "small" else 0)
    tail = ops.TailWeightsX3(wt)
    x_exp, e_y, e_res = 3, 2, 4
    xs, rs = ops.to_split(x, x_exp), ops.to_split(pre, e_res)
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    kw = dict(residual=rs, res_exp=e_res, flags=ops.EPI_RELU | ops.EPI_ADD_PRE, out_exp=e_y)
    t = layer.forward_tail(xs, x_exp, scale, bias, tail, overflow=flag, **kw)
    t_nores = layer.forward_tail(xs, x_exp, scale, bias, tail, flags=ops.EPI_RELU, out_exp=e_y, overflow=flag)
    post = layer(xs, x_exp, scale, bias, to_f32=True, **kw)           # the unfused route: the layer's own result, stored as fp32
    conv64 = _aff64(F.conv_transpose3d(x.double().cpu(), w.double().cpu(), None, 2, 1, 1), scale, bias)
    return {"t": t, "t_nores": t_nores, "post": post, "flag": flag, "wt": wt, "shape": shape,
            "post64": torch.relu(conv64 + pre.double().cpu()), "post64_nores": torch.relu(conv64)}


def _contract64(post, wt, shape):
    """T [N, 27, 8 classes, d, h, w] of a stored result, in float64."""
    n, c = post.shape[:2]
    d_, h_, w_ = shape
    t = torch.einsum("ck,ncdhw->nkdhw", wt.double().cpu().reshape(c, 27), post.double().cpu())
    return t.reshape(n, 27, d_, 2, h_, 2, w_, 2).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(n, 27, 8, d_, h_, w_)


@pytest.mark.parametrize("form", TAIL_FORMS)
def test_tail_projection_every_parity_class_vs_unfused_and_float64(form):
    from snvc_amd import ops
    r = tail_case(form)
    assert int(r["flag"].item()) == 0
    t, shape = r["t"], r["shape"]
    assert t.shape == (1, 27, 8) + shape and torch.isfinite(t).all()
    tref = _contract64(r["post64"], r["wt"], shape)
    for cls in range(8):          # each class on its own: a class that is wrong or missing cannot hide behind the others' magnitude
        check(t[:, :, cls].cpu().numpy(), tref[:, :, cls].numpy(), TIGHT, f"tail {form}: class {cls} vs float64")
    check(t.cpu().numpy(), _contract64(r["post"], r["wt"], shape).numpy(), TIGHT, f"tail {form}: vs the stored layer, contracted")
    check(r["t_nores"].cpu().numpy(), _contract64(r["post64_nores"], r["wt"], shape).numpy(), TIGHT, f"tail {form}: no residual")
    got = ops.deconv_tail_gather(t)
    ref = F.conv_transpose3d(r["post64"], r["wt"].double().cpu(), None, 2, 1, 1)
    check(got.cpu().numpy(), ref.numpy(), TIGHT, f"tail {form}: gathered vs float64")


def stack_tail_case():
    """The global stack on a 12 x 20 x 160 volume: the hourglass's conv5 sees the coarse (1, 64, 3, 5, 40) input; fused tail against
    the two-launch tail (``fused_tail = False``)."""
    import bench
    from snvc_amd.models import submodule as S
    from snvc_amd.models.stereo_volume import GlobalStack
    m = GlobalStack(32)
    m.load_state_dict(bench.seeded_state(m, 5))
    m.eval().to(dev())
    g = np.random.default_rng(3)
    left = torch.from_numpy(g.standard_normal((1, 32, 20, 160)).astype(np.float32)).to(dev())
    right = torch.from_numpy(g.standard_normal((1, 32, 20, 160)).astype(np.float32)).to(dev())
    shift = torch.from_numpy(np.arange(12, dtype=np.float32)[None] * 0.5).to(dev())
    with torch.no_grad():
        before = S._ROUTES["x3_fused_tail"]
        a = m.forward_pair(left, right, shift, 1)
        assert S._ROUTES["x3_fused_tail"] == before + 1
        m.fused_tail = False
        b = m.forward_pair(left, right, shift, 1)
        assert S._ROUTES["x3_fused_tail"] == before + 1
    return {"fused": a, "unfused": b}


def test_global_stack_fused_tail_on_the_coarse_grid_equals_the_unfused_route():
    r = stack_tail_case()
    assert torch.isfinite(r["fused"]).all()
    check(r["fused"].cpu().numpy(), r["unfused"].cpu().numpy(), TIGHT, "fused tail vs fused_tail=False, coarse grid 3 x 5 x 40")


# ------------------------------------------------------------------------------------------------------------- conv3d_x3s2q_kernel
S2_CASES = {"288_jobs": (2, 32, 64, (48, 48, 94)), "single_job": (1, 32, 64, (2, 3, 5))}


def x3s2q_case(case):
    """288_jobs: 2 x (12 x 6 x 2) tiles of one 64-channel block -- more jobs than the launch has workgroups (one per CU), so a
    workgroup hands over between tiles; odd output width 47 (a partial second W tile).  single_job: one partial tile."""
    from snvc_amd import _lib as L_
    from snvc_amd import ops
    n, cin, cout, sp = S2_CASES[case]
    torch.manual_seed(13 + len(case))
    x = torch.randn(n, cin, *sp, device=dev()) * 1.5
    w = torch.randn(cout, cin, 3, 3, 3, device=dev()) * np.sqrt(2.0 / (cin * 27))
    scale, bias = _aff(cout, True)
    x_exp, e_y = 3, 2
    flag = torch.zeros(1, dtype=torch.int32, device=dev())
    layer = ops.Conv3dLayerX3(w, 3, 2, 1, 1, False)
    old = ops.X3_Q16_S2[0]
    ops.X3_Q16_S2[0] = True
    try:
        y = layer(ops.to_split(x, x_exp), x_exp, scale, bias, flags=ops.EPI_RELU, out_exp=e_y, overflow=flag)
        y_plain = layer(ops.to_split(x, x_exp), x_exp, None, None, flags=0, out_exp=e_y, overflow=flag)
        assert layer.algo == L_.ALGO_X3_Q16, layer.algo
    finally:
        ops.X3_Q16_S2[0] = old
    conv64 = F.conv3d(x.double().cpu(), w.double().cpu(), None, 2, 1)
    return {"y": y, "y_f32": ops.from_split(y, e_y, cout), "y_plain": y_plain, "y_plain_f32": ops.from_split(y_plain, e_y, cout),
            "flag": flag, "ref": torch.relu(_aff64(conv64, scale, bias)), "ref_plain": conv64}


@pytest.mark.parametrize("case", list(S2_CASES))
def test_x3s2q_tile_hand_over_and_single_job_vs_float64(case):
    r = x3s2q_case(case)
    assert int(r["flag"].item()) == 0
    assert torch.isfinite(r["y"].float()).all()
    check(r["y_f32"].cpu().numpy(), r["ref"].numpy(), TIGHT, f"x3s2q {case}: affine + ReLU")
    check(r["y_plain_f32"].cpu().numpy(), r["ref_plain"].numpy(), TIGHT, f"x3s2q {case}: no affine")
    if case == "288_jobs":        # the two samples' tiles are walked by the same workgroups: each sample on its own as well
        for i in range(2):
            check(r["y_f32"][i:i + 1].cpu().numpy(), r["ref"][i:i + 1].numpy(), TIGHT, f"x3s2q {case}: sample {i}")
