"""Guard bands (tests/guarded.py) around the split-mode kernels of conv3d_f16.hip, the layout passes of layout_f16.hip, the fused
first layer and the sheared and warped first layers of sheared_conv.hip: the partial tiles, tile hand-overs, fused image fills and early-loading
epilogues that get rewritten most.  Cases and assertions as in tests/test_gpu_guard_conv.py: each is an existing test run unchanged,
once as it is and once with every operand placed between NaN guards and every allocation of the wrappers between guard zones.

Second placement: 4 bytes off 256 where the wrapper or the launcher branches on alignment (the layout passes, the depth-1 layers, the
sheared backward, the scale reduction); 16 bytes off 256 where the C side refuses operands that are not 16-byte aligned (the split
convolutions' per-channel vectors, the sheared expand's planes: "must be 16-byte aligned" is the contract there, and 256 + 16 is the
least such an operand may have), 32 for the fused first layer ("gi / p_il / v_scale / v_bias must be 32-byte aligned"); None -- the
aligned placement alone -- where the wrapper falls back to another pass off 16 bytes and the existing test asserts that the aligned
pass ran (the twin passes: ``twin_falls_back_case`` and ``act_backward_apply_twin_case`` check the fall-back at 4 bytes off
instead).  Split pairs themselves are allocated by the wrappers, hence always 256-byte aligned.
"""
import pytest
import torch

import guarded as GD
import test_gpu_epilogue_paths as EP_M
import test_gpu_x3_train as X3T_M

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, EP, F16, TAIL, X3T, FFL, SPLIT = ("test_gpu_parity", "test_gpu_epilogue_paths", "test_gpu_f16", "test_gpu_tail", "test_gpu_x3_train",
                                     "test_gpu_fused_first_layer", "test_gpu_split_format")
ROUND_TRIP_SHAPES = [(1, 8, (2, 3, 258)), (1, 32, (3, 5, 68)), (2, 64, (6, 8, 20))]


def layout_round_trip_case(shape):
    """to_split / from_split and to_c8 / from_c8.  x * 2^e = hi + lo with hi = half(x * 2^e) and lo = half of the rest: 22 bits of x
    unless lo is subnormal (steps of 2^-24), so |x' - x| <= 2^-21 |x| + 2^-24 * 2^-e; the C8 layout holds half(x) exactly."""
    from snvc_amd import ops
    n, c, sp = shape
    torch.manual_seed(c)
    x = torch.randn(n, c, *sp, device=DEV) * 3
    for e in (0, 3):
        pair = ops.to_split(x, e)
        assert pair.shape == (n, 2, c // 8) + sp + (8,) and torch.isfinite(pair.float()).all()
        back = ops.from_split(pair, e, c)
        assert ((back - x).abs() <= 2.0 ** -21 * x.abs() + 2.0 ** (-24 - e)).all()
    assert torch.equal(ops.from_c8(ops.to_c8(x), c), x.half().float())


def twin_falls_back_case(shape):
    """affine_act with ``twin_mul`` on operands that are not 16-byte aligned: the plain pass's bits and no twin."""
    from snvc_amd import ops
    n, c, sp = shape
    torch.manual_seed(c + 1)
    raw, res = torch.randn(n, c, *sp, device=DEV) * 3, torch.randn(n, c, *sp, device=DEV)
    scale, shift = torch.rand(1, c, device=DEV) + 0.5, torch.randn(1, c, device=DEV)
    flags = ops.EPI_RELU | ops.EPI_ADD_PRE
    ref = ops.affine_act(raw, scale, shift, res, flags, False)
    got = ops.affine_act(raw, scale, shift, res, flags, False, amax=ops.amax_word(torch.device(DEV)), twin_mul=ops.split_scale_of(ref))
    assert torch.equal(got, ref) and torch.isfinite(got).all()
    assert (ops.twin_of(got) is None) == bool(raw.data_ptr() % 16 or res.data_ptr() % 16)


def act_backward_apply_twin_case(shape):
    """act_backward_reduce and act_backward_apply with ``twin_mul`` at the layout shapes (tail waves, partial channel groups), as
    test_gpu_x3_train._act_backward_apply_twin does at its one shape: the twin pass's draw and g are the plain pass's bit for bit, the
    pair is to_split(draw) bit for bit, the words hold max|gy| and max|draw|; operands off 16 bytes: the plain pass's bits, no twin."""
    from snvc_amd import ops
    n, c, sp = shape
    torch.manual_seed(c + 2)
    dev = torch.device(DEV)
    raw, gy, res = (torch.randn(n, c, *sp, device=DEV) * m for m in (3.0, 1e-4, 1.0))
    scale, shift = torch.rand(1, c, device=DEV) + 0.5, torch.randn(1, c, device=DEV)
    A, B, Cc = torch.randn(c, device=DEV), torch.randn(c, device=DEV) * 1e-5, torch.randn(c, device=DEV) * 1e-6
    flags = ops.EPI_RELU | ops.EPI_ADD_PRE
    d0, g0 = ops.act_backward_apply(raw, gy, res, scale, shift, A, B, Cc, flags, False, True)
    amg = ops.amax_word(dev)
    s1 = ops.act_backward_reduce(raw, gy, res, scale, shift, flags, False, amax_gy=amg)
    assert torch.equal(s1, ops.act_backward_reduce(raw, gy, res, scale, shift, flags, False)) and torch.isfinite(s1).all()
    assert amg.max().view(torch.float32).item() == gy.abs().max().item()
    ax = ops.amax_from_bound(raw.abs().max())
    mul = ops.split_scale_bound(c, c, dev, a=A, amax_p=amg, b=B, l1=torch.ones(c, device=DEV), amax_x=ax, cc=Cc)
    am = ops.amax_word(dev)
    d1, g1 = ops.act_backward_apply(raw, gy, res, scale, shift, A, B, Cc, flags, False, True, amax=am, twin_mul=mul)
    assert torch.equal(d0, d1) and torch.equal(g0, g1) and torch.isfinite(d1).all()
    assert am.max().view(torch.float32).item() == d1.abs().max().item()
    twin = ops.twin_of(d1)
    assert (twin is None) == bool(raw.data_ptr() % 16 or gy.data_ptr() % 16 or res.data_ptr() % 16)
    if twin is not None:
        assert torch.equal(twin[0], ops.to_split(d0, mul_dev=mul))


def fused_first_case(q, m0, narrow):
    """test_conv2_pair_and_side_head_through_ops under its module's autouse fixture: the 16x16x32 form at every size."""
    from snvc_amd import ops
    from test_gpu_fused_first_layer import test_conv2_pair_and_side_head_through_ops as case
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    try:
        case(q, m0, True, narrow)
    finally:
        ops.X3_Q16_MIN_JOBS[0] = old


# (id, module, function, keyword arguments, second placement in bytes or None, options of run_case)
CASES = [(f"f32_out_{c.split(' (')[0].replace(' ', '_').replace('->', '_')}", X3T, "test_split_layer_f32_output_residual_and_statistics", dict(case=c), 16, {})
         for c in X3T_M._LAYERS]
CASES += [(f"x3q_{c}_{'affine' if a else 'plain'}", EP, "test_x3q_partial_tiles_affine_and_side_head_vs_float64", dict(case=c, affine=a), 16, {})
          for c, a in EP_M.X3Q_CASES]
CASES += [(f"x3s2q_{c}", EP, "test_x3s2q_tile_hand_over_and_single_job_vs_float64", dict(case=c), 16,
           dict(arena_bytes=2 << 30) if c == "288_jobs" else {}) for c in EP_M.S2_CASES]
CASES += [(f"tail_{f}", EP, "test_tail_projection_every_parity_class_vs_unfused_and_float64", dict(form=f), 16, {}) for f in EP_M.TAIL_FORMS]
CASES += [(f"split_{c}", F16, "test_split_mode_layers_vs_float64", dict(case=c), 16, {}) for c in ("k3_32_32_odd", "k3s2_32_64", "deconv_64_64")]
CASES += [(f"q16_{c}", F16, "test_split_mode_16x16x32_forms_vs_float64", dict(case=c), 16, {}) for c in ("k7_16_64", "k5d2_8_96", "k3_64_32_ragged")]
CASES += [(f"depth1_{c}", TAIL, "test_depth1_split_layer_vs_float64", dict(case=c), 4, {}) for c in ("3x7_8_32_ragged", "3x3_64_64_tiny")]
for i, s in enumerate(ROUND_TRIP_SHAPES):
    CASES += [(f"round_trip_{i}", __name__, "layout_round_trip_case", dict(shape=s), 4, {}),
              (f"affine_act_twin_{i}", X3T, "test_affine_act_twin", dict(flags_res=("relu+pre", True), shape=s), None, {}),
              (f"twin_falls_back_{i}", __name__, "twin_falls_back_case", dict(shape=s), 4, {}),
              (f"act_backward_apply_twin_{i}", __name__, "act_backward_apply_twin_case", dict(shape=s), 4, {})]
CASES += [(f"act_backward_apply_twin_{'g' if g else 'nog'}", X3T, "test_act_backward_apply_twin", dict(flags_res=("relu+pre", True), want_g=g), None, {})
          for g in (False, True)]
CASES += [(f"split_scale_of_{n}", TAIL, "test_split_scale_in_one_launch_equals_the_torch_expression", dict(n=n), 4, {}) for n in (1, 3, 1023)]
# the fused first layer: gi, p_il, the scale / bias vectors and the pair; narrow = 8: G's index leaves its rows on both sides
CASES += [(f"fused_first_q{q}_m{m0}_narrow{nw}", __name__, "fused_first_case", dict(q=q, m0=m0, narrow=nw), 32, {})
          for q, m0, nw in ((1, 0, 0), (2, 1, 0), (1, 0, 8))]
# the sheared first layer: statistics, backward and weight-gradient workspaces
for q, m0 in ((2, 0), (2, 5), (1, 1)):
    CASES += [(f"sheared_bn_q{q}_m{m0}", P, "test_sheared_fused_batchnorm_entry_points_vs_numpy", dict(q=q, m0=m0), 16, {}),
              (f"sheared_bwd_q{q}_m{m0}", P, "test_sheared_backward_entry_points_vs_numpy", dict(q=q, m0=m0), 4, {})]
CASES += [(f"sheared_upsample_split_q{q}", TAIL, "test_sheared_upsample_split_equals_upsample_then_split", dict(q=q), 4, {}) for q in (1, 2)]
# the producers that tests/test_gpu_split_format.py calls directly, at its shapes (ragged channel group, two depth chunks, partial wave)
CASES += [("mul_broadcast_split_c20", SPLIT, "mul_broadcast_split_case", dict(c=20, sp=(2, 3, 67)), 4, {}),
          ("mul_broadcast_split_c8_one_voxel", SPLIT, "mul_broadcast_split_case", dict(c=8, sp=(1, 1, 1)), 4, {})]
CASES += [(f"sheared_expand_split_q{q}_{'planes' if pl else 'no_planes'}", SPLIT, "sheared_expand_split_case", dict(q=q, with_planes=pl), 16, {})
          for q, pl in ((1, True), (2, False))]
CASES += [(f"warped_expand_split_{'planes' if pl else 'no_planes'}", SPLIT, "warped_expand_split_case", dict(with_planes=pl), 16, {})
          for pl in (True, False)]
# one row per row / chunk form of the first-layer kernels (tests/test_gpu_first_layer_forms.py, each case run unchanged -- it asserts its form
# through the query first): RB 8 with a short last block, RB 3 and RB 2 with idle threads in the last wave; both statistics workspaces
# (the forward partials with fewer row blocks than rows, the fused backward's at 64 lanes and at one); 16 depth chunks with a short one
# and one without planes, and the end plane alone in its chunk; the weight gradient's two column chunks; the adjoint's second trip
FORMS = "test_gpu_first_layer_forms"
CASES += [(f"forms_sheared_expand_{n}_{m}", FORMS, "sheared_expand_case", dict(name=n, mode=m), 16, dict(arena_bytes=512 << 20) if "w320" in n else {})
          for n, m in (("rb8_short_block", "plain"), ("rb8_short_block", "amax"), ("rb3_w320", "affine"), ("rb2_w44", "plain"))]
CASES += [(f"forms_sheared_stats_{n}", FORMS, "sheared_stats_case", dict(name=n), 16, dict(arena_bytes=512 << 20) if "w320" in n else {})
          for n in ("rb8_short_block", "rb3_w320")]
CASES += [(f"forms_sheared_backward_{n}", FORMS, "sheared_backward_case", dict(name=n), 16, {}) for n in ("w512_q2", "w8_q1")]
CASES += [(f"forms_sheared_split_{n}_q{q}", FORMS, "sheared_expand_split_case", dict(name=n, q=q), 16, {})
          for n, q in (("d131", 4), ("d131", 1), ("d241_end_plane_alone", 2))]
CASES += [(f"forms_warped_split_{n}", FORMS, "warped_expand_split_case", dict(name=n), 16, {}) for n in ("d131", "d241_end_plane_alone")]
CASES += [(f"forms_sheared_wgrad_{n}_c{c}", FORMS, "sheared_wgrad_case", dict(name=n, cin=c), 4, {}) for n, c in (("wu321", 5), ("wu388", 32))]
CASES += [(f"forms_sheared_reduce_{n}", FORMS, "sheared_reduce_case", dict(name=n), 4, {}) for n in ("slots_308", "wg2_260")]

RUNS = [(c, off) for c in CASES for off in (0, c[4]) if off is not None]          # the two placements back to back: one unguarded run


@pytest.mark.parametrize("case,off", RUNS, ids=[f"{c[0]}-{'aligned' if not off else 'off%d' % off}" for c, off in RUNS])
def test_guarded(case, off):
    _, module, name, kwargs, _, options = case
    GD.run_existing(module, name, kwargs, DEV, off, **options)
