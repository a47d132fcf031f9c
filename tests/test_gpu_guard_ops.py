"""Guard bands (tests/guarded.py) around everything that is not a 3D convolution: cost volume and warped expand (cost_volume.hip),
the gather in both directions (voxel_gather*.hip), the norm / activation passes and the small ops of elementwise.hip, and two to four
of the smallest existing cases of every newer op.  Cases and assertions as in tests/test_gpu_guard_conv.py: each is an existing test
run unchanged, once as it is and once with every operand placed between guards (floating operands: NaN; index and label operands:
the tensor's own minimum, a value inside the valid range) and every allocation of the wrappers between guard zones.

Second placement: 4 bytes off 256; 8 or 16 where the entry point refuses less ("transposed y / residual must be 8-byte aligned",
``snvc_depth_class_sums``, ``snvc_deconv_tail_gather`` and ``snvc_fc_eval_forward`` ask for 16): the least alignment its contract allows.
The rows of tests/geometry_cases.py (``forms_*``: one guarded run per launcher form of the cost volume and the gather, the test
functions of tests/test_gpu_geometry_forms.py run unchanged) carry their own second placement -- 16 bytes for the vector and LDS forms,
4 for the scalar ones -- because each asserts, through the form query, that it still takes the form it is there for.

``loose``: the results of the two float-atomics forms -- the call ``voxel_gather_backward(..., deterministic=False)`` and the RoI-aware
pool's backward -- differ in bits from run to run and are compared with the unguarded run at the tolerance of the op's existing test
(2e-4 of the largest magnitude; 1e-5 absolute); everything else those cases allocate, the deterministic adjoint and the pool's forward
outputs included, is compared bit for bit.
"""
import pytest

import guarded as GD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P, EPI = "test_gpu_parity", "test_gpu_epilogue"
GATHER_ATOMICS = dict(loose=(("deterministic=False", 2e-4, 0.0),))          # test_voxel_gather_backward_deterministic: 2e-4 * scale
ROI_ATOMICS = dict(loose=(("in backward", 0.0, 1e-5),))           # test_roiaware_pool3d_bit_exact: assert_allclose(rtol 1e-5, atol 1e-5)


def affine_act_case(shape, per_sample):
    """test_gpu_epilogue.test_affine_act's body on a shape its own table leaves out (VEC_TAIL: whole float4 pieces and a ragged last one)."""
    import test_gpu_epilogue as E
    cs = E.Case(shape, per_sample, 21)
    for flags in E.FLAG_SETS:
        E._check_affine(cs, flags, cs.scale, cs.shift, None)
    E._check_affine(cs, E.RELU | E.PRE, None, cs.shift, None)
    E._check_affine(cs, E.RELU, cs.scale, None, None)


def targets_case(name):
    """test_gpu_targets.test_small_cases_match_the_reference without its cache: the targets are generated in this very call."""
    import test_gpu_targets as T
    fields, meta = T.generated.__wrapped__(name)
    T.compare_small(name, fields, meta)


def _table():
    import decode_cases as DEC
    import depth_cases as DC
    import fcmodel_cases as FC
    import geometry_cases as GEO
    import neck2d_backward_cases as NB
    import roi_crop_cases as RC
    import test_gpu_epilogue as E
    import test_gpu_hrnet as HR
    import test_gpu_iou3d as IOU
    import test_gpu_parity as TP
    t = []
    # ---------------------------------------------------------------------------------------------- cost volume, warped expand
    for i in (1, 2, 3, 4):                                    # odd W, downsample 2 and 3, double
        N, C, H, W, D, ds, dtype = TP.CV_CASES[i]
        kw = dict(N=N, C=C, H=H, W=W, D=D, ds=ds, dtype=dtype)
        t += [(f"cost_volume_fwd_{i}", P, "test_cost_volume_forward_bit_exact", kw, 4, {}),
              (f"cost_volume_bwd_{i}", P, "test_cost_volume_backward_bit_exact", kw, 4, {})]
    t += [("warped_expand_bwd_beyond_the_image", P, "test_warped_expand_backward_vs_oracle", dict(case="beyond_the_image"), 16, {}),
          ("warped_expand_bwd_odd_width", P, "test_warped_expand_backward_vs_oracle", dict(case="odd_width"), 4, {})]
    t += [("shift_structure", P, "test_shift_structure_flags", {}, 4, {})]
    # the any-shift first layer with more than one row per workgroup (tests/test_gpu_first_layer_forms.py, run unchanged): RB 8 with a
    # short last block, RB 2 with a single row left; p, y and planes must stay 16-byte aligned
    t += [(f"forms_warped_expand_{n}", "test_gpu_first_layer_forms", "warped_expand_case", dict(name=n), 16, {})
          for n in ("rb8_short_block", "rb2_one_row_left")]
    # ------------------------------------------------------------------------------------------------------------------ gather
    t += [("gather_edges", P, "test_voxel_gather_vs_torch_ref_edge_cases", {}, 4, {}),                       # (2, 5, 7 x 9, V 30, (28, 36))
          ("gather_lds", P, "test_voxel_gather_lds_path_bit_exact_with_edge_coordinates", dict(res=(64, 128)), 4, {}),   # fp32 and f16
          ("gather_bwd_edges", P, "test_voxel_gather_backward_deterministic", dict(case="edges"), 4, GATHER_ATOMICS),
          ("gather_bwd_coherent", P, "test_voxel_gather_backward_deterministic", dict(case="coherent"), 4, GATHER_ATOMICS),
          ("gather_zero_points_and_empties", P, "test_empty_and_ragged_inputs", {}, 4, {})]
    t += [(f"forms_{c.name}", "test_gpu_geometry_forms", GEO.TEST_OF_ENTRY[c.entry], dict(c=c), c.place,
           GATHER_ATOMICS if c.entry == "gather_bwd" and not c.det else {}) for c in GEO.GUARDED]
    # -------------------------------------------------------------------------------------------------- elementwise, epilogue
    big = dict(arena_bytes=512 << 20)
    for s in list(E.TINY) + [E.GROUPS, E.VEC_TAIL, E.SCALAR_TAIL]:
        opts = big if s == E.VEC_TAIL else {}
        t += [(f"norm_stats_{E._id(s)}", EPI, "test_norm_stats", dict(case=s, data="ordinary"), 4, {})]
        for ps in (False, True):
            t += [(f"act_backward_{E._id(s)}_ps{int(ps)}", EPI, "test_act_backward", dict(case=s, per_sample=ps), 4, opts)]
            if s == E.VEC_TAIL:                               # test_affine_act's own table has no VEC_TAIL
                t += [(f"affine_act_{E._id(s)}_ps{int(ps)}", __name__, "affine_act_case", dict(shape=s, per_sample=ps), 4, opts)]
            else:
                t += [(f"affine_act_{E._id(s)}_ps{int(ps)}", EPI, "test_affine_act", dict(case=s, per_sample=ps), 4, {})]
    t += [("bn_backward_coefs", EPI, "test_bn_backward_coefs", dict(n=1, c=70, with_gamma=True), 4, {})]
    t += [(f"avgpool_depth4_{'x'.join(map(str, s))}", P, "test_avgpool_depth4_autograd_vs_torch", dict(shape=s), 4, {})
          for s in ((1, 3, 10, 4, 4), (2, 2, 3, 5, 6))]
    t += [("small_ops", P, "test_small_ops", {}, 4, {})]     # mul_broadcast, argmax_rows (7, 1000), disparity_regression (2, 12, 5, 7)
    t += [(f"deconv_tail_gather_{'x'.join(map(str, s))}", "test_gpu_tail", "test_tail_gather_is_the_scatter_half_of_a_one_channel_transposed_layer",
           dict(shape=s, n=2), 16, {}) for s in ((3, 4, 33), (1, 1, 1))]
    t += [("zero_stuff2x", "test_gpu_neck2d", "test_zero_stuff_and_fused_deconv2d_vs_torch", {}, 8, {})]
    # --------------------------------------------------------------------------------------------------------- everything else
    t += [("volume_resample", P, "test_volume_resample_vs_grid_sample", dict(align=False), 4, {}),           # (2, 5, 6, 7, 9)
          ("rect_to_psv_grid", P, "test_psv_to_grid_chain_vs_torch", {}, 4, {}),
          ("roiaware_max", P, "test_roiaware_pool3d_bit_exact", dict(method="max", out_size=(3, 5, 2)), 4, ROI_ATOMICS),
          ("roiaware_avg", P, "test_roiaware_pool3d_bit_exact", dict(method="avg", out_size=(3, 5, 2)), 4, ROI_ATOMICS),
          ("points_in_boxes", P, "test_points_in_boxes", {}, 4, {}),
          ("iou3d_pairwise", "test_gpu_iou3d", "test_pairwise_matrix_forms", dict(case=IOU.BEV_CASES[0]), 4, {}),
          ("iou3d_odd_sizes", "test_gpu_iou3d", "test_empty_and_odd_sizes", {}, 4, {}),
          ("iou3d_nms", "test_gpu_iou3d", "test_nms_keep_lists_equal_the_reference", dict(n=IOU.NMS_SCENES[0][0], t=IOU.NMS_SCENES[0][1]), 4, {})]
    t += [(f"loss_{n}", "test_gpu_loss", "test_small_cases_against_the_reference", dict(name=n), 4, {}) for n in ("occ_odd", "depth", "focal")]
    t += [("loss_strided_mse", "test_gpu_loss", "test_strided_predictions", dict(name="mse"), 4, {})]
    t += [(f"targets_{n}", __name__, "targets_case", dict(name=n), 4, {}) for n in ("odd2d", "odd3d")]
    t += [(f"roi_crop_{m}", "test_gpu_roi_crop", "test_raw_crops_are_bit_equal", dict(name=RC.NAMES[0], mode=m, order="rgb"), 4, {})
          for m in ("fixed5", "exact")]
    t += [(f"decode_{n}", "test_gpu_decode", "test_cases_equal_the_host_route", dict(name=n), 4, {}) for n in (DEC.NAMES[0], "edges")]
    t += [("depth_forward", "test_gpu_depth", "test_forward_and_confidence_against_float64", dict(c=DC.COMPARED[0]), 4, {}),
          ("depth_backward", "test_gpu_depth", "test_backward_against_float64_autograd", dict(c=[c for c in DC.CASES if c.grad][0]), 4, {}),
          ("depth_points", "test_gpu_depth", "test_points_are_bit_equal_to_the_reference", dict(c=DC.POINTS_BY_NAME["single"], filt="all"), 4, {}),
          ("depth_points_compact", "test_gpu_depth", "test_compaction_keeps_the_pixel_order", dict(c=DC.POINTS_BY_NAME["single"], variant="half"), 4, {}),
          ("fc_eval", "test_gpu_fcmodel", "test_eval_against_the_references_float64", dict(c=FC.EVAL_CASES[0], hip=True), 16, {}),
          ("fc_train_step", "test_gpu_fcmodel", "test_training_step_against_the_references_float64", dict(c=FC.TRAIN_CASES[0]), 4, {}),
          ("hrnet_fusion", "test_gpu_hrnet", "test_fusion_forward_and_backward_against_torch", dict(case=HR.FUSE_CASES[0], offset=1), 4, {}),
          ("dsgn_spp_pool", "test_gpu_dsgn", "test_spp_pool_vs_avg_pool2d", dict(hw=(64, 100)), 4, {}),
          ("dsgn_spp_upsample", "test_gpu_dsgn", "test_spp_upsample_vs_interpolate", dict(hw=(37, 53), align=False), 4, {}),
          ("dsgn_dilated", "test_gpu_dsgn", "test_dilated_layer_vs_torch", dict(cin=16, cout=16, hw=(37, 53)), 4, {})]
    t += [(f"conv2d_{cin}_{cout}_k{k}s{s}", "test_gpu_neck2d", "test_fused_conv2d_vs_torch", dict(k=k, stride=s, cin=cin, cout=cout, hw=hw), 4, {})
          for cin, cout, hw in ((9, 32, (6, 4)), (64, 27, (13, 34))) for k in (1, 3) for s in (1, 2)]
    # one row per data-gradient kind of the 2D autograd function (tests/test_gpu_neck2d_backward.py, run unchanged): the [::2, ::2] scatter
    # at odd extents, the cropped transposed layer, the stride-2 layer behind the transposed one, the flattened 1x1 layer
    t += [(f"neck2d_backward_{n}", "test_gpu_neck2d_backward", "test_row", dict(row=NB.BY_NAME[n]), 4, {})
          for n in ("k1s2_odd_bn_relu", "k3s2_odd_bn_relu", "deconv_bn_relu_res", "whole_bias_sigmoid")]
    return t


CASES = _table()
RUNS = [(c, off) for c in CASES for off in (0, c[4]) if off is not None]


@pytest.mark.parametrize("case,off", RUNS, ids=[f"{c[0]}-{'aligned' if not off else 'off%d' % off}" for c, off in RUNS])
def test_guarded(case, off):
    _, module, name, kwargs, _, options = case
    GD.run_existing(module, name, kwargs, DEV, off, **options)


def test_a_planted_write_on_the_device_is_reported():
    """The harness on device memory: a plain torch write one element past an output -- inside the arena, nothing faults -- is seen after
    the stream has drained, for that allocation and that side, and a read past a placed operand is NaN."""
    import torch
    with GD.guarded(DEV, 8 << 20, check_on_exit=False) as g:
        out = torch.empty((3, 37), dtype=torch.float32, device=DEV)
        x = g.place(torch.ones(5), misalign=4)
        assert x.device.type == "cuda" and x.data_ptr() % 256 == 4 and g.violations() == []
        assert torch.isnan(x.as_strided((6,), (1,), x.storage_offset()).sum())
        out.as_strided((1,), (1,), out.storage_offset() + out.numel()).fill_(1.0)
        found = g.violations()
    assert len(found) == 1 and found[0].startswith("after empty (3, 37) torch.float32") and "4 guard bytes changed" in found[0], found
