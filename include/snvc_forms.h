/*
 * snvc_forms.h -- which kernel form the geometry launchers of libsnvc_hip.so take: the cost volume (csrc/cost_volume.hip) and the
 * feature -> voxel gather in both directions (csrc/voxel_gather.hip, csrc/voxel_gather_bwd.hip); and which form the weight
 * gradient of the 3D convolutions takes (csrc/conv3d_bwd.hip), which form their fp32 forward takes (csrc/conv3d.hip) and which
 * rows per workgroup, depth chunks and column chunks the first-layer kernels take (csrc/sheared_conv.hip; last section).  Kept apart
 * from snvc_hip.h,
 * whose declaration set and ABI number are pinned; this header versions itself through snvc_forms_abi_version().
 *
 * Every launcher decides its form in one host function, from the sizes, the element type, the alignment of its operands and the
 * compute-unit count of the current device (256 when there is none).  The queries below call that same function and launch
 * nothing: host code only, no device needed, no pointer is read.  A test asks the query which form its shape takes before it
 * compares values, so that a case which stops reaching its form fails instead of passing on a sibling.
 *
 * Return value of every query: a form id of the entry point's enum (> 0); 0 when the launcher would return SNVC_OK without a
 * launch (an empty tensor); or -(snvc_status) when the launcher refuses the arguments -- the same code, with the same text in
 * snvc_last_error_string(), that the entry point itself gives for these sizes.  What only a pointer can show (NULL operands)
 * is not checked here.  `info` (SNVC_FORMS_INFO int64 values, not NULL) receives what the launch will use; slots that a form
 * does not use are 0.
 *
 * `aligned` is a mask of what is 16-byte aligned: SNVC_FORMS_ALIGNED_IN -- the tensors read (cost volume: left and right;
 * gather: both coordinate arrays); SNVC_FORMS_ALIGNED_OUT -- what is written (the output or outputs, and the gather's
 * channels-last workspace, which must also be there).  The two backward queries take no mask: no backward form depends on
 * alignment (the cost-volume kernels read 4-byte-aligned pairs, the gather's adjoints are scalar; the sorted form's workspace
 * must be 256-byte aligned, which only the pointer shows).
 */
#ifndef SNVC_FORMS_H
#define SNVC_FORMS_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature or enum change. */
SNVC_API int snvc_forms_abi_version(void);

enum { SNVC_FORMS_INFO = 8 };
enum { SNVC_FORMS_ALIGNED_IN = 1, SNVC_FORMS_ALIGNED_OUT = 2, SNVC_FORMS_ALIGNED_ALL = 3 };

/* snvc_cost_volume_forward / snvc_cost_volume_forward_right (right_only != 0).
 * info: [0] RB rows per workgroup, [1] hblocks row blocks per plane, [2] dsplit depth chunks, [3] dchunk planes per chunk,
 *       [4] grid.x, [5] grid.y, [6] threads per workgroup, [7] dynamic LDS bytes. */
enum snvc_cost_volume_forward_form_id {
    SNVC_CVF_ROWS = 1,          /* cost_volume_fwd_rows<true>: fp32, downsample 1, W % 4 == 0, W <= 2048, aligned */
    SNVC_CVF_ROWS_RIGHT = 2,    /* cost_volume_fwd_rows<false>: the same kernel without the left half (snvc_cost_volume_forward_right) */
    SNVC_CVF_F32X4 = 3,         /* cost_volume_fwd_f32x4: as ROWS but W > 2048 (or N*C*H >= 2^30) */
    SNVC_CVF_F64X2 = 4,         /* cost_volume_fwd_f64x2: fp64, downsample 1, W % 2 == 0, aligned */
    SNVC_CVF_GENERIC_F32 = 5,   /* cost_volume_fwd_generic<float> */
    SNVC_CVF_GENERIC_F64 = 6    /* cost_volume_fwd_generic<double> */
};
SNVC_API int snvc_cost_volume_forward_form(int64_t N, int64_t C, int64_t Hi, int64_t Wi, int64_t D, int64_t downsample, int dtype,
                                           int right_only, int aligned, int64_t *info);

/* snvc_cost_volume_backward / snvc_cost_volume_backward_right (right_only != 0; downsample must then be 1).  H, W are the
 * volume's, as in the entry points.  info: [4] grid.x, [6] threads per workgroup. */
enum snvc_cost_volume_backward_form_id {
    SNVC_CVB_ROWS = 1,          /* cost_volume_bwd_rows_f32<true>: fp32, downsample 1, W >= 2 */
    SNVC_CVB_ROWS_RIGHT = 2,    /* cost_volume_bwd_rows_f32<false> (snvc_cost_volume_backward_right) */
    SNVC_CVB_GATHER_F32 = 3,    /* cost_volume_bwd_gather<float>: downsample > 1 or W == 1 */
    SNVC_CVB_GATHER_F64 = 4     /* cost_volume_bwd_gather<double> */
};
SNVC_API int snvc_cost_volume_backward_form(int64_t N, int64_t C, int64_t H, int64_t W, int64_t D, int64_t downsample, int dtype,
                                            int right_only, int64_t *info);

/* The gather's forward.  kind: which entry point -- snvc_voxel_gather_forward_ws (fp32 output), snvc_voxel_gather_forward_f16 (C8
 * half) or snvc_voxel_gather_forward_split (a split C8 pair).
 * info: [0] run voxels per workgroup (LDS forms), [1] nruns, [2] 1 when the crop resolution takes the reciprocal-multiply
 *       normalisation (both extents powers of two; LDS forms), [3] channel slices per run (LDS forms), [4] grid.x, [5] grid.y * grid.z (the batch),
 *       [6] threads per workgroup, [7] dynamic LDS bytes. */
enum snvc_voxel_gather_kind { SNVC_GATHER_F32 = 0, SNVC_GATHER_C8 = 1, SNVC_GATHER_SPLIT = 2 };
enum snvc_voxel_gather_forward_form_id {
    SNVC_GF_PLAIN = 1,          /* voxel_gather_fwd: no (aligned) workspace, F % 4 != 0 or F > 256 */
    SNVC_GF_CL = 2,             /* voxel_gather_fwd_cl: channels-last maps, one voxel per thread (V % 4 != 0 or unaligned) */
    SNVC_GF_CL_X4 = 3,          /* voxel_gather_fwd_cl_x4: four voxels per thread (V < 4096 or a plane beyond the LDS form) */
    SNVC_GF_LDS = 4,            /* voxel_gather_fwd_lds<4, 0, 512, .>: Hf * Wf <= 4608, V >= 4096 */
    SNVC_GF_CL_C8 = 5,          /* voxel_gather_fwd_cl_c8 */
    SNVC_GF_LDS_C8 = 6,         /* voxel_gather_fwd_lds<8, 1, 1024, .> */
    SNVC_GF_LDS_SPLIT = 7       /* voxel_gather_fwd_lds<8, 2, 1024, .> */
};
SNVC_API int snvc_voxel_gather_forward_form(int kind, int64_t N, int64_t F, int64_t Hf, int64_t Wf, int64_t V, float res_x, float res_y,
                                            int aligned, int64_t *info);

/* The gather's adjoint: snvc_voxel_gather_backward_det (deterministic != 0) or snvc_voxel_gather_backward.
 * info: [0] vchunk voxels per workgroup (LDS atomics), [1] voxel chunks = grid.x (LDS atomics), [2] channel passes of 64 per
 *       piece (sorted), [3] the sorted form's upper bound of pieces = its grid.x, [4] grid.x, [5] grid.y, [6] threads per
 *       workgroup, [7] dynamic LDS bytes. */
enum snvc_voxel_gather_backward_form_id {
    SNVC_GB_LDS_ATOMICS = 1,    /* voxel_gather_bwd_lds<2>: two channel planes fit 64 KiB of LDS */
    SNVC_GB_GLOBAL_ATOMICS = 2, /* voxel_gather_bwd */
    SNVC_GB_SORTED = 3          /* keys, radix sort, gather_bwd_pieces_kernel<64>, combine: no atomics */
};
SNVC_API int snvc_voxel_gather_backward_form(int64_t N, int64_t F, int64_t Hf, int64_t Wf, int64_t V, int deterministic, int64_t *info);

/* snvc_conv3d_wgrad / snvc_conv3d_wgrad_amax (csrc/conv3d_bwd.hip): the plan the launcher itself makes for this descriptor.  x_align /
 * g_align: the largest of 16 / 8 / 4 that divides the address of x / g.  The forms in their order of precedence; a layer that misses
 * a condition takes the next form of its key (ksize, stride, dilation).  vec: rows and batch strides of both operands in whole
 * pieces of 4 floats (2: g in pieces of 2) at aligned addresses, without SNVC_ALGO_SCALAR_STAGING; flat16: both tensors readable
 * as 16-byte aligned float4 streams.
 * info: [0] bytes of a staging piece (16 / 8 / 4), [1] workspace bytes the form's kernels touch (never more than
 *       snvc_conv3d_wgrad_workspace_bytes; the split-operand forms keep their amax words at its end), [2] split-operand forms: dparts
 *       depth parts; 12-wave forms: P partitions; k1: voxel chunks; generic forms: partitions, [3] split-operand forms: dchunk planes per
 *       part; 12-wave forms: upx units per XCD; generic forms: tap chunks (grid.z), [4] grid.x, [5] grid.y * grid.z, [6] threads per
 *       workgroup, [7] dynamic LDS bytes. */
enum snvc_conv3d_wgrad_form_id {
    SNVC_WG_K1_STREAM = 1,      /* wgrad_k1_small_partial + _final: k1, stride 1, Cout <= 2, D*H*W % 4 == 0, 16-byte aligned operands */
    SNVC_WG_X3 = 2,             /* conv3d_wgrad_x3_kernel<16- | 8-byte rows>: key 311, flat16, vec == 4 or 8-byte rows on both grids, neither
                                   WGRAD_FP32 nor DIRECT, columns x depth parts within the slab budget */
    SNVC_WG_WINO = 3,           /* conv3d_wgrad_wino_kernel: key 311, vec == 4, not DIRECT */
    SNVC_WG_X3S2 = 4,           /* conv3d_wgrad_x3s2_kernel: key 321, flat16, vec 4 or 2, neither WGRAD_FP32 nor DIRECT, the big grid
                                   exactly twice the small one, slab budget */
    SNVC_WG_S2 = 5,             /* conv3d_wgrad_s2_kernel<4 | 2>: key 321, flat16, vec 4 or 2, not DIRECT */
    SNVC_WG_KSPLIT = 6,         /* conv3d_wgrad_kernel<K-split WgradCfg, 4 | 2>: keys 311 / 321 with vec != 0 */
    SNVC_WG_TAPS = 7            /* conv3d_wgrad_kernel<tap-split WgradCfg, 0>: keys 111, 311, 321, 511, 512, 711, scalar staging */
};
SNVC_API int snvc_conv3d_wgrad_form(const snvc_conv3d_desc *desc_host, int x_align, int g_align, int64_t *info);

/* snvc_conv3d_forward / _forward_ex / _forward_head / _forward_side_head / _forward_stats (csrc/conv3d.hip): what the dispatcher
 * itself launches for this call.  entry: which entry point is meant.  *_align: the largest of 16 / 8 / 4 that divides the address of
 * x, y, the residual, the depth planes and y_head; 0 for a NULL pointer (y of forward_head; a residual or planes that are not
 * given).  The families are tried in the order of the enum's sections; a layer that misses a condition of one goes to the next, and
 * every layer make_plan accepts ends on the direct (or transposed) MFMA configuration of its key.  In the conditions:
 *   vec16: Win % 4 == 0, x 16-byte aligned, x batch stride % 4 == 0;  vec8: the same for 2 and 8 bytes;
 *   fastc: Dout*Hout*Wout < 2^27, Cout % 32 == 0, no Sigmoid, no SNVC_ALGO_GENERIC_EPILOGUE;
 *   epi16: Wout % 4 == 0, y and residual batch strides % 4 == 0, y / residual / planes 16-byte aligned;  fast = fastc && epi16;
 *   pair8: Wout % 2 == 0, y and residual batch strides % 2 == 0, y / residual (/ planes) 8-byte aligned;
 *   stream16: x / y / residual 16-byte aligned, all three batch strides % 4 == 0.
 * info: [0] bytes of an input staging piece (16 / 8 / 4), [1] the epilogue variant as the kernel's template argument -- direct forms:
 *       EPI 0 generic, 1 fast, 2 fast with residual; transposed forms: EPI 0..2 as before, 3 / 4 fused head without / with residual,
 *       5 statistics; Winograd forms: RES + 2 * PLANE + 4 * XMODE (XMODE 1 side head, 2 depth-4 average, 3 statistics); streaming
 *       and VALU forms: 0, [2] tiles (direct, transposed, K3_COUT1), jobs (Winograd) or 16-byte pieces per channel (streaming forms),
 *       [3] channel groups, [4] grid.x, [5] grid.y * grid.z, [6] threads per workgroup, [7] dynamic LDS bytes. */
enum snvc_conv3d_forward_entry {
    SNVC_CFE_FORWARD = 0,      /* snvc_conv3d_forward, snvc_conv3d_forward_ex */
    SNVC_CFE_HEAD = 1,         /* snvc_conv3d_forward_head */
    SNVC_CFE_SIDE_HEAD = 2,    /* snvc_conv3d_forward_side_head */
    SNVC_CFE_STATS = 3         /* snvc_conv3d_forward_stats */
};
enum snvc_conv3d_forward_form_id {
    /* streaming and VALU forms (not for depth-1 layers) */
    SNVC_CF_POINTWISE_SMALL_1 = 1,  /* pointwise_small_kernel<1>: k1, stride 1, Cout == 1, D*H*W % 4 == 0, stream16 */
    SNVC_CF_POINTWISE_SMALL_2 = 2,  /* pointwise_small_kernel<2>: the same with Cout == 2 */
    SNVC_CF_POINTWISE_EXPAND_1 = 3, /* pointwise_expand_kernel<1>: k1, stride 1, Cin == 1, Cout > 2, D*H*W % 4 == 0, stream16, no planes /
                                       head / statistics, no SNVC_ALGO arithmetic bits */
    SNVC_CF_POINTWISE_EXPAND_2 = 4, /* pointwise_expand_kernel<2>: the same with Cin == 2 */
    SNVC_CF_K3_COUT1 = 5,           /* conv3d_k3_cout1_kernel: 3x3x3, stride 1, dilation 1, Cout == 1, no planes */
    SNVC_CF_DECONV_COUT1 = 6,       /* deconv3d_cout1_kernel (csrc/conv3d_small.hip): transposed, Cout == 1, no head, Win % 4 == 0, stream16 */
    /* Winograd, 3x3x3 stride 2: vec16, fast or (fastc && pair8), no planes, not SNVC_ALGO_DIRECT */
    SNVC_CF_WINO_S2_PIPE4 = 7,      /* conv3d_winos2_pipe_kernel<WinoS2PipeCfg<4>>: fast, not SNVC_ALGO_WINO_TILE_STD; carries the statistics */
    SNVC_CF_WINO_S2_PIPE2 = 8,      /* conv3d_winos2_pipe_kernel<WinoS2PipeCfg<2>>: 8-byte output rows, not WINO_TILE_STD */
    SNVC_CF_WINO_S2 = 9,            /* conv3d_winok_kernel<CfgWinoS2>: WINO_TILE_STD, fast */
    SNVC_CF_WINO_S2_V8 = 10,        /* conv3d_winok_kernel<CfgWinoS2v8>: WINO_TILE_STD, 8-byte output rows */
    /* Winograd, k5 / k7 stride 1: vec16, fast, no planes, not SNVC_ALGO_DIRECT */
    SNVC_CF_WINO_K5 = 11,           /* conv3d_winok_kernel<CfgWinoK5> */
    SNVC_CF_WINO_K5D2 = 12,         /* conv3d_winok_kernel<CfgWinoK5D2>: dilation 2 */
    SNVC_CF_WINO_K7 = 13,           /* conv3d_winok_kernel<CfgWinoK7> */
    /* Winograd, depth-1 3x3 stride 1 */
    SNVC_CF_WINO_P = 14,            /* conv3d_wino_dma_kernel<CfgWinoP>: Hout, Wout >= 32, vec16, fast, not DIRECT, no planes / head / pooling /
                                       statistics, SNVC_ALGO_WINO_TILE_BIG or at least two jobs (1 x 16 x 32 tiles) per CU */
    /* Winograd, 3x3x3 stride 1: pair8, fastc, wide (vec16 && epi16) or vec8, not SNVC_ALGO_DIRECT */
    SNVC_CF_WINO_BIG = 15,          /* conv3d_wino_dma_kernel<CfgWinoBig>: SNVC_ALGO_WINO_TILE_BIG and wide */
    SNVC_CF_WINO_N3 = 16,           /* conv3d_wino_dma_kernel<CfgWinoN3>: the default form -- wide, no tile bits (or BIG without wide); the only
                                       one that carries the side head, the depth-4 average and the statistics */
    SNVC_CF_WINO_N = 17,            /* conv3d_wino_kernel<CfgWinoN>: SNVC_ALGO_WINO_TILE_NARROW_REG and wide */
    SNVC_CF_WINO_N8 = 18,           /* conv3d_wino_kernel<CfgWinoN8>: not wide (8-byte rows), tile bits other than STD */
    SNVC_CF_WINO = 19,              /* conv3d_wino_kernel<CfgWino>: SNVC_ALGO_WINO_TILE_STD and wide */
    SNVC_CF_WINO8 = 20,             /* conv3d_wino_kernel<CfgWino8>: SNVC_ALGO_WINO_TILE_STD, not wide */
    /* direct MFMA forms, by (ksize, stride, dilation); M2: Cout > 32.  EPI 1 / 2 where the configuration builds them (K3S2*, K5M1,
     * K7M1, P3*): fast and no planes */
    SNVC_CF_K1M1 = 21, SNVC_CF_K1M2 = 22,       /* conv3d_mfma_kernel<CfgK1M1 | CfgK1M2> */
    SNVC_CF_K3M1 = 23, SNVC_CF_K3M2 = 24,       /* <CfgK3M1 | CfgK3M2> */
    SNVC_CF_K3S2M1 = 25, SNVC_CF_K3S2M2 = 26,   /* <CfgK3S2M1 | CfgK3S2M2> */
    SNVC_CF_K5M1 = 27, SNVC_CF_K5M2 = 28,       /* <CfgK5M1 | CfgK5M2> */
    SNVC_CF_K5D2M1 = 29, SNVC_CF_K5D2M2 = 30,   /* <CfgK5D2M1 | CfgK5D2M2> */
    SNVC_CF_K7M1 = 31, SNVC_CF_K7M2 = 32,       /* <CfgK7M1 | CfgK7M2> */
    /* depth-1 direct forms (ksize_d == 1), one 32-channel group per workgroup */
    SNVC_CF_P1M1S = 33,             /* <CfgP1M1s>: k1 */
    SNVC_CF_P1S2M1S = 34,           /* <CfgP1S2M1s>: k1, stride 2 */
    SNVC_CF_P3M1S = 35,             /* <CfgP3M1s>: k3 */
    SNVC_CF_P3S2M1S = 36,           /* <CfgP3S2M1s>: k3, stride 2 */
    SNVC_CF_P7M1S = 37,             /* <CfgP7M1s>: 3 (H) x 7 (W) */
    SNVC_CF_P3D2M1S = 38,           /* <CfgP3D2M1s>: k3, dilation 2 */
    /* transposed MFMA forms (k3, s2, p1, op1); y / residual 8-byte aligned.  EPI 3 / 4 (forward_head) and 5 (statistics) on DCM1 alone */
    SNVC_CF_DCM1 = 39,              /* deconv3d_mfma_kernel<CfgDCM1>: Cout <= 32 or Cout % 32 == 0; vec16 or not even vec8 */
    SNVC_CF_DCM2 = 40,              /* <CfgDCM2>: Cout > 32 and Cout % 32 != 0 */
    SNVC_CF_DCM1_V8 = 41,           /* <CfgDCM1v8>: as DCM1, vec8 without vec16 */
    SNVC_CF_DCM2_V8 = 42,           /* <CfgDCM2v8>: as DCM2, vec8 without vec16 */
    SNVC_CF_DCP = 43,               /* <CfgDCP>: the depth-1 transposed layer */
    SNVC_CF_DCP_V8 = 44             /* <CfgDCPv8>: vec8 without vec16 */
};
SNVC_API int snvc_conv3d_forward_form(const snvc_conv3d_desc *desc_host, int entry, int x_align, int y_align, int res_align,
                                      int planes_align, int y_head_align, int64_t *info);

/* The first-layer family (csrc/sheared_conv.hip): the sheared and the any-shift first convolution.  entry: which entry point is
 * meant; the sizes are the entry point's own (WG / WG2: row lengths of g and gcol; entries that do not take q, m0, WG, WG2 or flags
 * ignore them).  The form id names the kernel instantiation.  Every launcher takes its rows per workgroup, chunks and LDS bytes from
 * one host function, and the query reports what that function returns.
 * info: [0] RB rows per workgroup, [1] row blocks (the last one holds H - (blocks - 1) * RB rows), [2] depth chunks (split
 *       producers; chunk k holds planes k * per_chunk .. min(D, (k + 1) * per_chunk) - 1, none when k * per_chunk >= D) or column
 *       chunks (weight gradient), [3] planes per chunk, columns per chunk (weight gradient) or the row width in threads
 *       (warped_expand_backward), [4] grid.x, [5] grid.y * grid.z, [6] threads per workgroup, [7] dynamic LDS bytes. */
enum snvc_first_layer_entry {
    SNVC_FLE_SHEARED_EXPAND = 0,            /* snvc_sheared_expand, snvc_sheared_expand_amax without amax words */
    SNVC_FLE_SHEARED_EXPAND_AMAX = 1,       /* snvc_sheared_expand_amax with amax words */
    SNVC_FLE_SHEARED_EXPAND_STATS = 2,      /* snvc_sheared_expand_stats */
    SNVC_FLE_SHEARED_EXPAND_SPLIT = 3,      /* snvc_sheared_expand_split */
    SNVC_FLE_SHEARED_BACKWARD_REDUCE = 4,   /* snvc_sheared_backward_reduce */
    SNVC_FLE_SHEARED_REDUCE = 5,            /* snvc_sheared_reduce */
    SNVC_FLE_WARPED_EXPAND = 6,             /* snvc_warped_expand; flags & SNVC_WARPED_EXPAND_R3 selects the r3 kernel */
    SNVC_FLE_WARPED_EXPAND_SPLIT = 7,       /* snvc_warped_expand_split */
    SNVC_FLE_WARPED_EXPAND_BACKWARD = 8     /* snvc_warped_expand_backward */
};
enum snvc_first_layer_form_id {
    SNVC_FL_EXPAND_Q1 = 1, SNVC_FL_EXPAND_Q2 = 2, SNVC_FL_EXPAND_Q4 = 3,                  /* sheared_expand_kernel<Q, 0> */
    SNVC_FL_EXPAND_AMAX_Q1 = 4, SNVC_FL_EXPAND_AMAX_Q2 = 5, SNVC_FL_EXPAND_AMAX_Q4 = 6,   /* sheared_expand_kernel<Q, 2> */
    SNVC_FL_STATS_Q1 = 7, SNVC_FL_STATS_Q2 = 8,                                           /* sheared_expand_kernel<Q, 1> + the norm finalize */
    SNVC_FL_SPLIT_Q1 = 9, SNVC_FL_SPLIT_Q2 = 10, SNVC_FL_SPLIT_Q4 = 11,                   /* sheared_expand_split_kernel<Q> */
    SNVC_FL_BWD_Q1 = 12, SNVC_FL_BWD_Q2 = 13,                                             /* sheared_bwd_kernel<Q> + sheared_fold_kernel */
    SNVC_FL_REDUCE_Q1 = 14, SNVC_FL_REDUCE_Q2 = 15,                                       /* sheared_reduce_kernel<Q> */
    SNVC_FL_WARPED_WIN = 16,                /* warped_expand_win_kernel */
    SNVC_FL_WARPED_R3 = 17,                 /* warped_expand_kernel (SNVC_WARPED_EXPAND_R3) */
    SNVC_FL_WARPED_SPLIT = 18,              /* warped_expand_split_kernel */
    SNVC_FL_WARPED_BWD = 19,                /* warped_expand_bwd_kernel */
    SNVC_FL_WGRAD = 20                      /* sheared_wgrad_kernel + sheared_wgrad_reduce_kernel */
};
SNVC_API int snvc_first_layer_form(int entry, int64_t N, int64_t C, int64_t D, int64_t H, int64_t W, int q, int m0, int64_t WG, int64_t WG2,
                                   int flags, int64_t *info);
/* snvc_sheared_wgrad.  info: [2] column chunks, [3] columns per chunk (the last chunk holds WU - (chunks - 1) * cols), [4] grid.x =
 * H * chunks, [5] channel groups * N, [6] threads per workgroup. */
SNVC_API int snvc_sheared_wgrad_form(int64_t N, int64_t C, int64_t CO, int64_t H, int64_t WU, int64_t *info);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_FORMS_H */
