/*
 * snvc_forms.h -- which kernel form the geometry launchers of libsnvc_hip.so take: the cost volume (csrc/cost_volume.hip) and the
 * feature -> voxel gather in both directions (csrc/voxel_gather.hip, csrc/voxel_gather_bwd.hip); and which form the weight
 * gradient of the 3D convolutions takes (csrc/conv3d_bwd.hip; last section).  Kept apart from snvc_hip.h,
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

#ifdef __cplusplus
}
#endif
#endif /* SNVC_FORMS_H */
