/*
 * snvc_iou3d.h -- C ABI of the rotated-box IoU / NMS family in libsnvc_hip.so (gfx950), the native side of
 * snvc.extension.iou3d_nms.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this
 * header versions itself through snvc_iou3d_abi_version().
 *
 * Conventions are those of snvc_hip.h: device pointers unless the name ends in _host, `stream` is a hipStream_t
 * passed as void* (NULL = default stream), every call is asynchronous on it and allocates nothing, int status
 * return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.
 *
 * Boxes are float32 [x, y, z, dx, dy, dz, heading], row-major, heading counter-clockwise about +z.
 *
 * BEV overlap follows the reference's definition (iou3d_nms_kernel.cu box_overlap), not exact clipping: the
 * overlap polygon is the proper crossings of the two outlines (touching and collinear edges add none) plus each
 * box's corners that lie strictly inside the other box grown by 1e-2 on each half-extent; its area is the
 * shoelace area of those points in angular order about their mean.  Two 2x2 boxes 5 mm apart therefore overlap
 * by 0.01 m^2.  Geometry is evaluated relative to the first box's centre.
 *   iou_bev = overlap / max(area_a + area_b - overlap, 1e-8)
 *   iou3d   = overlap * h / max(vol_a + vol_b - overlap * h, 1e-6),  h = height overlap of [z - dz/2, z + dz/2]
 */
#ifndef SNVC_IOU3D_H
#define SNVC_IOU3D_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_iou3d_abi_version(void);

enum { SNVC_IOU3D_OVERLAP = 0, SNVC_IOU3D_IOU_BEV = 1, SNVC_IOU3D_IOU_3D = 2 };
enum { SNVC_NMS_ROTATED = 0, SNVC_NMS_NORMAL = 1 };
#define SNVC_NMS_MAX_BOXES 65536

/* ------------------------------------------------------------------------------------
 * Pairwise BEV overlap / BEV IoU / 3D IoU
 * replaces: iou3d_nms_cuda.boxes_overlap_bev_gpu, boxes_overlap_bev_onebyone_gpu, boxes_iou_bev_gpu,
 *           boxes_iou_bev_onebyone_gpu (iou3d_nms.cpp:51-129, kernels iou3d_nms_kernel.cu:236-294), and the torch ops
 *           of boxes_iou3d_gpu (iou3d_nms_utils.py:53-87), fused into the `what = SNVC_IOU3D_IOU_3D` launch.
 *   onebyone == 0: out [num_a][num_b], out[i][j] = f(a_i, b_j); workspace of
 *                  snvc_iou3d_pairwise_workspace_bytes(num_a, num_b) bytes (per-box corners, cos/sin, area).
 *   onebyone != 0: num_b must equal num_a; out [num_a], out[i] = f(a_i, b_i); workspace unused (may be NULL).
 *   Every element of out is written.
 * ---------------------------------------------------------------------------------- */
SNVC_API int64_t snvc_iou3d_pairwise_workspace_bytes(int64_t num_a, int64_t num_b);
SNVC_API int snvc_iou3d_pairwise(const float *boxes_a, int64_t num_a, const float *boxes_b, int64_t num_b, int what,
                                 int onebyone, void *workspace, float *out, void *stream);

/* ------------------------------------------------------------------------------------
 * NMS over boxes sorted by descending score
 * replaces: iou3d_nms_cuda.nms_gpu / nms_normal_gpu (iou3d_nms.cpp:131-229, kernels iou3d_nms_kernel.cu:296-399)
 *   kind SNVC_NMS_ROTATED: rotated BEV IoU; SNVC_NMS_NORMAL: axis-aligned BEV IoU that ignores the heading.
 *   Box i suppresses box j > i when iou(box_i, box_j) > thresh (the higher-ranked box is the first argument).
 *   Two launches in stream order: the upper-triangle 64x64 tiles of the suppression mask, then one workgroup that
 *   walks the mask greedily.  keep [num_boxes] int64 receives the kept indices in rank order, num_keep [1] int32
 *   their count; both stay on the device.  0 <= num_boxes <= SNVC_NMS_MAX_BOXES (the mask of 65536 boxes is 512 MB).
 *   workspace: snvc_iou3d_nms_workspace_bytes(num_boxes) bytes, contents ignored.
 * ---------------------------------------------------------------------------------- */
SNVC_API int64_t snvc_iou3d_nms_workspace_bytes(int64_t num_boxes);
SNVC_API int snvc_iou3d_nms(const float *boxes, int64_t num_boxes, float thresh, int kind, void *workspace,
                            int64_t *keep, int32_t *num_keep, void *stream);

/* ------------------------------------------------------------------------------------
 * Backward of the differentiable one-by-one 3D IoU
 * replaces: BoxesIou3dDifferentiableFunction.backward (iou3d_nms_utils.py:164-174) with
 *           numerical_jaccobian.get_numerical_jacobian(fn, (a, b), a, eps) (numerical_jaccobian.py:17-57)
 *   grad_a[i][k] = grad[i] * (iou3d(a_i with a_ik = a_ik + eps, b_i) - iou3d(a_i with a_ik = a_ik - eps, b_i)) / (2 eps),
 *   every step in fp32 as the reference's torch code takes it.  boxes_a, boxes_b, grad_a [num][7], grad [num].
 * ---------------------------------------------------------------------------------- */
SNVC_API int snvc_iou3d_backward(const float *boxes_a, const float *boxes_b, const float *grad, int64_t num, float eps,
                                 float *grad_a, void *stream);

/* ------------------------------------------------------------------------------------
 * Host BEV IoU matrix (HOST function: host pointers, no device work, no stream), built from the same geometry code
 * replaces: iou3d_nms_cuda.boxes_iou_bev_cpu (iou3d_cpu.cpp:232-252)
 *   iou_host [num_a][num_b]
 * ---------------------------------------------------------------------------------- */
SNVC_API int snvc_iou3d_boxes_iou_bev_cpu(const float *boxes_a_host, int64_t num_a, const float *boxes_b_host,
                                          int64_t num_b, float *iou_host);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_IOU3D_H */
