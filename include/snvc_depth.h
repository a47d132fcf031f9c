/*
 * snvc_depth.h -- C ABI of the depth read-out and the pseudo-LiDAR projection in libsnvc_hip.so (gfx950), the native side
 * of snvc_amd.depth.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header versions
 * itself through snvc_depth_abi_version().
 *
 * Conventions are those of snvc_hip.h and snvc_fc.h: device pointers unless said otherwise, `stream` is a hipStream_t
 * passed as void* (NULL = default stream), every call is asynchronous on it, allocates nothing and never waits for the
 * device, int status return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.
 * Every argument the host can see is checked before anything is launched.  All tensors are dense row-major float32 unless
 * said otherwise.  There are no atomics and every sum has a fixed order, so the same input gives the same bits.
 *
 * The read-out: depth[n][y][x] = sum_d softmax_d(U[n][.][y][x])[d] * levels[d], U the trilinear
 * interpolation of cost [N][D][H][W] to [N][D_out][H_out][W_out] by F.interpolate's coordinate rule.  Per axis with input
 * extent I, output extent O and scale s (align_corners == 0: s = I / O, src = max(0, s * (o + 0.5) - 0.5); align_corners
 * != 0: s = (I - 1) / (O - 1), or 0 when O == 1, src = s * o; s and src in float32): i0 = min(floor(src), I - 1), i1 =
 * min(i0 + 1, I - 1), t = src - i0, value = (1 - t) * v[i0] + t * v[i1].  U is never stored.
 */
#ifndef SNVC_DEPTH_H
#define SNVC_DEPTH_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_depth_abi_version(void);

/* Largest D and D_out the read-out takes (the planes are walked in chunks that fit the LDS, so the bound is one of index
 * width, not of LDS size); beyond it the calls return SNVC_ERR_UNSUPPORTED.  H_out >= H and W_out >= W are required: the
 * tiling assumes up-sampling (SNVC_ERR_UNSUPPORTED otherwise). */
enum { SNVC_DEPTH_MAX_PLANES = 2048 };

/* Pixels per block of the compaction's count / scan / write passes. */
enum { SNVC_DEPTH_POINTS_BLOCK = 256 };

/* Forward, one launch: a workgroup owns an 8 x 64 tile of output pixels, stages the planes of the tile's low-resolution
 * footprint in LDS (32 KiB at a time) and every lane walks d_out for its pixels with an online softmax.  cost [N][D][H][W]; levels [D_out];
 * depth [N][H_out][W_out].  Optional outputs of the same shape as depth (NULL = not written): conf = the largest
 * probability over d_out = 1 / z; m = the largest logit; z = the sum over d_out of exp(U - m).  m and z are what the
 * backward reads.  A zero extent returns SNVC_OK unlaunched. */
SNVC_API int snvc_depth_readout_forward(const float *cost, const float *levels, float *depth, float *conf, float *m, float *z,
                                        int64_t N, int64_t D, int64_t H, int64_t W, int64_t D_out, int64_t H_out, int64_t W_out,
                                        int align_corners, void *stream);

/* Backward with respect to cost, one launch, gather form: a workgroup owns a tile of 4 x 16 low-resolution columns and a
 * range of planes, restages their footprint (one column and one plane of halo on every side), recomputes the probabilities of
 * the output pixels that touch its columns from m and z, and every thread sums the contributions of one column's planes
 * in a fixed order.  gy [N][H_out][W_out] is the gradient of depth; depth, m, z are the forward's; dcost [N][D][H][W] is
 * written whole (no zero-fill needed before the call). */
SNVC_API int snvc_depth_readout_backward(const float *cost, const float *levels, const float *depth, const float *m, const float *z,
                                         const float *gy, float *dcost, int64_t N, int64_t D, int64_t H, int64_t W, int64_t D_out,
                                         int64_t H_out, int64_t W_out, int align_corners, void *stream);

/* Rectified-camera points of a depth map [N][H][W].  P is [3][4] (p_per_sample == 0) or [N][3][4].  For pixel (i, j): u =
 * origin_u + j * stride_u, v = origin_v + i * stride_v, x = ((u - P[0][2]) * z) / P[0][0] + P[0][3] / (-P[0][0]), y = ((v -
 * P[1][2]) * z) / P[1][1] + P[1][3] / (-P[1][1]); every operation is one correctly rounded float32 operation in that order
 * (nothing is contracted).  A point is valid when z is finite, z_lo <= z < z_hi and, with conf [N][H][W] not NULL, conf >=
 * min_conf.  points [N][H][W][3] holds (x, y, z), zeros where invalid; valid [N][H][W] is uint8 0 / 1. */
SNVC_API int snvc_depth_to_points(const float *depth, const float *P, int p_per_sample, const float *conf, float min_conf, float z_lo,
                                  float z_hi, float origin_u, float origin_v, float stride_u, float stride_v, float *points,
                                  uint8_t *valid, int64_t N, int64_t H, int64_t W, void *stream);

/* Bytes of the workspace snvc_depth_to_points_compact needs (one int32 per block of SNVC_DEPTH_POINTS_BLOCK pixels and
 * sample), or < 0 if a size is negative or H * W is 2^31 or more. */
SNVC_API int64_t snvc_depth_points_workspace_bytes(int64_t N, int64_t HW);

/* The same points, compacted in order: sample n's first counts[n] rows of points [N][H * W][3] are its valid points in
 * row-major pixel order, the rows after them are zero; counts is int32 [N].  Three launches on the stream (a count per
 * block, an exclusive scan per sample, the writes); nothing comes back to the host.  workspace: 4-byte aligned,
 * snvc_depth_points_workspace_bytes(N, H * W) bytes. */
SNVC_API int snvc_depth_to_points_compact(const float *depth, const float *P, int p_per_sample, const float *conf, float min_conf,
                                          float z_lo, float z_hi, float origin_u, float origin_v, float stride_u, float stride_v,
                                          void *workspace, float *points, int32_t *counts, int64_t N, int64_t H, int64_t W,
                                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_DEPTH_H */
