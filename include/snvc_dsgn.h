/*
 * snvc_dsgn.h -- C ABI of the spatial-pyramid-pooling (SPP) head of the DSGN image backbone in libsnvc_hip.so (gfx950),
 * the native side of snvc_amd.models.submodule.feature_extraction.  Kept apart from snvc_hip.h, whose declaration set and
 * ABI number are pinned; this header versions itself through snvc_dsgn_abi_version().
 *
 * The backbone's convolutions (including the 3 x 3 / dilation-2 layers of layer4) are snvc_conv3d_forward launches on
 * depth-1 views (snvc_hip.h, desc.ksize_d = 1); only the pooling and the upsampling of the SPP branches live here.
 *
 * Conventions are those of snvc_hip.h: device pointers unless the name ends in _host, `stream` is a hipStream_t passed as
 * void* (NULL = default stream), every call is asynchronous on it and allocates nothing, int status return (snvc_status),
 * snvc_last_error_string() for the text of the last failure on the calling thread.  Every argument is checked on the host
 * before anything is launched.  Tensors are NCHW float32 with dense (C, H, W) planes; a batch stride (in elements, 0 =
 * dense) lets an input or output be a channel slice of a larger buffer.
 */
#ifndef SNVC_DSGN_H
#define SNVC_DSGN_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_dsgn_abi_version(void);

/* ------------------------------------------------------------------------------------
 * The four average pools of the SPP head in one pass over their input
 * replaces: nn.AvgPool2d((k, k), stride=(k, k)) for k = 64, 32, 16, 8 in branch1 .. branch4 of feature_extraction
 *           (submodule.py:424-442), each reading output_skip again.
 *   x [N][C][H][W] (batch stride x_batch_stride) is read once.  Partial windows are dropped, as in the reference:
 *   out_k [N][C][H / k][W / k], contiguous, for k = 8, 16, 32, 64 (out8, out16, out32, out64).
 *   Each 8 x 8 window is summed row by row, left to right, then divided by 64 (the order of F.avg_pool2d: out8 is
 *   bit-exact); a window of 16, 32 or 64 is the sum of its 8 x 8 window sums (row-major), divided by k * k.
 *   Needs H >= 64, W >= 64 and (H / 8) * (W / 8) <= SNVC_DSGN_MAX_CELLS (the 8 x 8 sums of one plane are kept in LDS).
 * ---------------------------------------------------------------------------------- */
#define SNVC_DSGN_MAX_CELLS 8192
SNVC_API int snvc_dsgn_spp_pool(const float *x, int64_t x_batch_stride, float *out8, float *out16, float *out32, float *out64,
                                int64_t N, int64_t C, int64_t H, int64_t W, void *stream);

/* ------------------------------------------------------------------------------------
 * Bilinear upsampling of the four SPP branch maps straight into their channel slices of the concat buffer
 * replaces: the four F.interpolate(branch, (H, W), mode='bilinear', align_corners=...) calls and their part of the
 *           torch.cat of feature_extraction.forward (submodule.py:478-512).
 *   maps_host[k] [N][C][extents_host[2k]][extents_host[2k+1]], contiguous, k = 0 .. 3;
 *   y + k * C * H * W is the [N][C][H][W] slice of map k (batch stride y_batch_stride, 0 = 4 * C * H * W).
 *   Source indices follow F.interpolate's arithmetic for both values of align_corners (scale (in - 1) / (out - 1), or
 *   in / out with the half-pixel offset clamped at 0), in fp32, with the multiply-adds of the weighted sum fused as
 *   PyTorch's ROCm build fuses them: bit-exact against F.interpolate.
 * ---------------------------------------------------------------------------------- */
SNVC_API int snvc_dsgn_spp_upsample(const float *const *maps_host, const int64_t *extents_host, float *y, int64_t y_batch_stride,
                                    int64_t N, int64_t C, int64_t H, int64_t W, int align_corners, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_DSGN_H */
