/*
 * snvc_hrnet.h -- C ABI of the HRNet multi-resolution fusion in libsnvc_hip.so (gfx950), the native side of
 * snvc_amd.models.hrnet.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header
 * versions itself through snvc_hrnet_abi_version().
 *
 * Conventions are those of snvc_hip.h: device pointers unless the name ends in _host, `stream` is a hipStream_t
 * passed as void* (NULL = default stream), every call is asynchronous on it and allocates nothing, int status
 * return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.  Every
 * argument is checked on the host before anything is launched.
 *
 * Tensors are contiguous NCHW float32.  A term of factor f is [N][C][H/f][W/f] and stands for its nearest-neighbour
 * upsampling by f to [N][C][H][W] (nn.Upsample(scale_factor=f, mode='nearest'): out[y][x] = t[y/f][x/f]).
 */
#ifndef SNVC_HRNET_H
#define SNVC_HRNET_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_hrnet_abi_version(void);

#define SNVC_HRNET_MAX_TERMS 4

/* ------------------------------------------------------------------------------------
 * Fusion sum of one output branch of an HRNet module
 * replaces: HighResolutionModule.forward's fusion loop (hrnet.py:235-252: y = y + x[j] / y + fuse_layers[i][j](x[j]),
 *           then relu(y)) together with the nn.Upsample(scale_factor=2**(j-i), mode='nearest') that ends each
 *           up path (hrnet.py:204).
 *   out = act(t0 + up(t1) + up(t2) + up(t3)), summed left to right in fp32 (no fused multiply-add), a NULL term
 *   skipped; act(v) = v > 0 ? v : 0 when relu != 0, the identity otherwise.
 *   terms_host[k]: device pointer of term k (terms_host[0] must not be NULL); factors_host[k] in {1, 2, 4, 8};
 *   extents_host[2k], extents_host[2k+1]: that term's own (height, width), which must equal (H / f_k, W / f_k) with
 *   no remainder (an HRNet input that is not a multiple of 32 lands here: SNVC_ERR_INVALID_ARGUMENT, nothing cropped).
 *   out [N][C][H][W] may alias term 0 when factors_host[0] == 1 (in place); it must not alias another term.
 * ---------------------------------------------------------------------------------- */
SNVC_API int snvc_hrnet_fuse_forward(const void *const *terms_host, const int32_t *factors_host, const int64_t *extents_host,
                                     float *out, int64_t N, int64_t C, int64_t H, int64_t W, int relu, void *stream);

/* ------------------------------------------------------------------------------------
 * Backward of snvc_hrnet_fuse_forward
 * replaces: autograd's backward of the same lines (threshold_backward of the ReLU, then upsample_nearest2d_backward
 *           of each up path and the identity of every factor-1 term).
 *   g = relu ? (out > 0 ? gy : 0) : gy over [N][C][H][W]; `out` may be NULL when relu == 0.
 *   grad1 [N][C][H][W] receives g (the gradient of every factor-1 term) unless NULL;
 *   grad2 / grad4 / grad8 [N][C][H/f][W/f] receive the f x f block sums of g unless NULL, each block summed row by
 *   row top to bottom, every row left to right: a fixed order, no atomics, bitwise repeatable.
 *   gy and out are read once.  H and W must be multiples of every factor whose buffer is given.
 * ---------------------------------------------------------------------------------- */
SNVC_API int snvc_hrnet_fuse_backward(const float *gy, const float *out, float *grad1, float *grad2, float *grad4, float *grad8,
                                      int64_t N, int64_t C, int64_t H, int64_t W, int relu, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_HRNET_H */
