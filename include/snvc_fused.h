/*
 * snvc_fused.h -- C ABI of the fused sheared first layer in libsnvc_hip.so (gfx950): the split-mode 3x3x3 layer behind the
 * sheared first convolution (conv3d_x3q_kernel) produces its own input image from the first layer's 2D operands instead of
 * reading the first layer's result back from memory.  Kept apart from snvc_hip.h, whose declaration set and ABI number are
 * pinned; this header versions itself through snvc_fused_abi_version().
 *
 * Conventions are those of snvc_hip.h: device pointers unless said otherwise, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every call is asynchronous on it, allocates nothing and never waits for the device, int status
 * return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.
 *
 * The channel-interleaved ("il") layout: float32 [N][classes][ceil(C / 8)][H][pitch][8] -- the 8 channels of a channel group
 * of one (class, row, column) are 32 adjacent bytes, column x of the tensor sits at pitch position lp + x.  The positions
 * outside [lp, lp + width) are never written by this library: the caller zeroes the buffer once, and an index that leaves
 * the tensor's row reads 0 there (what the expand pass substitutes for an out-of-range G index).
 *   mode 0 ("class-major"): output channel oc = cls * C + co  (G and G' of snvc_sheared_prep_x3)
 *   mode 1 ("class-minor"): output channel oc = co * 3 + cls  (the left half's depth-class planes)
 */
#ifndef SNVC_FUSED_H
#define SNVC_FUSED_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_fused_abi_version(void);

/* Host function: float index of output channel `oc` (of 3 * C), row h, column x inside ONE sample of an il buffer with
 * `classes` classes whose first class is `cls0` (G': 3 of 6), or -1 for arguments outside the layout.  The kernels use the
 * same function. */
SNVC_API int64_t snvc_fused_il_index(int mode, int64_t oc, int64_t C, int64_t H, int64_t pitch, int64_t lp, int64_t cls0,
                                     int64_t h, int64_t x);

/* snvc_sheared_prep_x3 (same arguments, same float32 results g / gcol) that ALSO writes G as classes 0..2 and G' as classes
 * 3..5 of `gi`, an il buffer [N][6][C / 8][H][pitch][8] with left pad lp (both sections share pitch and lp).  No extra
 * launch: an output option of the two 3x7 layers' epilogues.  Cout3 == 3 * C. */
SNVC_API int snvc_fused_sheared_prep_x3(const float *right, int64_t N, int64_t C, int64_t H, int64_t W, int q, int64_t WU, int off,
                                        int64_t WU2, int off2, const void *packed_g, const void *packed_col, int64_t Cout3,
                                        float out_mul_g, float out_mul_col, void *rq_split, void *rq2_split, void *scratch8,
                                        float *mul_dev, float *g, float *gcol, float *gi, int64_t pitch, int64_t lp, void *stream);

/* snvc_f16x3_conv2d_from_f32 with ONE 3x3 layer of 3 * C output channels (class-minor) whose result is also written as the
 * il buffer p_il [N][3][C / 8][H][W][8] (pitch W, no pad). */
SNVC_API int snvc_fused_planes_from_f32(const float *x, int64_t N, int64_t C, int64_t H, int64_t W, const void *packed, int64_t cout,
                                        float out_mul, float *y, float *p_il, void *ws_split, void *scratch8, float *mul_dev,
                                        void *stream);

/* snvc_f16x3_conv3d_forward for a 3x3x3 / stride-1 / pad-1 layer on the 16x16x32 kernel form (desc->algo SNVC_ALGO_X3_Q16)
 * with a split C8 output (+ side head), whose INPUT is the sheared first layer's result, formed inside the launch:
 *   v1[c][d][h][w] = med3(fma(G[cls][c][h][q * w - d - m0 + off] + P[cls][c][h][w], v_scale[c], v_bias[c]), lo, 65504)
 * (the last column w == W - 1 reads G' at q * (W - 1) - d - m0 + off2; cls = 0 | 1 | 2 for d == 0 | interior | D - 1; lo = 0
 * with SNVC_EPI_RELU in v_flags, else -65504), split as hi = (half)v1, lo = (half)(v1 - hi): operation for operation the
 * values snvc_sheared_expand_split stores.  desc gives the layer (Cin = the first layer's channels, D / H / W of v1);
 * gi / p_il as above.  *overflow is raised when a stored |v1| or a stored output reaches 65504. */
SNVC_API int snvc_fused_first_conv3d_forward(const snvc_conv3d_desc *desc, const void *packed_weight, const float *scale,
                                             const float *bias, void *y_hi, void *y_lo, const float *head, float *y_head,
                                             float head_mul, int *overflow, const float *gi, int64_t pitch, int64_t lp,
                                             const float *p_il, const float *v_scale, const float *v_bias, int q, int m0, int off,
                                             int off2, int v_flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_FUSED_H */
