/*
 * snvc_fc.h -- C ABI of the fully-connected box head in libsnvc_hip.so (gfx950), the native side of
 * snvc_amd.models.FCmodel.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header
 * versions itself through snvc_fc_abi_version().
 *
 * Conventions are those of snvc_hip.h and snvc_decode.h: device pointers unless said otherwise, `stream` is a hipStream_t
 * passed as void* (NULL = default stream), every call is asynchronous on it, allocates nothing and never waits for the
 * device, int status return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.
 * Every argument the host can see is checked before anything is launched.  All tensors are dense row-major float32 unless
 * said otherwise.  Every product is an exact float32 product accumulated in float32 (v_mfma_f32_16x16x4_f32); there are no
 * atomics and every sum has a fixed order, so the same input gives the same bits.
 *
 * The network ("FC box head"): L = 1 + 2 * num_blocks layers of Linear + BatchNorm1d + activation (+ dropout),
 * the layers 1, 2 / 3, 4 / ... paired into residual blocks (the block's input is added to its second layer's result), then
 * one plain Linear to output_size.
 */
#ifndef SNVC_FC_H
#define SNVC_FC_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_fc_abi_version(void);

/* Largest input_size, num_neurons and output_size the kernels take; num_neurons must be a multiple of 16. */
enum { SNVC_FC_MAX_WIDTH = 1024 };

/* Floats of the packed eval buffer, or < 0 if a size is outside the kernels' range.  Layout, layer after layer in call
 * order: the weights as slabs of 16 output neurons, slab s holding [Kp][16] floats (element [k][j] = weight of neuron
 * 16 s + j for input k, times the neuron's folded BatchNorm scale; zero for k >= K and for neurons past the layer's
 * width), then one shift per neuron padded likewise.  Kp is K rounded up to a multiple of 4, the neuron count is
 * rounded up to a multiple of 16. */
SNVC_API int64_t snvc_fc_packed_floats(int64_t input_size, int64_t num_neurons, int64_t num_blocks, int64_t output_size);

/* Eval forward of the whole network in one launch: one workgroup per 16 rows, activations in LDS from input to output.
 * x [N][input_size]; packed as above; out [N][output_size], or [N][num_neurons] with representation != 0 (the launch
 * stops before the last Linear).  leaky != 0: LeakyReLU with slope 0.01, else ReLU.  N = 0 returns SNVC_OK unlaunched. */
SNVC_API int snvc_fc_eval_forward(const float *x, const float *packed, float *out, int64_t N, int64_t input_size,
                                  int64_t num_neurons, int64_t num_blocks, int64_t output_size, int leaky, int representation,
                                  void *stream);

/* Training forward of one layer, one workgroup per 16 neurons walking all N rows.  x [N][K], weight [M][K], bias [M].
 * gamma != NULL (M a multiple of 16, N >= 2): z = x W^T + b; batch mean and biased variance per neuron; xhat = (z - mean) *
 * istd with istd = 1 / sqrt(var + eps); y = act(gamma * xhat + beta); with mask (uint8 [N][M], 0 = dropped) y is y *
 * keep_scale where kept and 0 where dropped; with residual [N][M] it is added last.  Written: xhat [N][M], mean [M], istd
 * [M], out [N][M]; running_mean and running_var move by `momentum` (the unbiased variance for the running value) and
 * *num_batches_tracked (int64, may be NULL) grows by one.
 * gamma == NULL: the plain Linear, out = x W^T + b; every other pointer but x, weight, bias and out is ignored. */
SNVC_API int snvc_fc_train_layer_forward(const float *x, const float *weight, const float *bias, const float *gamma,
                                         const float *beta, float *running_mean, float *running_var,
                                         int64_t *num_batches_tracked, const uint8_t *mask, const float *residual, float *xhat,
                                         float *mean, float *istd, float *out, int64_t N, int64_t K, int64_t M, float eps,
                                         float momentum, float keep_scale, int leaky, void *stream);

/* Training backward of one layer, first launch (slab-owned as the forward): dy [N][M] is the gradient of the layer's
 * output.  gamma != NULL: the dropout, activation and BatchNorm backward give dz [N][M], dgamma [M], dbeta [M]; then
 * dweight [M][K] = dz^T x and dbias [M] = the column sums of dz.  gamma == NULL: dz is not written, dy takes its place. */
SNVC_API int snvc_fc_train_layer_backward_params(const float *dy, const float *x, const float *xhat, const float *gamma,
                                                 const float *beta, const float *istd, const uint8_t *mask, float *dz,
                                                 float *dgamma, float *dbeta, float *dweight, float *dbias, int64_t N,
                                                 int64_t K, int64_t M, float keep_scale, int leaky, void *stream);

/* Training backward of one layer, second launch (one workgroup per 16 rows): dx [N][K] = dz W (+ skip [N][K] if not
 * NULL: the gradient that reaches a residual block's input past its two layers).  dx may be skip itself: each element is read,
 * then written, by one lane. */
SNVC_API int snvc_fc_train_layer_backward_input(const float *dz, const float *weight, const float *skip, float *dx, int64_t N,
                                                int64_t K, int64_t M, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_FC_H */
