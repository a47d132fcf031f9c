/*
 * snvc_loss.h -- C ABI of the training losses in libsnvc_hip.so (gfx950), the native side of snvc_amd.models.loss3d.
 * Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header versions itself through
 * snvc_loss_abi_version().
 *
 * Conventions are those of snvc_hip.h: device pointers, `stream` is a hipStream_t passed as void* (NULL = default stream),
 * every call is asynchronous on it, allocates nothing and never waits for the device, int status return (snvc_status),
 * snvc_last_error_string() for the text of the last failure on the calling thread.  Every argument is checked on the host
 * before anything is launched.  Tensors are dense float32 unless said otherwise.
 *
 * Every loss is one streaming pass that leaves one fp32 partial per workgroup (per-lane fp32 sums, a wave reduction, the
 * waves of a workgroup added in wave order), followed by a one-workgroup launch that adds the partials in float64 in a fixed
 * order, writes the loss (float32) and leaves the normalisers the backward pass needs in `fin` (float64).  No
 * floating-point atomics: the same input gives the same bits.  The backward pass is one launch that reads `fin` and the
 * upstream gradient scalar `gout` on the device and writes every gradient element once (exactly 0 where the loss's mask
 * excludes the element).
 */
#ifndef SNVC_LOSS_H
#define SNVC_LOSS_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_loss_abi_version(void);

/* Elementwise losses over a [rows][cols] view of the prediction `a`.  "flat" kinds are called with rows = 1. */
enum snvc_loss_kind {
    /* mean over all elements of (a w - b w)^2, w = roww[row] (NULL: 1).                                     VoxelMSELoss */
    SNVC_LOSS_MSE_ROWS = 0,
    /* row r belongs to part r % group; per part 0.5 (mean over b > 0 of (a - b)^2 + mean over b <= 0 of the same), mean
       over parts.  A part without a positive target sets SNVC_LOSS_FLAG_NO_POSITIVE in *flag.            VoxelMSELossWeighted */
    SNVC_LOSS_MSE_POSNEG = 1,
    /* flat.  b in {-1, 0, 1}; mean over b != -1 of  -[b == 1] p0 (1 - a)^p1 log(a + 1e-7) - [b == 0] (1 - p0) a^p1
       log((1 - a) + 1e-7); 0 if nothing is counted.                                                        OccupancyLoss */
    SNVC_LOSS_OCCUPANCY = 2,
    /* c [rows / group][cols] is shared by the `group` rows of a sample; mean of |a - b| over c == 1; 0 if none. OffsetLoss */
    SNVC_LOSS_OFFSET = 3,
    /* flat.  smooth-L1 (beta p0) mean over the mask: c (uint8, same shape) != 0, or with c = NULL b != -1 && b < 60.
       Empty mask: 0, or NaN with SNVC_LOSS_EMPTY_IS_NAN.                                      DepthLoss, calc_disp_loss */
    SNVC_LOSS_SMOOTH_L1_MASKED = 4,
    /* flat.  p = sigmoid(a); sum of the OCCUPANCY term over b in {0, 1} times c (same shape, NULL: 1); b is float32, or
       int32 / int64 / uint8 with SNVC_LOSS_TARGET_*.  A b outside {0, 1} sets SNVC_LOSS_FLAG_BAD_TARGET.  sigmoid_focal_loss_multi_target */
    SNVC_LOSS_SIGMOID_FOCAL = 5,
    /* flat, cols = M * group.  l = |a - b| < p0 ? 0.5 (a - b)^2 / p0 : |a - b| - 0.5 p0;
       sum_m(mean over the `group` columns of l * roww[m]) / sum_m roww[m].                                  smooth_l1_loss */
    SNVC_LOSS_SMOOTH_L1_ROWS = 6,
    SNVC_LOSS_KINDS = 7
};

enum snvc_loss_flags {
    SNVC_LOSS_EMPTY_IS_NAN = 1,
    SNVC_LOSS_TARGET_INT32 = 2,     /* SIGMOID_FOCAL: b is int32, int64 or uint8 (bool) instead of float32; at most one of the three */
    SNVC_LOSS_TARGET_INT64 = 4,
    SNVC_LOSS_TARGET_UINT8 = 8
};

/* Bits a loss ORs into *flag (int32 on the device) for the caller to look at later. */
#define SNVC_LOSS_FLAG_NO_POSITIVE 1
#define SNVC_LOSS_FLAG_BAD_TARGET 2

/* rows of SNVC_LOSS_MSE_ROWS (with roww), MSE_POSNEG and OFFSET map to the launch grid's second dimension */
#define SNVC_LOSS_MAX_ROWS 65535

typedef struct snvc_loss_desc {
    int32_t kind;           /* snvc_loss_kind */
    int32_t flags;          /* snvc_loss_flags */
    int64_t rows, cols;
    int64_t group;          /* see the kind; 1 where unused */
    float p0, p1;           /* see the kind */
    const float *a;         /* prediction [rows][cols] */
    const void *b;          /* target, same shape */
    const void *c;          /* see the kind; may be NULL where optional */
    const float *roww;      /* see the kind; may be NULL where optional */
    float *partials;        /* workspace of snvc_loss_partials_count() floats; forward writes, finalisation reads */
    double *fin;            /* 2 doubles (MSE_POSNEG: 2 * group): normalisers, written by forward, read by backward */
    float *loss;            /* one float, written by forward */
    int32_t *flag;          /* one int32, ORed into by forward */
    const float *gout;      /* backward: the upstream gradient of *loss (one float on the device) */
    float *ga;              /* backward: gradient for a, same shape, every element written */
} snvc_loss_desc;

/* Floats of desc->partials for desc's kind / rows / cols; < 0 if the descriptor is invalid. */
SNVC_API int64_t snvc_loss_partials_count(const snvc_loss_desc *desc);
/* Two launches (the streaming pass and the finalisation).  Reads a, b, c, roww once. */
SNVC_API int snvc_loss_forward(const snvc_loss_desc *desc, void *stream);
/* One launch.  Reads a, b, c, roww, fin, gout; writes ga. */
SNVC_API int snvc_loss_backward(const snvc_loss_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------
 * W_loss (p = 1): prob, off [B][D][HW] are read in place (no permuted copy); target [B][HW]; mask [B][HW] uint8;
 * levels [D].  Per masked pixel sum_d prob |levels[d] + off - target|; *loss = their mean (NaN for an empty mask, as the
 * mean of nothing is).  pixel_loss (may be NULL) receives the per-pixel sums, 0 outside the mask.
 * partials: snvc_loss_wdist_partials_count() floats; fin: 2 doubles.
 * Backward: gpix (may be NULL) is a per-pixel upstream gradient [B][HW] used instead of gout[0] / count; gprob and goff
 * (either may be NULL) are written in full.
 * ---------------------------------------------------------------------------------- */
SNVC_API int64_t snvc_loss_wdist_partials_count(int64_t B, int64_t D, int64_t HW, int per_pixel);
SNVC_API int snvc_loss_wdist_forward(const float *prob, const float *off, const float *target, const uint8_t *mask,
                                     const float *levels, int64_t B, int64_t D, int64_t HW, float *pixel_loss, float *partials,
                                     double *fin, float *loss, void *stream);
SNVC_API int snvc_loss_wdist_backward(const float *prob, const float *off, const float *target, const uint8_t *mask,
                                      const float *levels, int64_t B, int64_t D, int64_t HW, const double *fin, const float *gout,
                                      const float *gpix, float *gprob, float *goff, void *stream);

/* ------------------------------------------------------------------------------------
 * depth_regression_loss: smooth-L1 (beta 1) mean over gt != -1 && gt < 60 of  sum_d softmax_d(cost)[d] levels[d] - gt.
 * cost [B][D][HW], levels [D], gt [B][HW].  The softmax over D is taken in registers (a stable two-step form per D slice,
 * merged across the slices of a workgroup); neither the probabilities nor the depth map are written.  0 for an empty mask.
 * partials: snvc_loss_depth_regression_partials_count() floats; fin: 2 doubles.  Backward writes gcost in full.
 * ---------------------------------------------------------------------------------- */
SNVC_API int64_t snvc_loss_depth_regression_partials_count(int64_t B, int64_t HW);
SNVC_API int snvc_loss_depth_regression_forward(const float *cost, const float *levels, const float *gt, int64_t B, int64_t D,
                                                int64_t HW, float *partials, double *fin, float *loss, void *stream);
SNVC_API int snvc_loss_depth_regression_backward(const float *cost, const float *levels, const float *gt, int64_t B, int64_t D,
                                                 int64_t HW, const double *fin, const float *gout, float *gcost, void *stream);

/* Adjoint of snvc_disparity_regression with respect to x: gx[n][d][i] = gy[n][i] * depth[d]. */
SNVC_API int snvc_loss_disparity_regression_backward(const float *gy, const float *depth, float *gx, int64_t N, int64_t D,
                                                     int64_t HW, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_LOSS_H */
