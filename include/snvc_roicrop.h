/*
 * snvc_roicrop.h -- C ABI of the stereo RoI cropper in libsnvc_hip.so (gfx950), the native side of
 * snvc_amd.geometry.RoICropper.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header
 * versions itself through snvc_roicrop_abi_version().
 *
 * Conventions are those of snvc_hip.h and snvc_targets.h: device pointers unless said otherwise, `stream` is a hipStream_t
 * passed as void* (NULL = default stream), the call is asynchronous on it, allocates nothing and never waits for the device,
 * int status return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.  Every
 * argument the host can see is checked before anything is launched; what lives in device memory (the image descriptors, the
 * frame indices) is checked by the kernels: a frame index outside 0 .. F-1 or a descriptor with a NULL pointer, a
 * non-positive size, a side above SNVC_ROICROP_MAX_SIDE or a row stride below 3 * width reads nothing and gives an all-zero
 * crop (before normalisation).
 *
 * What is computed (the specification is in DESIGN.md, "RoI crops"): for sample n = (h, w, l, x, y, z, ry) and each camera,
 * the nine projected points of the RoI box (the sample with its size replaced by grid_range), the crop centre and size
 * around them (enlarged by 1.1, grown to aspect_ratio), the 2x3 affine `trans` onto the out_w x out_h patch, the bilinear
 * warp of the uint8 image with a zero border, and ToTensor + Normalize.  No atomics, every output element is written exactly
 * once: the same input gives the same bits.
 */
#ifndef SNVC_ROICROP_H
#define SNVC_ROICROP_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_roicrop_abi_version(void);

#define SNVC_ROICROP_MAX_SIDE 32767     /* image and patch sides: the fixed-point coordinates keep 5 fractional bits */
#define SNVC_ROICROP_MAX_SAMPLES 32767  /* (sample, side) maps to the launch grid's second dimension */

/* One interleaved uint8 image [height][width][3] in device memory; rows start row_stride bytes apart.  No alignment is
 * assumed for `data` or `row_stride`. */
typedef struct snvc_roicrop_image {
    const uint8_t *data;
    int32_t height, width;
    int64_t row_stride;      /* bytes, >= 3 * width */
} snvc_roicrop_image;

enum { SNVC_ROICROP_FIXED5 = 0, SNVC_ROICROP_EXACT = 1 };

/* Host memory. */
typedef struct snvc_roicrop_config {
    int32_t out_w, out_h;    /* resolution = (Wr, Hr): width first, 1 .. SNVC_ROICROP_MAX_SIDE */
    int32_t interpolation;   /* SNVC_ROICROP_FIXED5: source coordinates in 1/32 px, integer blend (the default);
                                SNVC_ROICROP_EXACT: float64 source coordinates, float32 blend, round to nearest */
    int32_t swap_rb;         /* 1: the images are BGR, channels 0 and 2 are swapped on the read */
    int32_t raw;             /* 0: float32 rois, normalised through `norm_table`; 1: uint8 rois, the warp's own result */
    int32_t reserved;        /* 0 */
    double aspect_ratio;     /* height / width the crop is grown to, > 0 */
    double grid_range[3];    /* df_params['range']: the (h, w, l) of the RoI box */
} snvc_roicrop_config;

/* Bytes of `workspace` for N samples (8-byte aligned); < 0 if N is negative or above SNVC_ROICROP_MAX_SAMPLES. */
SNVC_API int64_t snvc_roicrop_workspace_bytes(int64_t N);

/* left_images / right_images: F descriptors each.  frame: int32 [N], the descriptor (and projection) of sample n, or NULL:
 * every sample uses descriptor 0.  samples: float64 [N][7].  P_left / P_right: float64 [F][12], row-major [3][4].
 * norm_table: float32 [3][256], entry [c][p] = (p / 255 - mean_c) / std_c as the caller's float32 arithmetic gives it;
 * unused (may be NULL) with raw = 1.
 * Outputs: left_rois / right_rois: float32 (raw = 0) or uint8 (raw = 1) [N][3][out_h][out_w]; trans_l / trans_r: float64
 * [N][2][3]; kpts_l / kpts_r: float64 [N][9][2]; local_l / local_r: float32 [N][9][2] = float32(trans . [kpts; 1]).
 * Two launches: a prologue of one thread per (sample, side), which writes trans, kpts, local and leaves the six
 * coefficients of the inverse transform in `workspace`, and the warp, one thread per output pixel. */
SNVC_API int snvc_roicrop(const snvc_roicrop_config *cfg, const snvc_roicrop_image *left_images,
                          const snvc_roicrop_image *right_images, int64_t F, const int32_t *frame, const double *samples,
                          const double *P_left, const double *P_right, int64_t N, const float *norm_table, void *workspace,
                          void *left_rois, void *right_rois, double *trans_l, double *trans_r, double *kpts_l, double *kpts_r,
                          float *local_l, float *local_r, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_ROICROP_H */
