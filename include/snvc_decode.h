/*
 * snvc_decode.h -- C ABI of the device-side box read-out in libsnvc_hip.so (gfx950), the native side of
 * snvc_amd.decode.refine_boxes.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header
 * versions itself through snvc_decode_abi_version().
 *
 * Conventions are those of snvc_hip.h and snvc_roicrop.h: device pointers unless said otherwise, `stream` is a hipStream_t
 * passed as void* (NULL = default stream), the call is asynchronous on it, allocates nothing and never waits for the device,
 * int status return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.  Every
 * argument the host can see is checked before anything is launched.
 *
 * What is computed (the specification is in DESIGN.md, "Box read-out"; the arithmetic is that of
 * snvc_amd.decode.ncf_to_update_2d, reference vernier.py:665-738): per (instance, part) heat map the first-maximum argmax
 * with numpy's NaN rule, its value, the map's minimum and whether it holds a NaN; per instance the filter's keep flag, the
 * part targets in the camera frame, the moved box (`one_part`) and the box fitted to all nine parts by two closed-form 2D
 * Procrustes fits (`all_parts`), in float64.  No atomics, every output element is written exactly once: the same input
 * gives the same bits.
 */
#ifndef SNVC_DECODE_H
#define SNVC_DECODE_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_decode_abi_version(void);

/* Where a part's offset in the object frame comes from. */
enum { SNVC_DECODE_GRID = 0, SNVC_DECODE_COORDS_F32 = 1, SNVC_DECODE_COORDS_F64 = 2 };

/* Host memory. */
typedef struct snvc_decode_config {
    double x_range[2];   /* cfg.x_range: a coordinate c in 0 .. 1 maps to x_range[0] + c * (x_range[1] - x_range[0]) */
    double z_range[2];   /* cfg.z_range, likewise */
    float min_val;       /* Filter: an instance is kept when every value of its P maps lies in [min_val, max_val], */
    float max_val;       /*   compared in float32 as numpy compares a float32 array with a scalar; a NaN bound keeps nothing */
    int32_t source;      /* SNVC_DECODE_GRID: grid_or_coordinates is the BEV grid, float64 [M][3], row `index` is read and
                            its y dropped; SNVC_DECODE_COORDS_F32 / _F64: it is the coordinate head's output, [N][P][2],
                            widened to double before the range is applied */
    int32_t reserved;    /* 0 */
} snvc_decode_config;

/* Bytes of `workspace` for N instances of P parts (8-byte aligned); < 0 if N is negative, P is neither 1 nor 9 or N * P
 * does not fit a launch grid. */
SNVC_API int64_t snvc_decode_workspace_bytes(int64_t N, int64_t P);

/* ncf: float32 [N][P][M], M = nl * nw cells per map.  samples: float64 [N][7] = (h, w, l, x, y, z, ry), not written.
 * P is 1 or 9 (the fit has nine points).  M >= 1.  N = 0 returns SNVC_OK without a launch.
 * Outputs: conf float32 [N][P]; index int64 [N][P]; keep uint8 [N] (0 or 1); one_part float64 [N][7]; all_parts float64
 * [N][7], unused (may be NULL) with P = 1.  The row of a rejected instance in one_part and all_parts is its sample.
 * Two launches: the scan, one workgroup per map (argmax, minimum and NaN flag from one read of the map, the last two left
 * in `workspace`), and the fit, one thread per instance. */
SNVC_API int snvc_decode_boxes(const snvc_decode_config *cfg, const float *ncf, const double *samples,
                               const void *grid_or_coordinates, int64_t N, int64_t P, int64_t M, void *workspace, float *conf,
                               int64_t *index, uint8_t *keep, double *one_part, double *all_parts, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_DECODE_H */
