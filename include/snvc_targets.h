/*
 * snvc_targets.h -- C ABI of the local (Vernier) model's training targets in libsnvc_hip.so (gfx950), the native side of
 * snvc_amd.geometry.TargetGenerator.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this header
 * versions itself through snvc_targets_abi_version().
 *
 * Conventions are those of snvc_hip.h: device pointers unless said otherwise, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every call is asynchronous on it, allocates nothing and never waits for the device, int status
 * return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.  Every argument is
 * checked on the host before anything is launched.
 *
 * The calls take boxes, not planes: `samples` and `labels` are [N][7] float64 rows (h, w, l, x, y, z, ry), the proposal and
 * the ground-truth box that belongs to it.  Every decision (inside / outside a box, the voxel a position falls in) is taken
 * in float64, as the reference takes it with numpy on the host.  Both calls first run a one-thread-per-sample prologue that
 * leaves the sample's twelve box planes, its part indices and its heat-map windows in `workspace`
 * (snvc_targets_workspace_bytes(N) bytes, 8-byte aligned); the two calls may share one workspace on one stream.
 * No atomics: every thread that hits an element stores the same value, so the same input gives the same bits.
 */
#ifndef SNVC_TARGETS_H
#define SNVC_TARGETS_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_targets_abi_version(void);

#define SNVC_TARGETS_MAX_PARTS 9       /* centre + eight corners (_get_cam_cord) */
#define SNVC_TARGETS_MAX_SAMPLES 7000  /* N * num_parts maps to the launch grid's second dimension */

/* What refinementDataset reads from its cfg / df_params (KITTIRefinement_dataset.py:88-95).  Host memory. */
typedef struct snvc_targets_grid {
    int32_t nh, nw, nl;     /* grid_resolution */
    int32_t num_parts;      /* 1 .. SNVC_TARGETS_MAX_PARTS */
    int32_t sigma;          /* >= 1; the heat-map window is +-3 sigma cells */
    int32_t grid_type;      /* 2: maps [nl][nw] indexed [z][x]; 3: volumes [nh][nw][nl] indexed [y][x][z] */
    double spacing[3];      /* (dy, dx, dz) */
    double grid_range[3];   /* df_params['range']: the (h, w, l) of the RoI box */
    double ranges[6];       /* x_range, y_range, z_range: (min, max) each, the linspace ends of _init_3d_grid */
} snvc_targets_grid;

/* Bytes of `workspace` for N samples; < 0 if N is negative or above SNVC_TARGETS_MAX_SAMPLES. */
SNVC_API int64_t snvc_targets_workspace_bytes(int64_t N);

/* The per-part Gaussian heat maps and the part positions in the sample's frame: replaces
 * refinementDataset._construct_neural_confidence_field (KITTIRefinement_dataset.py:722-777) with _get_cam_cord (:523-553),
 * _get_basis (:704-720), _draw_heatmaps_3d (:623-664) and _draw_heatmaps_2d (:666-702), and the float32 casts of
 * _generate_displacement_field (:900-902).
 * fields: float32 [N][num_parts][nl][nw] (grid_type 2) or [N][num_parts][nh][nw][nl] (grid_type 3); every element is
 * written exactly once, as 0 or as a window value, so the buffer needs no clearing.  corners_local: float32 [N][num_parts][3].
 * Two launches: the prologue and one streaming pass. */
SNVC_API int snvc_targets_fields(const snvc_targets_grid *grid, const double *samples, const double *labels, int64_t N,
                                 void *workspace, float *fields, float *corners_local, void *stream);

/* The foreground (1) / background (0) / undefined (-1) grid: replaces refinementDataset._get_point_cloud
 * (KITTIRefinement_dataset.py:779-826) with construct_mesh_cuboid and Mesh.in_mesh (snvc/utils/bounding_box.py:286-297,
 * 360-390), the grid points of _to_cam (:828-846) that it is handed, and, with velo_to_rect, Calibration.project_velo_to_rect
 * (snvc/dataset/kitti_util.py:252-277) of _generate_displacement_field (:885-887).
 * points: [num_points][3], float32 (points_f64 = 0) or float64.  Sample n tests the rows slices[2n] .. slices[2n] +
 * slices[2n+1] - 1 (int64 pairs (first row, count) on the device, count <= max_points; rows at or past num_points are
 * left out), or with slices = NULL the rows 0 .. max_points - 1.
 * velo_to_rect: NULL, or 21 float64 on the device, V2C [3][4] then R0 [3][3], applied to every point before it is tested.
 * occupancy: float32 [N][nh][nw][nl], every element written.  in_roi / in_fg: NULL (both), or uint8 [N][max_points]:
 * 1 where the sample's k-th point is inside the RoI box / inside the RoI box and the ground-truth box, 0 elsewhere.
 * Three launches, queued by this one call: the prologue, the pass over the voxels (-1 or 0) and the pass over the points
 * (1 where the voxel pass left a non-zero value). */
SNVC_API int snvc_targets_occupancy(const snvc_targets_grid *grid, const double *samples, const double *labels, int64_t N,
                                    const void *points, int points_f64, int64_t num_points, const int64_t *slices,
                                    int64_t max_points, const double *velo_to_rect, void *workspace, float *occupancy,
                                    uint8_t *in_roi, uint8_t *in_fg, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_TARGETS_H */
