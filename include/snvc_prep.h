/*
 * snvc_prep.h -- C ABI of the POOLED 2D prep of the fused sheared first layer in libsnvc_hip.so (gfx950): what
 * snvc_fused_sheared_prep_x3 (the right feature's scale, Rq -> G, Rq' -> G') and snvc_fused_planes_from_f32 (the left feature's
 * scale, its split pair, the 3x3 depth-class planes) queue as eight launches, queued as three:
 *   stage A  split_scale_pair_kernel   both features' scales, one grid of two workgroup ranges
 *   stage B  split_producers_kernel    the split pairs Rq, Rq' and the left feature's, one 1D grid of three block ranges
 *   stage C  conv2d_x3q_pool_kernel    G, G' and the left planes, one grid of three job ranges (gridDim.z = N)
 * Every range runs the body of the kernel it replaces on the same operands with its own local block index and block count, so
 * every output holds the bits the two calls leave.  No cooperative launch, no device-wide wait: a stage is ordered behind the one
 * before it by the stream.  Kept apart from snvc_hip.h and snvc_fused.h, whose declaration sets and ABI numbers are pinned; this
 * header versions itself through snvc_prep_abi_version().
 *
 * Conventions are those of snvc_hip.h: device pointers unless said otherwise, `stream` is a hipStream_t passed as void*
 * (NULL = default stream), every call is asynchronous on it, allocates nothing and never waits for the device, int status
 * return (snvc_status), snvc_last_error_string() for the text of the last failure on the calling thread.
 */
#ifndef SNVC_PREP_H
#define SNVC_PREP_H

#include <stdint.h>

#include "snvc_fused.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_prep_abi_version(void);

/* snvc_prep_pooled_x3's `pool` bits: a stage whose bit is clear is queued as the single launches it replaces (same results).
 * A measurement knob -- the stages were timed one by one with it (profiles/prep_pool/); the model always passes both bits. */
#define SNVC_PREP_POOL_AB 1 /* stages A and B */
#define SNVC_PREP_POOL_C 2  /* stage C */

/* The three grids of a shape, host memory.  Sub-problems in range order: stage A (right, left); stages B and C (G's, G''s, the left
 * feature's).  A range's blocks are [sum of the counts before it, + its own count). */
typedef struct snvc_prep_pool_plan_t {
    int64_t a_blocks[2];  /* stage A: workgroups that fold the right / the left feature */
    int64_t b_blocks[3];  /* stage B: blocks of 256 threads that write Rq / Rq' / the left pair */
    int64_t b_items[3];   /* stage B: threads with work: N * C/8 * H * WU (WU2); N * C/8 * H * W */
    int64_t b_row_blocks; /* stage B, left pair: blocks per (sample, channel group), block = (n * C/8 + g) * b_row_blocks + bx */
    int64_t c_jobs[3];    /* stage C: (tile, 32-channel block) jobs PER SAMPLE of G / G' / the left planes, on gridDim.x */
    int64_t c_samples;    /* stage C: gridDim.z */
} snvc_prep_pool_plan_t;

/* Host function, no device: the plan of snvc_prep_pooled_x3 for right / left features [N][C][H][W] and sheared widths WU / WU2
 * -- the one function the launcher itself uses for its three grids.  SNVC_OK, or the launcher's own refusal of the shape. */
SNVC_API int snvc_prep_pool_plan(int64_t N, int64_t C, int64_t H, int64_t W, int64_t WU, int64_t WU2, snvc_prep_pool_plan_t *plan);

/* Host function: the plane of the class-minor plain result [3 * C] that row `row` of a class-major layer is written to (left_rows 1;
 * the function the epilogue uses): (row % C) * 3 + row / C, or -1 outside [0, 3 * C). */
SNVC_API int64_t snvc_prep_plain_plane(int64_t row, int64_t C);

/* Host function: the sub-problem and the local block index of block `block` of stage 0 | 1 | 2 (A | B | C) -- the function the
 * kernels use.  Returns the sub-problem (0, 1, 2) with *local set, or -1 for a stage or a block outside the plan. */
SNVC_API int snvc_prep_pool_locate(const snvc_prep_pool_plan_t *plan, int stage, int64_t block, int64_t *local);

/* snvc_fused_sheared_prep_x3(right, ..., mul_right, g, gcol, gi, pitch, lp) and snvc_fused_planes_from_f32(left, N, C, H, W,
 * packed_left, cout_left, out_mul_left, planes, p_il, left_split, ., mul_left) in one call: the same results in g, gcol, gi, planes,
 * p_il, the three split workspaces and the two scales.  scratch16: FOUR zeroed 32-bit words, left zero (words 0, 1: the right
 * feature's maximum and arrival counter, words 2, 3: the left's), one per stream.  pool: SNVC_PREP_POOL_* bits.
 * left_rows 0: packed_left's rows are class-minor (row = co * 3 + cls, what snvc_fused_planes_from_f32 takes).  left_rows 1: they are
 * class-major (row = cls * C + co): the lane's eight channels are one channel group of p_il, written as two 16-byte stores, and row r
 * of the plain result goes to plane snvc_prep_plain_plane(r, C) -- `planes` and `p_il` hold the same bytes either way. */
SNVC_API int snvc_prep_pooled_x3(const float *right, int64_t N, int64_t C, int64_t H, int64_t W, int q, int64_t WU, int off, int64_t WU2,
                                 int off2, const void *packed_g, const void *packed_col, int64_t Cout3, float out_mul_g, float out_mul_col,
                                 void *rq_split, void *rq2_split, float *mul_right, float *g, float *gcol, float *gi, int64_t pitch,
                                 int64_t lp, const float *left, const void *packed_left, int64_t cout_left, float out_mul_left, float *planes,
                                 float *p_il, void *left_split, float *mul_left, void *scratch16, int left_rows, int pool, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_PREP_H */
