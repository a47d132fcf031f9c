/*
 * snvc_dedup.h -- C ABI of the wedge deduplication of the fused sheared first layer in libsnvc_hip.so (gfx950).  Kept apart from
 * snvc_hip.h and snvc_fused.h, whose declaration sets and ABI numbers are pinned; this header versions itself through
 * snvc_dedup_abi_version().  Conventions are those of snvc_hip.h.
 *
 * The wedge.  The first layer's result v1 (snvc_fused.h) does not depend on the plane d where the plane is interior (class 1) and
 * the G index q * w - d - m0 + off is below 0: there G is the literal 0 of gi's zeroed pad.  The layer behind it is tiled
 * 4 (d) x 4 (h) x 32 (w).  Tile (d0, w0) is PURE when every voxel of its input image -- planes d0 - 1 .. d0 + 4, columns w0 - 1 ..
 * w0 + 32 -- is such a voxel:
 *   d0 >= 2  and  d0 + 3 <= D - 3;   w0 + 32 < W - 1  (the last column reads G');   q * (w0 + 32) - (d0 - 1) - m0 + off < 0.
 * The pure tiles of one (n, th, tw) are consecutive in d0, receive the same image and store the same bits on every depth row.  The
 * first is the REPRESENTATIVE, the others are DUPLICATES: they are not computed; one depth row of the representative is copied to
 * each of their rows by a second kernel of the same call on the same stream.
 */
#ifndef SNVC_DEDUP_H
#define SNVC_DEDUP_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_dedup_abi_version(void);

/* snvc_fused_first_conv3d_forward (same arguments, same results bit for bit, the overflow word included) that does not compute the
 * duplicate tiles but copies them.  The copy uses 16-byte accesses only: with a side head whose rows are not 16-byte aligned
 * (W % 4 != 0 or y_head itself), and for a shape without duplicates, the call IS snvc_fused_first_conv3d_forward: one launch. */
SNVC_API int snvc_dedup_fused_first_conv3d_forward(const snvc_conv3d_desc *desc, const void *packed_weight, const float *scale,
                                                   const float *bias, void *y_hi, void *y_lo, const float *head, float *y_head,
                                                   float head_mul, int *overflow, const float *gi, int64_t pitch, int64_t lp,
                                                   const float *p_il, const float *v_scale, const float *v_bias, int q, int m0, int off,
                                                   int off2, int v_flags, void *stream);

/* Host function, no device work: the duplicates of a layer of desc's Din / Win under (q, m0, off), by the rule the kernels use.
 * first_td[tw] / last_td[tw], tw < max_tw (host arrays): the representative's and the last duplicate's depth tile index of tile
 * column tw, or -1 / -1 where the column has no duplicate.  Returns the number of duplicate tiles of one (n, th) over ALL tile
 * columns, or -1 for arguments outside the above. */
SNVC_API int64_t snvc_dedup_fused_first_tiles(const snvc_conv3d_desc *desc, int q, int m0, int off, int64_t *first_td, int64_t *last_td,
                                              int max_tw);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_DEDUP_H */
