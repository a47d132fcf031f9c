/*
 * snvc_alias.h -- C ABI of the aliased wedge duplicates in libsnvc_hip.so (gfx950).  Kept apart from snvc_hip.h, snvc_fused.h and
 * snvc_dedup.h, whose declaration sets and ABI numbers are pinned; this header versions itself through snvc_alias_abi_version().
 * Conventions are those of snvc_hip.h.
 *
 * snvc_dedup.h: the fused first layer's duplicate tiles are not computed; a second kernel copies one depth row of the column's
 * representative tile to each of their rows, so that the caller sees a fully populated tensor.  Here nothing is copied: the
 * producer leaves the duplicates' rows of the split pair and of the side head UNWRITTEN, and each reader of those tensors is given
 * the producer's descriptor and reads the representative's row where a duplicate's would be.  A duplicate tile (d0, w0) of the
 * 4 (d) x 32 (w) tiling has the representative d0' = the first pure d0 of tile column w0 (snvc_dedup.h's rule), and its plane d
 * holds what plane d0' + (d & 3) holds: one remap (d, w) -> d', the identity outside duplicates, the same for every row h.
 *
 * A tensor written this way has exactly one valid use: as the input of an entry point of this header, with the same descriptor.
 */
#ifndef SNVC_ALIAS_H
#define SNVC_ALIAS_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Which rows of a [D][.][W] tensor were not written: the duplicates of snvc_dedup.h's rule under (D, W, q, m0, off).  All zero:
 * none (every row was written). */
typedef struct snvc_wedge_desc {
    int32_t D, W;        /* the producing layer's depth and width */
    int32_t q, m0, off;  /* the fused first layer's q (1 | 2), m0 and off, as given to the producer */
} snvc_wedge_desc;

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_alias_abi_version(void);

/* Host function, no device work: the plane that holds the bits of voxel (d, ., w) of a tensor written under desc -- d itself outside
 * duplicate tiles.  -1 for a null desc, q other than 1 | 2 or (d, w) outside [0, D) x [0, W). */
SNVC_API int64_t snvc_alias_depth(const snvc_wedge_desc *desc, int64_t d, int64_t w);

/* snvc_dedup_fused_first_conv3d_forward (same arguments) WITHOUT the copy: one launch; the duplicates' rows of y_hi / y_lo / y_head
 * keep whatever they held.  Everything written, the overflow word included, is what snvc_fused_first_conv3d_forward writes.  The
 * descriptor of the result is (desc->Din, desc->Win, q, m0, off).  No alignment is asked of y_head beyond its own type's. */
SNVC_API int snvc_alias_fused_first_conv3d_forward(const snvc_conv3d_desc *desc, const void *packed_weight, const float *scale,
                                                   const float *bias, void *y_hi, void *y_lo, const float *head, float *y_head,
                                                   float head_mul, int *overflow, const float *gi, int64_t pitch, int64_t lp,
                                                   const float *p_il, const float *v_scale, const float *v_bias, int q, int m0, int off,
                                                   int off2, int v_flags, void *stream);

/* snvc_f16x3_conv3d_forward of a layer with a split C8 result, no residual and no side head, whose input pair was written under
 * in_alias (in_alias->D == desc->Din, in_alias->W == desc->Win): same results bit for bit as on the fully populated pair.  Built
 * for the stride-2 3x3x3 layer on the 16x16x32 form (SNVC_ALGO_X3_Q16); every other layer or form is refused with
 * SNVC_ERR_UNSUPPORTED and a message, nothing is launched.  in_alias NULL: snvc_f16x3_conv3d_forward itself. */
SNVC_API int snvc_alias_f16x3_conv3d_forward(const snvc_conv3d_desc *desc, const void *x_hi, const void *x_lo, const void *packed_weight,
                                             const float *scale, const float *bias, void *y_hi, void *y_lo, int *overflow,
                                             const snvc_wedge_desc *in_alias, void *stream);

/* snvc_deconv_tail_gather whose residual [n][4 nd][4 nh][4 nw] was written under res_alias (D == 4 nd, W == 4 nw): same results bit
 * for bit.  res_alias NULL: snvc_deconv_tail_gather itself. */
SNVC_API int snvc_alias_deconv_tail_gather(const float *t, const float *bias, const float *residual, float *y, int64_t n, int64_t nd,
                                           int64_t nh, int64_t nw, const snvc_wedge_desc *res_alias, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_ALIAS_H */
