/*
 * snvc_hgdedup.h -- C ABI of the hourglass's duplicate tiles in libsnvc_hip.so (gfx950).  Kept apart from snvc_hip.h, snvc_fused.h,
 * snvc_dedup.h, snvc_forms.h and snvc_alias.h, whose declaration sets and ABI numbers are pinned; this header versions itself through
 * snvc_hgdedup_abi_version().  Conventions are those of snvc_hip.h; snvc_wedge_desc is snvc_alias.h's.
 *
 * snvc_alias.h: the fused first layer's conv2 leaves its duplicate wedge tiles unwritten and its readers look at the representative's
 * rows.  One layer further the same holds at voxel level: conv2's result v2 at (d, w) does not depend on d where the v1 voxels it
 * reads -- planes d - 1 .. d + 1, columns w - 1 .. w + 1 -- all lie on the wedge:
 *     d - 1 >= 1,   d + 1 <= D - 2,   w + 1 < W - 1,   q (w + 1) - (d - 1) - m0 + off < 0.
 * The stride-2 3x3x3 layer behind conv2 (the hourglass's first) works on output tiles of 2 (d) x 4 (h) x 32 (w).  Tile (od0, ow0)
 * reads planes 2 od0 - 1 .. 2 od0 + 3 and columns 2 ow0 - 1 .. 2 ow0 + 63 of v2 and is PURE when all of them are d-invariant:
 *     od0 >= 2,   2 od0 + 4 <= D - 2,   2 ow0 + 64 < W - 1,   q (2 ow0 + 64) - (2 od0 - 2) - m0 + off < 0.
 * A pure tile stores, bit for bit, what tile (od0 - 2, ow0) stores when that one is pure too.  The pure od0 of a tile column are
 * consecutive; the first is the column's representative, the others are DUPLICATES: they are not computed, their rows of the result
 * stay unwritten, and the result's reader looks at plane first + (od & 1) where a duplicate's plane od would be -- one remap
 * (od, ow) -> od', the identity outside duplicates, the same for every row.  The descriptor is still conv2's (D, W, q, m0, off).
 *
 * A tensor written this way has exactly one valid use: as the input of snvc_hgdedup_reader_f16x3_conv3d_forward, with the same
 * descriptor.
 */
#ifndef SNVC_HGDEDUP_H
#define SNVC_HGDEDUP_H

#include <stdint.h>

#include "snvc_alias.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_hgdedup_abi_version(void);

/* The most tile columns with duplicates that the stride-2 launch can leave out; a shape with more is refused there. */
SNVC_API int snvc_hgdedup_max_columns(void);

/* Host function, no device work: 1 when tile (od0, ow0) of the stride-2 result is pure under desc, else 0.  -1 for a null desc, q other
 * than 1 | 2, or an origin off the 2 x 32 grid or outside the result [(D - 1) / 2 + 1] x [(W - 1) / 2 + 1]. */
SNVC_API int snvc_hgdedup_tile_pure(const snvc_wedge_desc *desc, int64_t od0, int64_t ow0);

/* Host function: the duplicates of one (sample, tile row), by the rule's closed form.  For every tile column tw < max_tw, first_td[tw]
 * is the representative's depth tile (od0 / 2) and last_td[tw] the last duplicate's; -1 / -1 for a column without duplicates.  -1 on
 * bad arguments. */
SNVC_API int64_t snvc_hgdedup_tiles(const snvc_wedge_desc *desc, int64_t *first_td, int64_t *last_td, int max_tw);

/* Host function: the plane of the stride-2 result that holds the bits of its voxel (od, ., ow) -- od itself outside duplicate tiles.
 * -1 on bad arguments. */
SNVC_API int64_t snvc_hgdedup_depth(const snvc_wedge_desc *desc, int64_t od, int64_t ow);

/* Host function: the stride-2 launch's walk over the tiles it computes, for a result with tiles_h tile rows.  Returns the live tiles per
 * sample -- all tiles minus tiles_h times snvc_hgdedup_tiles' count -- and, for 0 <= index < that number, writes the (depth tile, tile
 * row, tile column) that live tile `index` is (the function the kernel uses).  0: the shape has no duplicates or more columns with
 * duplicates than snvc_hgdedup_max_columns() (no walk is built).  -1 on bad arguments. */
SNVC_API int64_t snvc_hgdedup_live_tile(const snvc_wedge_desc *desc, int64_t tiles_h, int64_t index, int64_t *td, int64_t *th, int64_t *tw);

/* snvc_alias_f16x3_conv3d_forward (same arguments, in_alias not NULL) whose own duplicate tiles are not computed: their rows of
 * y_hi / y_lo keep whatever they held; everything written, the overflow word included, is what snvc_f16x3_conv3d_forward writes.
 * Without duplicates it is snvc_alias_f16x3_conv3d_forward.  Built for the stride-2 3x3x3 layer on the 16x16x32 form
 * (SNVC_ALGO_X3_Q16) and at most snvc_hgdedup_max_columns() columns with duplicates; anything else is refused with
 * SNVC_ERR_UNSUPPORTED and a message, nothing is launched. */
SNVC_API int snvc_hgdedup_f16x3_conv3d_forward(const snvc_conv3d_desc *desc, const void *x_hi, const void *x_lo, const void *packed_weight,
                                               const float *scale, const float *bias, void *y_hi, void *y_lo, int *overflow,
                                               const snvc_wedge_desc *in_alias, void *stream);

/* snvc_f16x3_conv3d_forward of a layer with a split C8 result, no residual and no side head, whose input pair was written by
 * snvc_hgdedup_f16x3_conv3d_forward under in_desc ((in_desc->D - 1) / 2 + 1 == desc->Din, likewise W): same results bit for bit as on
 * the fully populated pair; every tile is computed and written.  Built for the stride-1 3x3x3 layer on the 16x16x32 form
 * (SNVC_ALGO_X3_Q16); every other layer or form is refused with SNVC_ERR_UNSUPPORTED and a message, nothing is launched. */
SNVC_API int snvc_hgdedup_reader_f16x3_conv3d_forward(const snvc_conv3d_desc *desc, const void *x_hi, const void *x_lo,
                                                      const void *packed_weight, const float *scale, const float *bias, void *y_hi,
                                                      void *y_lo, int *overflow, const snvc_wedge_desc *in_desc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_HGDEDUP_H */
