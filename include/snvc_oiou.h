/*
 * snvc_oiou.h -- C ABI of the oriented-box IoU / DIoU / GIoU losses in libsnvc_hip.so (gfx950), the native side of
 * snvc_amd.thirdparty.oriented_iou_loss.  Kept apart from snvc_hip.h, whose declaration set and ABI number are pinned; this
 * header versions itself through snvc_oiou_abi_version().
 *
 * Conventions are those of snvc_loss.h: device pointers, `stream` is a hipStream_t passed as void* (NULL = default stream),
 * every call is asynchronous on it, allocates nothing and never waits for the device, int status return (snvc_status),
 * snvc_last_error_string() for the text of the last failure on the calling thread.  Every argument is checked on the host
 * before anything is launched.  Tensors are dense float32.
 *
 * A call serves M pairs (subject, clip).  Per pair the forward writes eight floats
 *     out[m] = { inter, area1, area2, u, iou, enc_w, enc_h, loss }
 * (DESIGN.md "Oriented IoU" has the definitions) in one launch.  The backward is one launch as well: it recomputes the pair
 * with one forward-mode tangent per input scalar and writes d(sum_k gout[m][k] out[m][k]) / d(input) for every input element
 * of the pair, each element once.  No atomics: the same input gives the same bits.
 */
#ifndef SNVC_OIOU_H
#define SNVC_OIOU_H

#include <stdint.h>

#include "snvc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Version of this header's ABI; bumped on any signature change. */
SNVC_API int snvc_oiou_abi_version(void);

enum snvc_oiou_form {
    SNVC_OIOU_BOXES = 0,   /* a, b: [M][5] = x, y, w, h, alpha; ctr_a, ctr_b unused (NULL) */
    SNVC_OIOU_QUADS = 1    /* a, b: [M][4][2] corners; ctr_a, ctr_b: [M][2] centres (they enter the DIoU distance only) */
};

enum snvc_oiou_kind {
    SNVC_OIOU_DIOU = 0,    /* loss = 1 - iou + d^2 / (enc_w^2 + enc_h^2) */
    SNVC_OIOU_GIOU = 1     /* loss = 1 - iou + (enc_w enc_h - u) / (enc_w enc_h) */
};

enum snvc_oiou_enclosing {
    SNVC_OIOU_SMALLEST = 0,   /* the least-area rectangle flush with a hull line of the eight corners */
    SNVC_OIOU_ALIGNED = 1     /* the axis-aligned box of the eight corners */
};

#define SNVC_OIOU_OUT 8       /* floats per pair in out / gout */

typedef struct snvc_oiou_desc {
    int32_t form;           /* snvc_oiou_form */
    int32_t kind;           /* snvc_oiou_kind */
    int32_t enclosing;      /* snvc_oiou_enclosing */
    int32_t reserved;       /* 0 */
    int64_t M;              /* pairs; 0 succeeds and launches nothing */
    const float *a;         /* subject, see the form */
    const float *b;         /* clip, see the form */
    const float *ctr_a;     /* QUADS: [M][2] */
    const float *ctr_b;     /* QUADS: [M][2] */
    float *out;             /* forward: [M][8], every element written */
    const float *gout;      /* backward: [M][8] upstream gradient of out */
    float *ga;              /* backward: gradient for a, same shape, every element written */
    float *gb;              /* backward: gradient for b */
    float *gctr_a;          /* backward, QUADS: gradient for ctr_a */
    float *gctr_b;          /* backward, QUADS: gradient for ctr_b */
} snvc_oiou_desc;

/* One launch.  Reads a, b (ctr_a, ctr_b); writes out. */
SNVC_API int snvc_oiou_forward(const snvc_oiou_desc *desc, void *stream);
/* One launch.  Reads a, b (ctr_a, ctr_b) and gout; writes ga, gb (gctr_a, gctr_b). */
SNVC_API int snvc_oiou_backward(const snvc_oiou_desc *desc, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SNVC_OIOU_H */
