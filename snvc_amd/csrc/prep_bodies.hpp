// Bodies of the two split-pair producers of the first layer's 2D prep, shared between their own kernels (sheared_conv.hip,
// layout_f16.hip) and the pooled producer launch (split_producers_kernel, conv3d_f16.hip; include/snvc_prep.h): one definition, so a
// pooled block stores what the single launch's block stores.  The block index (and for the 3D grid its y / z) is an argument: the
// single kernels pass their blockIdx, the pooled kernel the index inside its block range.
#pragma once
#include "common.hpp"

namespace snvc {
namespace prep {

typedef _Float16 h8p __attribute__((ext_vector_type(8)));

// sheared_upsample_split_kernel: Rq as a split C8 pair [N][2][C/8][H][WU][8], value * *mul_dev = hi + lo.  A thread = one position of
// one 8-channel group.
__device__ __forceinline__ void sheared_upsample_split_body(const float *r, _Float16 *yh, _Float16 *yl,
                                                            const float *mul_dev, int C, int H, int W, int q, int WU, int off,
                                                            int64_t total, unsigned bx) {
#pragma clang fp contract(off)
    const int64_t idx = (int64_t)bx * 256 + threadIdx.x;          // ((n * G + g) * H + h) * WU + i
    if (idx >= total) return;
    const int i = (int)(idx % WU), u = i - off;
    const int64_t t = idx / WU;
    const int h = (int)(t % H);
    const int64_t ng = t / H;
    const int G = (C + 7) >> 3, g = (int)(ng % G);
    const int64_t n = ng / G;
    const float mul = mul_dev[0];
    h8p hi, lo;
    const bool in = u >= 0 && u <= q * (W - 1);
    const int j = in ? u / q : 0;
    const bool whole = u - j * q == 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float v = 0.0f;
        const int co = g * 8 + c;
        if (in && co < C) {
            const float *rr = r + ((n * C + co) * (int64_t)H + h) * W;
            v = whole ? rr[j] : 0.5f * rr[j] + 0.5f * rr[j + 1];
        }
        v *= mul;
        hi[c] = (_Float16)v;
        lo[c] = (_Float16)(v - (float)hi[c]);
    }
    // [N][2 (hi | lo)][G][H][WU] pieces: a sample's two planes sit next to each other
    const int64_t pos = ((n * 2 * G + g) * (int64_t)H + h) * WU + i;
    *reinterpret_cast<h8p *>(yh + pos * 8) = hi;
    *reinterpret_cast<h8p *>(yl + pos * 8) = lo;
}

// ncdhw_f32_to_c8_split_kernel: value * mul (a power of two) = hi + lo, two C8 half planes; position s of channel group g of sample n
__device__ __forceinline__ void ncdhw_f32_to_c8_split_body(const float *x, _Float16 *yh, _Float16 *yl, int C,
                                                           int64_t S, int64_t x_bs, int64_t y_bs, float mul, const float *mul_dev,
                                                           int64_t s, int g, int64_t n) {
    if (s >= S) return;
    if (mul_dev) mul = *mul_dev;             // the scale chosen on the device (no host round trip): a power of two
    const float *xp = x + n * x_bs + (int64_t)g * 8 * S + s;
    h8p o, ol;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = (g * 8 + e < C) ? xp[(int64_t)e * S] * mul : 0.0f;
        o[e] = (_Float16)v;
        ol[e] = (_Float16)(v - (float)o[e]);
    }
    *reinterpret_cast<h8p *>(yh + n * y_bs + ((int64_t)g * S + s) * 8) = o;
    *reinterpret_cast<h8p *>(yl + n * y_bs + ((int64_t)g * S + s) * 8) = ol;
}

}  // namespace prep
}  // namespace snvc
