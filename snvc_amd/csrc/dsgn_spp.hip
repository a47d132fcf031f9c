// SPP head of the DSGN image backbone (include/snvc_dsgn.h) for gfx950.
//
// Reference: snvc/models/submodule.py feature_extraction (:424-442 branch1 .. branch4, :478-512 forward).  The reference
// pools output_skip four times (windows 64, 32, 16, 8), runs a 1x1 convbn + ReLU on each result, upsamples each back to
// H x W with F.interpolate and concatenates.  Here one launch reads output_skip once and writes all four pools, the four
// 1x1 layers run on the depth-1 conv kernels, and one launch upsamples the four branch maps into their channel slices of
// the concat buffer.
//
// Both kernels are memory-bound and small next to the convolutions around them (at 96 x 312 x 192 channels, N = 2, the
// pool reads 46 MB and the upsampling writes 31 MB).
#include "common.hpp"
#include "snvc_dsgn.h"

namespace snvc {
namespace {

constexpr int kThreads = 256;

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned grid_1d(int64_t n) { return (unsigned)((n + kThreads - 1) / kThreads); }

// One workgroup per (n, c) plane.  Pass 1: the 8 x 8 window sums of the plane (row by row, left to right, as
// F.avg_pool2d sums) into LDS, and out8.  Pass 2: every 16 / 32 / 64 window from the 8 x 8 sums.
template <bool VEC>
__global__ __launch_bounds__(kThreads) void spp_pool_kernel(const float *__restrict__ x, int64_t x_bs, float *__restrict__ o8,
                                                            float *__restrict__ o16, float *__restrict__ o32,
                                                            float *__restrict__ o64, int C, int H, int W) {
    __shared__ float cell[SNVC_DSGN_MAX_CELLS];
    const int64_t nc = blockIdx.x;
    const int64_t n = nc / C, c = nc - n * C;
    const float *plane = x + n * x_bs + c * (int64_t)H * W;
    const int h8 = H / 8, w8 = W / 8;
    for (int b = threadIdx.x; b < h8 * w8; b += kThreads) {
        const int by = b / w8, bx = b - by * w8;
        const float *p = plane + (int64_t)(8 * by) * W + 8 * bx;
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if constexpr (VEC) {
                const float4 u = *reinterpret_cast<const float4 *>(p + (int64_t)r * W);
                const float4 v = *reinterpret_cast<const float4 *>(p + (int64_t)r * W + 4);
                s += u.x; s += u.y; s += u.z; s += u.w;
                s += v.x; s += v.y; s += v.z; s += v.w;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) s += p[(int64_t)r * W + e];
            }
        }
        cell[b] = s;
        o8[nc * h8 * w8 + b] = s / 64.0f;
    }
    __syncthreads();
    float *const outs[3] = {o16, o32, o64};
#pragma unroll
    for (int level = 0; level < 3; ++level) {
        const int f = 2 << level, k = 8 * f;         // f x f cells per window of k x k
        const int hk = H / k, wk = W / k;
        for (int o = threadIdx.x; o < hk * wk; o += kThreads) {
            const int oy = o / wk, ox = o - oy * wk;
            float s = 0.0f;
            for (int r = 0; r < f; ++r)
                for (int e = 0; e < f; ++e) s += cell[(oy * f + r) * w8 + ox * f + e];
            outs[level][nc * hk * wk + o] = s / (float)(k * k);
        }
    }
}

struct UpMaps {
    const float *m[4];
    int h[4], w[4];
    float rh[4], rw[4];      // source-index scales, computed on the host as F.interpolate computes them
};

// F.interpolate's source index (area_pixel_compute_source_index, linear modes)
__device__ inline float src_index(float scale, int dst, int align) {
    if (align) return scale * dst;
    const float s = scale * (dst + 0.5f) - 0.5f;
    return s < 0.0f ? 0.0f : s;
}

// One lane per output element of [N][4C][H][W].
__global__ __launch_bounds__(kThreads) void spp_upsample_kernel(UpMaps M, float *__restrict__ y, int64_t y_bs, int64_t total,
                                                                int C, int H, int W, int align) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int ox = (int)(i % W);
    int64_t r = i / W;
    const int oy = (int)(r % H);
    r /= H;
    const int kc = (int)(r % (4 * C));
    const int64_t n = r / (4 * C);
    const int k = kc / C, c = kc - k * C;
    const int ih = M.h[k], iw = M.w[k];
    const float *src = M.m[k] + (n * C + c) * (int64_t)ih * iw;

    const float h1r = src_index(M.rh[k], oy, align);
    const int h1 = (int)h1r;
    const int h1p = (h1 < ih - 1) ? 1 : 0;
    const float h1lambda = h1r - h1;
    const float h0lambda = 1.0f - h1lambda;
    const float w1r = src_index(M.rw[k], ox, align);
    const int w1 = (int)w1r;
    const int w1p = (w1 < iw - 1) ? 1 : 0;
    const float w1lambda = w1r - w1;
    const float w0lambda = 1.0f - w1lambda;
    const float *r0 = src + (int64_t)h1 * iw, *r1 = src + (int64_t)(h1 + h1p) * iw;
    // F.interpolate's h0lambda * (w0lambda * a + w1lambda * b) + h1lambda * (w0lambda * c + w1lambda * d) with the multiply-adds
    // its build fuses, written out so that no compiler choice can change them: bit-exact against it (tests/test_gpu_dsgn.py)
    const float val = __builtin_fmaf(h0lambda, __builtin_fmaf(w0lambda, r0[w1], w1lambda * r0[w1 + w1p]),
                                     h1lambda * __builtin_fmaf(w0lambda, r1[w1], w1lambda * r1[w1 + w1p]));
    y[n * y_bs + (int64_t)kc * H * W + (int64_t)oy * W + ox] = val;
}

// F.interpolate's area_pixel_compute_scale for a given output size (no scale_factor)
float up_scale(int64_t in, int64_t out, int align) {
    if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    return (float)in / (float)out;
}

}  // namespace
}  // namespace snvc

using namespace snvc;

extern "C" {

int snvc_dsgn_abi_version(void) { return 1; }

int snvc_dsgn_spp_pool(const float *x, int64_t x_batch_stride, float *out8, float *out16, float *out32, float *out64, int64_t N,
                       int64_t C, int64_t H, int64_t W, void *stream) {
    if (!x || !out8 || !out16 || !out32 || !out64) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dsgn_spp_pool: null pointer");
    if (N < 0 || C < 0 || H < 64 || W < 64 || H > INT32_MAX || W > INT32_MAX || C > INT32_MAX)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dsgn_spp_pool: needs N, C >= 0 and H, W >= 64 (the 64 x 64 window)");
    if ((H / 8) * (W / 8) > SNVC_DSGN_MAX_CELLS)
        return fail(SNVC_ERR_UNSUPPORTED, "snvc_dsgn_spp_pool: (H / 8) * (W / 8) exceeds SNVC_DSGN_MAX_CELLS");
    const int64_t plane = C * H * W;
    const int64_t xbs = x_batch_stride ? x_batch_stride : plane;
    if (xbs < plane) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dsgn_spp_pool: batch stride below C * H * W");
    if (N * C == 0) return SNVC_OK;
    if (N * C > INT32_MAX) return fail(SNVC_ERR_UNSUPPORTED, "snvc_dsgn_spp_pool: too many planes");
    const bool vec = aligned16(x) && W % 4 == 0 && xbs % 4 == 0;     // every 8-column row segment starts 16-byte aligned
    hipStream_t st = as_stream(stream);
    if (vec)
        spp_pool_kernel<true><<<(unsigned)(N * C), kThreads, 0, st>>>(x, xbs, out8, out16, out32, out64, (int)C, (int)H, (int)W);
    else
        spp_pool_kernel<false><<<(unsigned)(N * C), kThreads, 0, st>>>(x, xbs, out8, out16, out32, out64, (int)C, (int)H, (int)W);
    return check_launch("spp_pool_kernel");
}

int snvc_dsgn_spp_upsample(const float *const *maps_host, const int64_t *extents_host, float *y, int64_t y_batch_stride, int64_t N,
                           int64_t C, int64_t H, int64_t W, int align_corners, void *stream) {
    if (!maps_host || !extents_host || !y) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dsgn_spp_upsample: null pointer");
    if (N < 0 || C < 0 || H <= 0 || W <= 0 || H > INT32_MAX || W > INT32_MAX || C > INT32_MAX / 4)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dsgn_spp_upsample: bad N / C / H / W");
    const int64_t slab = 4 * C * H * W;
    const int64_t ybs = y_batch_stride ? y_batch_stride : slab;
    if (ybs < slab) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_dsgn_spp_upsample: batch stride below 4 * C * H * W");
    UpMaps M{};
    for (int k = 0; k < 4; ++k) {
        const int64_t h = extents_host[2 * k], w = extents_host[2 * k + 1];
        if (!maps_host[k] || h <= 0 || w <= 0 || h > H || w > W) {
            set_error("snvc_dsgn_spp_upsample: map %d is NULL or its extent %lld x %lld is not within 1 .. %lld x %lld", k,
                      (long long)h, (long long)w, (long long)H, (long long)W);
            return SNVC_ERR_INVALID_ARGUMENT;
        }
        M.m[k] = maps_host[k];
        M.h[k] = (int)h; M.w[k] = (int)w;
        M.rh[k] = up_scale(h, H, align_corners);
        M.rw[k] = up_scale(w, W, align_corners);
    }
    const int64_t total = N * slab;
    if (total == 0) return SNVC_OK;
    spp_upsample_kernel<<<grid_1d(total), kThreads, 0, as_stream(stream)>>>(M, y, ybs, total, (int)C, (int)H, (int)W,
                                                                              align_corners ? 1 : 0);
    return check_launch("spp_upsample_kernel");
}

}  // extern "C"
