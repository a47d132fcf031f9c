// Training losses (include/snvc_loss.h) for gfx950.
//
// Reference: snvc/models/loss3d.py.  There each loss is 15 - 45 elementwise launches with boolean-mask gathers and a host
// synchronisation (`if mask.sum() > 0`) in the middle.  Here a loss is one streaming pass plus a one-workgroup finalisation,
// and its gradient one more pass; mask counts and normalisers never leave the device.
//
// Reduction scheme (deterministic, no floating-point atomics): per-lane fp32 sums -> wave reduction (__shfl_down) -> the
// waves of a workgroup added in wave order -> one fp32 partial per workgroup in a workspace -> finalize_kernel adds the
// partials in float64 in a fixed order (a strided sum per lane, then a fixed LDS tree).
//
// All kernels are memory-bound; the measure is bytes over time (float4 loads wherever alignment allows).
#include "common.hpp"
#include "snvc_loss.h"

namespace snvc {
namespace {

constexpr int kThreads = 256;
constexpr int kIters = 4;            // float4 (or scalar) steps per lane of an elementwise workgroup
constexpr int kMaxK = 4;             // accumulators per workgroup partial

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

// ------------------------------------------------------------------------------------------------ reductions
// acc[K] of every lane -> dst[K] (one partial per workgroup).  blockDim.x is a multiple of 64, at most 1024.
template <int K>
__device__ inline void block_reduce_store(const float (&acc)[K], float *dst) {
    __shared__ float red[16][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) {
        float s = 0.0f;
        for (int w = 0; w < waves; ++w) s += red[w][threadIdx.x];
        dst[threadIdx.x] = s;
    }
}

// Sum of one double per lane over the 256 lanes of the finalisation workgroup, fixed tree; every lane gets the result.
__device__ inline double block_sum_f64(double v) {
    __shared__ double tree[kThreads];
    __syncthreads();                       // the previous call's readers are done
    tree[threadIdx.x] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) tree[threadIdx.x] += tree[threadIdx.x + s];
        __syncthreads();
    }
    return tree[0];
}

// ------------------------------------------------------------------------------------------------ per-element formulas
__device__ inline float sgn(float d) { return (d > 0.0f) ? 1.0f : ((d < 0.0f) ? -1.0f : 0.0f); }
__device__ inline float pw(float x, float gamma) { return gamma == 2.0f ? x * x : powf(x, gamma); }
__device__ inline float dpw(float x, float gamma) { return gamma == 2.0f ? 2.0f * x : gamma * powf(x, gamma - 1.0f); }

// the focal term of OccupancyLoss / sigmoid_focal_loss_multi_target for a target t in {0, 1} (anything else: 0)
__device__ inline float focal_value(float t, float p, float alpha, float gamma) {
    if (t == 1.0f) return -(pw(1.0f - p, gamma) * logf(p + 1e-7f)) * alpha;
    if (t == 0.0f) return -(pw(p, gamma) * logf((1.0f - p) + 1e-7f)) * (1.0f - alpha);
    return 0.0f;
}
__device__ inline float focal_dp(float t, float p, float alpha, float gamma) {
    if (t == 1.0f) {
        const float q = 1.0f - p, u = p + 1e-7f;
        return -(pw(q, gamma) / u - dpw(q, gamma) * logf(u)) * alpha;
    }
    if (t == 0.0f) {
        const float u = (1.0f - p) + 1e-7f;
        return -(dpw(p, gamma) * logf(u) - pw(p, gamma) / u) * (1.0f - alpha);
    }
    return 0.0f;
}
__device__ inline float sl1_value(float d, float beta) {
    const float n = fabsf(d);
    return n < beta ? 0.5f * n * n / beta : n - 0.5f * beta;
}
__device__ inline float sl1_grad(float d, float beta) { return fabsf(d) < beta ? d / beta : sgn(d); }

template <int V>
__device__ inline void load_f32(const float *p, int64_t i, float (&out)[V]) {
    if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(p + i);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
        out[0] = p[i];
    }
}
template <int V>
__device__ inline void load_u8(const uint8_t *p, int64_t i, float (&out)[V]) {
    if constexpr (V == 4) {
        const uint32_t v = *reinterpret_cast<const uint32_t *>(p + i);
        out[0] = (float)(v & 255u); out[1] = (float)((v >> 8) & 255u); out[2] = (float)((v >> 16) & 255u); out[3] = (float)(v >> 24);
    } else {
        out[0] = (float)p[i];
    }
}
// integer targets, converted to float (exact for the label values a loss compares against)
template <int V>
__device__ inline void load_i32(const int32_t *p, int64_t i, float (&out)[V]) {
    if constexpr (V == 4) {
        const int4 v = *reinterpret_cast<const int4 *>(p + i);
        out[0] = (float)v.x; out[1] = (float)v.y; out[2] = (float)v.z; out[3] = (float)v.w;
    } else {
        out[0] = (float)p[i];
    }
}
template <int V>
__device__ inline void load_i64(const int64_t *p, int64_t i, float (&out)[V]) {
    if constexpr (V == 4) {
        const longlong2 u = *reinterpret_cast<const longlong2 *>(p + i), v = *reinterpret_cast<const longlong2 *>(p + i + 2);
        out[0] = (float)u.x; out[1] = (float)u.y; out[2] = (float)v.x; out[3] = (float)v.y;
    } else {
        out[0] = (float)p[i];
    }
}
template <int V>
__device__ inline void load_target(const void *p, int flags, int64_t i, float (&out)[V]) {
    if (flags & SNVC_LOSS_TARGET_INT32) load_i32<V>(static_cast<const int32_t *>(p), i, out);
    else if (flags & SNVC_LOSS_TARGET_INT64) load_i64<V>(static_cast<const int64_t *>(p), i, out);
    else if (flags & SNVC_LOSS_TARGET_UINT8) load_u8<V>(static_cast<const uint8_t *>(p), i, out);
    else load_f32<V>(static_cast<const float *>(p), i, out);
}
template <int V>
__device__ inline void store_f32(float *p, int64_t i, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p + i) = make_float4(v[0], v[1], v[2], v[3]);
    else p[i] = v[0];
}

// ------------------------------------------------------------------------------------------------ elementwise kinds
// What a kind's pass needs on the device (a copy of snvc_loss_desc's pointers and numbers).
struct EwArgs {
    const float *a, *roww;
    const void *b, *c;
    const double *fin;
    const float *gout;
    float *ga;
    int64_t cols, group;
    float p0, p1;
    int flags;
};

// Each Op: K accumulators; begin_row() once per lane (row scalars); elem() per element: forward adds to acc, backward
// returns the gradient.  `x` is the third operand's value where the kind has one (HAS_C: float32 at the same index;
// C_U8: uint8 at the same index; C_SHARED: float32 at (row / group) * cols + col).
enum { C_NONE = 0, C_F32 = 1, C_U8 = 2, C_SHARED = 3 };

struct OpMseRows {
    static constexpr int K = 1, CMODE = C_NONE;
    float w, scale;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t row) {
        w = g.roww ? g.roww[row] : 1.0f;
        if (BWD) scale = (float)(g.fin[0] * (double)g.gout[0]);
    }
    template <bool BWD> __device__ float elem(const EwArgs &, int64_t, float a, float b, float, float (&acc)[K]) {
        const float d = a * w - b * w;
        if (BWD) return 2.0f * w * d * scale;
        acc[0] += d * d;
        return 0.0f;
    }
};

struct OpMsePosNeg {
    static constexpr int K = 4, CMODE = C_NONE;
    float sp, sn;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t row) {
        if (BWD) {
            const int64_t k = row % g.group;
            sp = (float)(g.fin[2 * k] * (double)g.gout[0]);
            sn = (float)(g.fin[2 * k + 1] * (double)g.gout[0]);
        }
    }
    template <bool BWD> __device__ float elem(const EwArgs &, int64_t, float a, float b, float, float (&acc)[K]) {
        const float d = a - b;
        const bool pos = b > 0.0f, neg = b <= 0.0f;
        if (BWD) return pos ? 2.0f * d * sp : (neg ? 2.0f * d * sn : 0.0f);
        if (pos) { acc[0] += d * d; acc[1] += 1.0f; }
        else if (neg) { acc[2] += d * d; acc[3] += 1.0f; }
        return 0.0f;
    }
};

struct OpOccupancy {
    static constexpr int K = 2, CMODE = C_NONE;
    float scale;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t) {
        if (BWD) scale = (float)(g.fin[0] * (double)g.gout[0]);
    }
    template <bool BWD> __device__ float elem(const EwArgs &g, int64_t, float p, float t, float, float (&acc)[K]) {
        if (t == -1.0f) return 0.0f;
        if (BWD) return focal_dp(t, p, g.p0, g.p1) * scale;
        acc[0] += focal_value(t, p, g.p0, g.p1);
        acc[1] += 1.0f;
        return 0.0f;
    }
};

struct OpOffset {
    static constexpr int K = 2, CMODE = C_SHARED;
    float scale;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t) {
        if (BWD) scale = (float)(g.fin[0] * (double)g.gout[0]);
    }
    template <bool BWD> __device__ float elem(const EwArgs &, int64_t, float a, float b, float occ, float (&acc)[K]) {
        if (!(occ == 1.0f)) return 0.0f;
        const float d = a - b;
        if (BWD) return sgn(d) * scale;
        acc[0] += fabsf(d);
        acc[1] += 1.0f;
        return 0.0f;
    }
};

struct OpSmoothL1Masked {
    static constexpr int K = 2, CMODE = C_U8;
    float scale;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t) {
        if (BWD) scale = (float)(g.fin[0] * (double)g.gout[0]);
    }
    template <bool BWD> __device__ float elem(const EwArgs &g, int64_t, float a, float b, float m, float (&acc)[K]) {
        const bool valid = g.c ? (m != 0.0f) : (b != -1.0f && b < 60.0f);
        if (!valid) return 0.0f;
        const float d = a - b;
        if (BWD) return sl1_grad(d, g.p0) * scale;
        acc[0] += sl1_value(d, g.p0);
        acc[1] += 1.0f;
        return 0.0f;
    }
};

struct OpSigmoidFocal {
    static constexpr int K = 2, CMODE = C_F32;
    float scale;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t) {
        if (BWD) scale = g.gout[0];
    }
    template <bool BWD> __device__ float elem(const EwArgs &g, int64_t, float x, float t, float w, float (&acc)[K]) {
        if (!g.c) w = 1.0f;
        const float p = 1.0f / (1.0f + expf(-x));
        if (BWD) return focal_dp(t, p, g.p0, g.p1) * (p * (1.0f - p)) * w * scale;
        acc[0] += focal_value(t, p, g.p0, g.p1) * w;
        if (!(t == 0.0f || t == 1.0f)) acc[1] += 1.0f;
        return 0.0f;
    }
};

struct OpSmoothL1Rows {
    static constexpr int K = 2, CMODE = C_NONE;
    float scale;
    template <bool BWD> __device__ void begin_row(const EwArgs &g, int64_t) {
        if (BWD) scale = (float)(g.fin[0] * (double)g.gout[0]);
    }
    template <bool BWD> __device__ float elem(const EwArgs &g, int64_t col, float a, float b, float, float (&acc)[K]) {
        // the row of a flat index: a 32-bit division wherever the tensor allows it (the 64-bit one costs several times as much)
        const int64_t m = g.cols <= (int64_t)UINT32_MAX ? (int64_t)((uint32_t)col / (uint32_t)g.group) : col / g.group;
        const float w = g.roww[m], d = a - b;
        if (BWD) return sl1_grad(d, g.p0) * w * scale;
        acc[0] += sl1_value(d, g.p0) * w;
        if (col - m * g.group == 0) acc[1] += w;
        return 0.0f;
    }
};

// grid (ceil(cols / (kThreads * kIters * V)), rows).  V = 4 needs cols % 4 == 0 and 16-byte aligned operands, so that a
// lane's four elements share a row and every access is aligned.
template <class OP, int V, bool BWD>
__global__ __launch_bounds__(kThreads) void ew_kernel(EwArgs g, float *__restrict__ partials) {
    const int64_t row = blockIdx.y;
    OP op;
    op.template begin_row<BWD>(g, row);
    const int64_t base = row * g.cols;
    const int64_t cbase = OP::CMODE == C_SHARED ? (row / g.group) * g.cols : base;
    const int64_t tile0 = (int64_t)blockIdx.x * (kThreads * kIters * V);
    float acc[OP::K];
#pragma unroll
    for (int k = 0; k < OP::K; ++k) acc[k] = 0.0f;
#pragma unroll
    for (int it = 0; it < kIters; ++it) {
        const int64_t col = tile0 + ((int64_t)it * kThreads + threadIdx.x) * V;
        if (col >= g.cols) continue;                     // cols % V == 0: col < cols means col + V <= cols
        float a[V], b[V], c[V], out[V];
        load_f32<V>(g.a, base + col, a);
        load_target<V>(g.b, g.flags, base + col, b);
#pragma unroll
        for (int e = 0; e < V; ++e) c[e] = 0.0f;
        if (OP::CMODE != C_NONE && g.c) {
            if constexpr (OP::CMODE == C_U8) load_u8<V>(static_cast<const uint8_t *>(g.c), cbase + col, c);
            else load_f32<V>(static_cast<const float *>(g.c), cbase + col, c);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) out[e] = op.template elem<BWD>(g, col + e, a[e], b[e], c[e], acc);
        if (BWD) store_f32<V>(g.ga, base + col, out);
    }
    if (!BWD) block_reduce_store<OP::K>(acc, partials + (row * gridDim.x + blockIdx.x) * OP::K);
}

constexpr int kKindK[SNVC_LOSS_KINDS] = {OpMseRows::K, OpMsePosNeg::K, OpOccupancy::K, OpOffset::K, OpSmoothL1Masked::K,
                                         OpSigmoidFocal::K, OpSmoothL1Rows::K};

// Finalisation kinds beyond the elementwise ones: (sum, count) -> mean, NaN when empty; the same, 0 when empty
enum { FIN_MEAN_NAN = 100, FIN_MEAN_ZERO = 101 };

// One workgroup.  partials [blocks][K] (MSE_POSNEG: block = (n * group + part) * nbx + bx) -> fin, loss, flag.
__global__ __launch_bounds__(kThreads) void finalize_kernel(int kind, int flags, const float *__restrict__ partials, int64_t blocks,
                                                            int K, int64_t nbx, int64_t rows, int64_t cols, int64_t group,
                                                            double *__restrict__ fin, float *__restrict__ loss,
                                                            int32_t *__restrict__ flag) {
    if (kind == SNVC_LOSS_MSE_POSNEG) {
        const int64_t samples = rows / group;
        double total = 0.0;
        bool missing = false;
        for (int64_t part = 0; part < group; ++part) {
            double T[4];
            for (int k = 0; k < 4; ++k) {
                double v = 0.0;
                for (int64_t j = threadIdx.x; j < samples * nbx; j += kThreads) {
                    const int64_t n = j / nbx, bx = j - n * nbx;
                    v += (double)partials[((n * group + part) * nbx + bx) * 4 + k];
                }
                T[k] = block_sum_f64(v);
            }
            if (threadIdx.x == 0) {
                fin[2 * part] = 0.5 / ((double)group * T[1]);
                fin[2 * part + 1] = 0.5 / ((double)group * T[3]);
            }
            total += 0.5 * (T[0] / T[1] + T[2] / T[3]);       // an empty half is 0 / 0 = NaN, as the mean of nothing is
            missing |= !(T[1] > 0.0);
        }
        if (threadIdx.x == 0) {
            loss[0] = (float)(total / (double)group);
            if (missing) atomicOr(flag, SNVC_LOSS_FLAG_NO_POSITIVE);
        }
        return;
    }
    double T[kMaxK] = {0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < K; ++k) {
        double v = 0.0;
        for (int64_t j = threadIdx.x; j < blocks; j += kThreads) v += (double)partials[j * K + k];
        T[k] = block_sum_f64(v);
    }
    if (threadIdx.x != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    switch (kind) {
    case SNVC_LOSS_MSE_ROWS:
        fin[0] = 1.0 / ((double)rows * (double)cols);
        loss[0] = (float)(T[0] * fin[0]);
        break;
    case SNVC_LOSS_SIGMOID_FOCAL:
        fin[0] = 1.0;
        loss[0] = (float)T[0];
        if (T[1] > 0.0) atomicOr(flag, SNVC_LOSS_FLAG_BAD_TARGET);
        break;
    case SNVC_LOSS_SMOOTH_L1_ROWS:
        fin[0] = 1.0 / ((double)group * T[1]);
        loss[0] = (float)(T[0] / ((double)group * T[1]));
        break;
    default: {                                              // (sum, count) -> mean
        const bool empty = !(T[1] > 0.0);
        const bool nan_if_empty = kind == FIN_MEAN_NAN || (kind == SNVC_LOSS_SMOOTH_L1_MASKED && (flags & SNVC_LOSS_EMPTY_IS_NAN));
        fin[0] = empty ? 0.0 : 1.0 / T[1];
        fin[1] = T[1];
        loss[0] = empty ? (nan_if_empty ? (float)nan : 0.0f) : (float)(T[0] / T[1]);
        break;
    }
    }
}

// ------------------------------------------------------------------------------------------------ W_loss
constexpr int kWdPlanes = 8;          // depth planes per workgroup of the mean form

// grid (ceil(HW / (kThreads * V)), chunks, B); a workgroup covers kThreads * V pixels over `planes` depth planes.
template <int V, bool BWD>
__global__ __launch_bounds__(kThreads) void wdist_kernel(const float *__restrict__ prob, const float *__restrict__ off,
                                                         const float *__restrict__ target, const uint8_t *__restrict__ mask,
                                                         const float *__restrict__ levels, int64_t D, int64_t HW, int planes,
                                                         float *__restrict__ pixel_loss, float *__restrict__ partials,
                                                         const double *__restrict__ fin, const float *__restrict__ gout,
                                                         const float *__restrict__ gpix, float *__restrict__ gprob,
                                                         float *__restrict__ goff) {
    const int64_t b = blockIdx.z, chunk = blockIdx.y;
    const int64_t col = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * V;
    float acc[2] = {0.0f, 0.0f};
    if (col < HW) {
        float t[V], m[V], g[V], pix[V];
        load_f32<V>(target, b * HW + col, t);
        load_u8<V>(mask, b * HW + col, m);
        if (BWD) {
            if (gpix) load_f32<V>(gpix, b * HW + col, g);
            else {
                const float s = (float)(fin[0] * (double)gout[0]);
#pragma unroll
                for (int e = 0; e < V; ++e) g[e] = s;
            }
        }
#pragma unroll
        for (int e = 0; e < V; ++e) pix[e] = 0.0f;
        const int64_t d0 = chunk * planes, d1 = (d0 + planes < D) ? d0 + planes : D;
        for (int64_t d = d0; d < d1; ++d) {
            const int64_t at = (b * D + d) * HW + col;
            const float lev = levels[d];
            float p[V], o[V], gp[V], go[V];
            load_f32<V>(prob, at, p);
            load_f32<V>(off, at, o);
#pragma unroll
            for (int e = 0; e < V; ++e) {
                const float diff = (lev + o[e]) - t[e];
                const bool valid = m[e] != 0.0f;
                if (BWD) {
                    gp[e] = valid ? fabsf(diff) * g[e] : 0.0f;
                    go[e] = valid ? p[e] * sgn(diff) * g[e] : 0.0f;
                } else if (valid) {
                    pix[e] += p[e] * fabsf(diff);
                }
            }
            if (BWD) {
                if (gprob) store_f32<V>(gprob, at, gp);
                if (goff) store_f32<V>(goff, at, go);
            }
        }
        if (!BWD) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                acc[0] += pix[e];
                if (chunk == 0 && m[e] != 0.0f) acc[1] += 1.0f;
            }
            if (pixel_loss) store_f32<V>(pixel_loss, b * HW + col, pix);
        }
    }
    if (!BWD) block_reduce_store<2>(acc, partials + ((b * gridDim.y + chunk) * gridDim.x + blockIdx.x) * 2);
}

// ------------------------------------------------------------------------------------------------ depth_regression_loss
constexpr int kDrSlices = 8;          // waves of a workgroup = slices of D; lane = pixel
constexpr int kDrThreads = 64 * kDrSlices;
constexpr int kDrCache = 32;          // planes of a slice kept in registers (D <= kDrSlices * kDrCache)

// grid (ceil(HW / 64), B).  Wave s of a workgroup takes planes [s * per, (s + 1) * per) of its 64 pixels: the maximum, then
// sum exp(x - max) and sum exp(x - max) * level; the eight (max, sum, weighted sum) triples of a pixel are merged through LDS.
// CACHED keeps the slice's planes in registers, so that the cost volume is read once in either direction.
template <bool CACHED, bool BWD>
__global__ __launch_bounds__(kDrThreads) void depth_regression_kernel(const float *__restrict__ cost, const float *__restrict__ levels,
                                                                      const float *__restrict__ gt, int64_t D, int64_t HW, int per,
                                                                      float *__restrict__ partials, const double *__restrict__ fin,
                                                                      const float *__restrict__ gout, float *__restrict__ gcost) {
    __shared__ float sm[kDrSlices][64], ss[kDrSlices][64], se[kDrSlices][64];
    __shared__ float pm[64], ps[64], pd[64], pg[64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int64_t b = blockIdx.y, pixel = (int64_t)blockIdx.x * 64 + lane;
    const bool inside = pixel < HW;
    const float target = inside ? gt[b * HW + pixel] : -1.0f;
    const bool valid = inside && target != -1.0f && target < 60.0f;
    const int64_t d0 = (int64_t)slice * per;
    const int count = (int)((d0 + per <= D) ? per : (D > d0 ? D - d0 : 0));
    const float *column = cost + (b * D + d0) * HW + pixel;
    float v[CACHED ? kDrCache : 1];
    float m = -INFINITY, s = 0.0f, e = 0.0f;
    if (valid) {
        if constexpr (CACHED) {
#pragma unroll
            for (int i = 0; i < kDrCache; ++i) v[i] = (i < count) ? column[(int64_t)i * HW] : -INFINITY;
#pragma unroll
            for (int i = 0; i < kDrCache; ++i) m = fmaxf(m, v[i]);
#pragma unroll
            for (int i = 0; i < kDrCache; ++i)
                if (i < count) {
                    const float w = expf(v[i] - m);
                    s += w;
                    e += w * levels[d0 + i];
                }
        } else {
            for (int i = 0; i < count; ++i) m = fmaxf(m, column[(int64_t)i * HW]);
            for (int i = 0; i < count; ++i) {
                const float w = expf(column[(int64_t)i * HW] - m);
                s += w;
                e += w * levels[d0 + i];
            }
        }
    }
    sm[slice][lane] = m; ss[slice][lane] = s; se[slice][lane] = e;
    __syncthreads();
    float acc[2] = {0.0f, 0.0f};
    if (slice == 0) {
        float M = -INFINITY, S = 0.0f, E = 0.0f, depth = 0.0f, g = 0.0f;
        if (valid) {
#pragma unroll
            for (int k = 0; k < kDrSlices; ++k) M = fmaxf(M, sm[k][lane]);
#pragma unroll
            for (int k = 0; k < kDrSlices; ++k) {
                const float f = (ss[k][lane] > 0.0f) ? expf(sm[k][lane] - M) : 0.0f;      // an empty slice has max -inf
                S += ss[k][lane] * f;
                E += se[k][lane] * f;
            }
            depth = E / S;
            const float diff = depth - target;
            if (BWD) g = sl1_grad(diff, 1.0f) * (float)(fin[0] * (double)gout[0]);
            else { acc[0] = sl1_value(diff, 1.0f); acc[1] = 1.0f; }
        }
        if (BWD) { pm[lane] = M; ps[lane] = S; pd[lane] = depth; pg[lane] = g; }
    }
    if constexpr (!BWD) {
        block_reduce_store<2>(acc, partials + (b * gridDim.x + blockIdx.x) * 2);
    } else {
        __syncthreads();
        if (!inside) return;
        const float M = pm[lane], depth = pd[lane], gs = valid ? pg[lane] / ps[lane] : 0.0f;
        float *gcol = gcost + (b * D + d0) * HW + pixel;
        if constexpr (CACHED) {
#pragma unroll
            for (int i = 0; i < kDrCache; ++i)
                if (i < count) gcol[(int64_t)i * HW] = valid ? gs * expf(v[i] - M) * (levels[d0 + i] - depth) : 0.0f;
        } else {
            for (int i = 0; i < count; ++i)
                gcol[(int64_t)i * HW] = valid ? gs * expf(column[(int64_t)i * HW] - M) * (levels[d0 + i] - depth) : 0.0f;
        }
    }
}

// gx[n][d][i] = gy[n][i] * depth[d]; grid (ceil(HW / (kThreads * V)), D, N)
template <int V>
__global__ __launch_bounds__(kThreads) void disparity_regression_bwd_kernel(const float *__restrict__ gy, const float *__restrict__ depth,
                                                                            float *__restrict__ gx, int64_t D, int64_t HW) {
    const int64_t n = blockIdx.z, d = blockIdx.y;
    const int64_t col = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * V;
    if (col >= HW) return;
    const float lev = depth[d];
    float g[V];
    load_f32<V>(gy, n * HW + col, g);
#pragma unroll
    for (int e = 0; e < V; ++e) g[e] *= lev;
    store_f32<V>(gx, (n * D + d) * HW + col, g);
}

// ------------------------------------------------------------------------------------------------ host side
struct EwPlan {
    int K;
    bool vec;
    int64_t nbx;
};

// Validates everything of `d` that both directions use; returns a status and fills `plan`.
int plan_elementwise(const snvc_loss_desc *d, const char *what, EwPlan *plan) {
    if (!d) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: null descriptor");
    if (d->kind < 0 || d->kind >= SNVC_LOSS_KINDS) {
        set_error("%s: unknown kind %d", what, d->kind);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (d->rows < 1 || d->cols < 0 || d->group < 1) {
        set_error("%s: needs rows >= 1, cols >= 0, group >= 1 (got %lld, %lld, %lld)", what, (long long)d->rows, (long long)d->cols,
                  (long long)d->group);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    const int kind = d->kind;
    const bool by_rows = kind == SNVC_LOSS_MSE_POSNEG || kind == SNVC_LOSS_OFFSET || (kind == SNVC_LOSS_MSE_ROWS && d->roww);
    if (!by_rows && d->rows != 1) {
        set_error("%s: kind %d is flat (rows = 1)", what, kind);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (d->rows > SNVC_LOSS_MAX_ROWS) {
        set_error("%s: rows %lld above SNVC_LOSS_MAX_ROWS", what, (long long)d->rows);
        return SNVC_ERR_UNSUPPORTED;
    }
    if ((kind == SNVC_LOSS_MSE_POSNEG || kind == SNVC_LOSS_OFFSET) && d->rows % d->group != 0) {
        set_error("%s: rows %lld is not a multiple of group %lld", what, (long long)d->rows, (long long)d->group);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (kind == SNVC_LOSS_SMOOTH_L1_ROWS && d->cols % d->group != 0) {
        set_error("%s: cols %lld is not a multiple of group %lld", what, (long long)d->cols, (long long)d->group);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (d->cols > 0 && (!d->a || !d->b)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: null prediction or target");
    const int tflags = d->flags & (SNVC_LOSS_TARGET_INT32 | SNVC_LOSS_TARGET_INT64 | SNVC_LOSS_TARGET_UINT8);
    if (tflags && (kind != SNVC_LOSS_SIGMOID_FOCAL || (tflags & (tflags - 1))))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: one SNVC_LOSS_TARGET_* flag at most, and for SIGMOID_FOCAL only");
    if (d->cols > 0 && kind == SNVC_LOSS_OFFSET && !d->c) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: OFFSET needs c (occupancy)");
    if (d->cols > 0 && kind == SNVC_LOSS_SMOOTH_L1_ROWS && !d->roww)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: SMOOTH_L1_ROWS needs roww");
    if ((kind == SNVC_LOSS_SMOOTH_L1_MASKED || kind == SNVC_LOSS_SMOOTH_L1_ROWS) && !(d->p0 > 0.0f))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: beta (p0) must be positive");
    if (!d->fin) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss: null fin");
    plan->K = kKindK[kind];
    bool vec = d->cols % 4 == 0 && aligned16(d->a) && aligned16(d->b) && (!d->ga || aligned16(d->ga));
    if (d->c) vec = vec && (kind == SNVC_LOSS_SMOOTH_L1_MASKED ? aligned4(d->c) : aligned16(d->c));
    plan->vec = vec;
    const int64_t tile = (int64_t)kThreads * kIters * (vec ? 4 : 1);
    plan->nbx = d->cols > 0 ? ceil_div(d->cols, tile) : 0;
    if (plan->nbx > INT32_MAX) {
        set_error("%s: too many elements in a row", what);
        return SNVC_ERR_UNSUPPORTED;
    }
    return SNVC_OK;
}

EwArgs ew_args(const snvc_loss_desc *d) {
    EwArgs g{};
    g.a = d->a; g.b = d->b; g.roww = d->roww; g.c = d->c;
    g.fin = d->fin; g.gout = d->gout; g.ga = d->ga;
    g.cols = d->cols; g.group = d->group; g.p0 = d->p0; g.p1 = d->p1; g.flags = d->flags;
    return g;
}

template <class OP, bool BWD>
void launch_ew(const EwArgs &g, const EwPlan &plan, int64_t rows, float *partials, hipStream_t st) {
    const dim3 grid((unsigned)plan.nbx, (unsigned)rows);
    if (plan.vec) ew_kernel<OP, 4, BWD><<<grid, kThreads, 0, st>>>(g, partials);
    else ew_kernel<OP, 1, BWD><<<grid, kThreads, 0, st>>>(g, partials);
}

template <bool BWD>
void dispatch_ew(int kind, const EwArgs &g, const EwPlan &plan, int64_t rows, float *partials, hipStream_t st) {
    switch (kind) {
    case SNVC_LOSS_MSE_ROWS: launch_ew<OpMseRows, BWD>(g, plan, rows, partials, st); break;
    case SNVC_LOSS_MSE_POSNEG: launch_ew<OpMsePosNeg, BWD>(g, plan, rows, partials, st); break;
    case SNVC_LOSS_OCCUPANCY: launch_ew<OpOccupancy, BWD>(g, plan, rows, partials, st); break;
    case SNVC_LOSS_OFFSET: launch_ew<OpOffset, BWD>(g, plan, rows, partials, st); break;
    case SNVC_LOSS_SMOOTH_L1_MASKED: launch_ew<OpSmoothL1Masked, BWD>(g, plan, rows, partials, st); break;
    case SNVC_LOSS_SIGMOID_FOCAL: launch_ew<OpSigmoidFocal, BWD>(g, plan, rows, partials, st); break;
    default: launch_ew<OpSmoothL1Rows, BWD>(g, plan, rows, partials, st); break;
    }
}

inline bool wdist_vec(const void *a, const void *b, const void *c, const void *m, const void *e, const void *f, const void *h,
                      int64_t HW) {
    return HW % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(c) && aligned4(m) && (!e || aligned16(e)) && (!f || aligned16(f)) &&
           (!h || aligned16(h));
}

int wdist_check(const void *prob, const void *off, const void *target, const void *mask, const void *levels, int64_t B, int64_t D,
                int64_t HW, const char *what) {
    if (B < 0 || D < 0 || HW < 0) {
        set_error("%s: negative size", what);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (B * D * HW > 0 && (!prob || !off || !target || !mask || !levels)) {
        set_error("%s: null pointer", what);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (B > 65535 || D > INT32_MAX || ceil_div(HW, (int64_t)kThreads) > INT32_MAX) {
        set_error("%s: B > 65535 or a dimension beyond the launch grid", what);
        return SNVC_ERR_UNSUPPORTED;
    }
    return SNVC_OK;
}

}  // namespace
}  // namespace snvc

using namespace snvc;

extern "C" {

int snvc_loss_abi_version(void) { return 1; }

int64_t snvc_loss_partials_count(const snvc_loss_desc *desc) {
    EwPlan plan{};
    snvc_loss_desc d;
    if (!desc) return -1;
    d = *desc;
    static double dummy;
    if (!d.fin) d.fin = &dummy;               // the count does not depend on it
    if (plan_elementwise(&d, "snvc_loss_partials_count", &plan) != SNVC_OK) return -1;
    const int64_t n = plan.nbx * d.rows * plan.K;
    return n > 0 ? n : 1;
}

int snvc_loss_forward(const snvc_loss_desc *d, void *stream) {
    EwPlan plan{};
    const int rc = plan_elementwise(d, "snvc_loss_forward", &plan);
    if (rc != SNVC_OK) return rc;
    if (!d->partials || !d->loss || !d->flag) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_forward: null partials, loss or flag");
    hipStream_t st = as_stream(stream);
    if (plan.nbx > 0) {
        dispatch_ew<false>(d->kind, ew_args(d), plan, d->rows, d->partials, st);
        const int lrc = check_launch("loss forward kernel");
        if (lrc != SNVC_OK) return lrc;
    }
    finalize_kernel<<<1, kThreads, 0, st>>>(d->kind, d->flags, d->partials, plan.nbx * d->rows, plan.K, plan.nbx, d->rows, d->cols,
                                            d->group, d->fin, d->loss, d->flag);
    return check_launch("loss finalize_kernel");
}

int snvc_loss_backward(const snvc_loss_desc *d, void *stream) {
    EwPlan plan{};
    const int rc = plan_elementwise(d, "snvc_loss_backward", &plan);
    if (rc != SNVC_OK) return rc;
    if (!d->gout || (d->cols > 0 && !d->ga)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_backward: null gout or ga");
    if (plan.nbx == 0) return SNVC_OK;
    dispatch_ew<true>(d->kind, ew_args(d), plan, d->rows, nullptr, as_stream(stream));
    return check_launch("loss backward kernel");
}

int64_t snvc_loss_wdist_partials_count(int64_t B, int64_t D, int64_t HW, int per_pixel) {
    if (B < 0 || D < 0 || HW < 0) return -1;
    const int64_t chunks = per_pixel ? 1 : ceil_div(D, (int64_t)kWdPlanes);
    const int64_t n = B * chunks * ceil_div(HW, (int64_t)kThreads) * 2;       // the scalar form's grid (the float4 form needs less)
    return n > 0 ? n : 1;
}

int snvc_loss_wdist_forward(const float *prob, const float *off, const float *target, const uint8_t *mask, const float *levels,
                            int64_t B, int64_t D, int64_t HW, float *pixel_loss, float *partials, double *fin, float *loss,
                            void *stream) {
    const int rc = wdist_check(prob, off, target, mask, levels, B, D, HW, "snvc_loss_wdist_forward");
    if (rc != SNVC_OK) return rc;
    if (!partials || !fin || !loss) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_wdist_forward: null partials, fin or loss");
    hipStream_t st = as_stream(stream);
    int64_t blocks = 0;
    if (B * D * HW > 0) {
        const bool vec = wdist_vec(prob, off, target, mask, pixel_loss, nullptr, nullptr, HW);
        const int planes = pixel_loss ? (int)D : kWdPlanes;
        const dim3 grid((unsigned)ceil_div(HW, (int64_t)kThreads * (vec ? 4 : 1)), (unsigned)ceil_div(D, (int64_t)planes), (unsigned)B);
        if (grid.y > 65535) return fail(SNVC_ERR_UNSUPPORTED, "snvc_loss_wdist_forward: D too large");
        if (vec)
            wdist_kernel<4, false><<<grid, kThreads, 0, st>>>(prob, off, target, mask, levels, D, HW, planes, pixel_loss, partials, nullptr,
                                                               nullptr, nullptr, nullptr, nullptr);
        else
            wdist_kernel<1, false><<<grid, kThreads, 0, st>>>(prob, off, target, mask, levels, D, HW, planes, pixel_loss, partials, nullptr,
                                                               nullptr, nullptr, nullptr, nullptr);
        const int lrc = check_launch("wdist_kernel");
        if (lrc != SNVC_OK) return lrc;
        blocks = (int64_t)grid.x * grid.y * grid.z;
    }
    finalize_kernel<<<1, kThreads, 0, st>>>(FIN_MEAN_NAN, 0, partials, blocks, 2, 0, 1, 0, 1, fin, loss, nullptr);
    return check_launch("loss finalize_kernel");
}

int snvc_loss_wdist_backward(const float *prob, const float *off, const float *target, const uint8_t *mask, const float *levels,
                             int64_t B, int64_t D, int64_t HW, const double *fin, const float *gout, const float *gpix, float *gprob,
                             float *goff, void *stream) {
    const int rc = wdist_check(prob, off, target, mask, levels, B, D, HW, "snvc_loss_wdist_backward");
    if (rc != SNVC_OK) return rc;
    if (!gpix && (!fin || !gout)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_wdist_backward: needs gpix, or fin and gout");
    if (B * D * HW == 0 || (!gprob && !goff)) return SNVC_OK;
    const bool vec = wdist_vec(prob, off, target, mask, gpix, gprob, goff, HW);
    const dim3 grid((unsigned)ceil_div(HW, (int64_t)kThreads * (vec ? 4 : 1)), (unsigned)ceil_div(D, (int64_t)kWdPlanes), (unsigned)B);
    if (grid.y > 65535) return fail(SNVC_ERR_UNSUPPORTED, "snvc_loss_wdist_backward: D too large");
    hipStream_t st = as_stream(stream);
    if (vec)
        wdist_kernel<4, true><<<grid, kThreads, 0, st>>>(prob, off, target, mask, levels, D, HW, kWdPlanes, nullptr, nullptr, fin, gout, gpix,
                                                          gprob, goff);
    else
        wdist_kernel<1, true><<<grid, kThreads, 0, st>>>(prob, off, target, mask, levels, D, HW, kWdPlanes, nullptr, nullptr, fin, gout, gpix,
                                                          gprob, goff);
    return check_launch("wdist_kernel (backward)");
}

int64_t snvc_loss_depth_regression_partials_count(int64_t B, int64_t HW) {
    if (B < 0 || HW < 0) return -1;
    const int64_t n = B * ceil_div(HW, (int64_t)64) * 2;
    return n > 0 ? n : 1;
}

static int depth_regression_check(const void *cost, const void *levels, const void *gt, int64_t B, int64_t D, int64_t HW,
                                  const char *what) {
    if (B < 0 || D < 1 || HW < 0) {
        set_error("%s: needs B, HW >= 0 and D >= 1", what);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (B * HW > 0 && (!cost || !levels || !gt)) {
        set_error("%s: null pointer", what);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (B > 65535 || D > INT32_MAX / 2 || ceil_div(HW, (int64_t)64) > INT32_MAX) {
        set_error("%s: B > 65535 or a dimension beyond the launch grid", what);
        return SNVC_ERR_UNSUPPORTED;
    }
    return SNVC_OK;
}

int snvc_loss_depth_regression_forward(const float *cost, const float *levels, const float *gt, int64_t B, int64_t D, int64_t HW,
                                       float *partials, double *fin, float *loss, void *stream) {
    const int rc = depth_regression_check(cost, levels, gt, B, D, HW, "snvc_loss_depth_regression_forward");
    if (rc != SNVC_OK) return rc;
    if (!partials || !fin || !loss) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_depth_regression_forward: null partials, fin or loss");
    hipStream_t st = as_stream(stream);
    int64_t blocks = 0;
    if (B * HW > 0) {
        const int per = (int)ceil_div(D, (int64_t)kDrSlices);
        const dim3 grid((unsigned)ceil_div(HW, (int64_t)64), (unsigned)B);
        if (per <= kDrCache)
            depth_regression_kernel<true, false><<<grid, kDrThreads, 0, st>>>(cost, levels, gt, D, HW, per, partials, nullptr, nullptr, nullptr);
        else
            depth_regression_kernel<false, false><<<grid, kDrThreads, 0, st>>>(cost, levels, gt, D, HW, per, partials, nullptr, nullptr, nullptr);
        const int lrc = check_launch("depth_regression_kernel");
        if (lrc != SNVC_OK) return lrc;
        blocks = (int64_t)grid.x * grid.y;
    }
    finalize_kernel<<<1, kThreads, 0, st>>>(FIN_MEAN_ZERO, 0, partials, blocks, 2, 0, 1, 0, 1, fin, loss, nullptr);
    return check_launch("loss finalize_kernel");
}

int snvc_loss_depth_regression_backward(const float *cost, const float *levels, const float *gt, int64_t B, int64_t D, int64_t HW,
                                        const double *fin, const float *gout, float *gcost, void *stream) {
    const int rc = depth_regression_check(cost, levels, gt, B, D, HW, "snvc_loss_depth_regression_backward");
    if (rc != SNVC_OK) return rc;
    if (!fin || !gout || (B * HW > 0 && !gcost)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_depth_regression_backward: null fin, gout or gcost");
    if (B * HW == 0) return SNVC_OK;
    const int per = (int)ceil_div(D, (int64_t)kDrSlices);
    const dim3 grid((unsigned)ceil_div(HW, (int64_t)64), (unsigned)B);
    hipStream_t st = as_stream(stream);
    if (per <= kDrCache)
        depth_regression_kernel<true, true><<<grid, kDrThreads, 0, st>>>(cost, levels, gt, D, HW, per, nullptr, fin, gout, gcost);
    else
        depth_regression_kernel<false, true><<<grid, kDrThreads, 0, st>>>(cost, levels, gt, D, HW, per, nullptr, fin, gout, gcost);
    return check_launch("depth_regression_kernel (backward)");
}

int snvc_loss_disparity_regression_backward(const float *gy, const float *depth, float *gx, int64_t N, int64_t D, int64_t HW,
                                            void *stream) {
    if (N < 0 || D < 0 || HW < 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_disparity_regression_backward: negative size");
    if (N * D * HW == 0) return SNVC_OK;
    if (!gy || !depth || !gx) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_loss_disparity_regression_backward: null pointer");
    if (N > 65535 || D > 65535) return fail(SNVC_ERR_UNSUPPORTED, "snvc_loss_disparity_regression_backward: N or D > 65535");
    const bool vec = HW % 4 == 0 && aligned16(gy) && aligned16(gx);
    const dim3 grid((unsigned)ceil_div(HW, (int64_t)kThreads * (vec ? 4 : 1)), (unsigned)D, (unsigned)N);
    hipStream_t st = as_stream(stream);
    if (vec) disparity_regression_bwd_kernel<4><<<grid, kThreads, 0, st>>>(gy, depth, gx, D, HW);
    else disparity_regression_bwd_kernel<1><<<grid, kThreads, 0, st>>>(gy, depth, gx, D, HW);
    return check_launch("disparity_regression_bwd_kernel");
}

}  // extern "C"
