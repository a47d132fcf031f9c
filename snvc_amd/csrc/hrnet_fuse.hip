// HRNet multi-resolution fusion (include/snvc_hrnet.h) for gfx950.
//
// Reference: snvc/models/hrnet.py HighResolutionModule.forward (:235-252) and the nn.Upsample(mode='nearest') of its
// up paths (:204).  The reference materialises every upsampled term at full resolution and adds them pairwise (one
// full-size write + read per term and per add); here the low-resolution terms are read as they are and one pass
// writes the activated sum.
//
// Both kernels are memory-bound.  Where W is a multiple of 8 and the pointers are 16-byte aligned, a lane owns 8
// consecutive outputs of one row: a factor-1 term is two 16-byte loads, factor 2 one 16-byte load, factor 4 one
// 8-byte load and factor 8 one scalar, so each low-resolution element is read once per output row it feeds.  The
// backward lane owns R rows x 8 columns (R = the largest factor asked for), reads gy and out once and writes the
// masked gradient and every block sum from registers.  Other widths take the same code one element (forward) or one
// R x R block (backward) per lane with scalar accesses.
#include "common.hpp"
#include "snvc_hrnet.h"

namespace snvc {
namespace {

constexpr int kThreads = 256;
constexpr int kMaxTerms = SNVC_HRNET_MAX_TERMS;

struct FuseTerms {
    const float *t[kMaxTerms];   // the non-NULL terms, in order, packed to the front
    int f[kMaxTerms];
    int n;
};

struct FuseGrads {
    float *g1, *g2, *g4, *g8;
};

__device__ inline float act(float v, int relu) { return relu ? (v > 0.f ? v : 0.f) : v; }

// The 8 outputs x0 .. x0 + 7 (x0 a multiple of 8) of one term row of factor f, upsampled.
__device__ inline void load8(const float *row, int f, int64_t x0, float v[8]) {
    if (f == 1) {
        const float4 a = *reinterpret_cast<const float4 *>(row + x0);
        const float4 b = *reinterpret_cast<const float4 *>(row + x0 + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
        v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if (f == 2) {
        const float4 a = *reinterpret_cast<const float4 *>(row + x0 / 2);
        v[0] = v[1] = a.x; v[2] = v[3] = a.y; v[4] = v[5] = a.z; v[6] = v[7] = a.w;
    } else if (f == 4) {
        const float2 a = *reinterpret_cast<const float2 *>(row + x0 / 4);
        v[0] = v[1] = v[2] = v[3] = a.x;
        v[4] = v[5] = v[6] = v[7] = a.y;
    } else {
        const float a = row[x0 / 8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = a;
    }
}

// One lane: V consecutive outputs of one row (V = 8 vectorised, 1 otherwise).  `out` may alias t[0] (factor 1): every
// lane reads its own outputs' term-0 values before it writes them.
template <int V>
__global__ __launch_bounds__(kThreads) void hrnet_fuse_fwd_kernel(FuseTerms T, float *out, int64_t rows, int H, int W, int relu) {
    const int64_t per_row = W / V;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= rows * per_row) return;
    const int64_t r = i / per_row;                  // (n * C + c) * H + y
    const int64_t x0 = (i - r * per_row) * V;
    const int64_t nc = r / H;
    const int y = (int)(r - nc * H);
    float acc[V];
#pragma unroll
    for (int k = 0; k < kMaxTerms; ++k) {
        if (k >= T.n) break;
        const int f = T.f[k];
        const int64_t wk = W / f;
        const float *row = T.t[k] + (nc * (H / f) + y / f) * wk;
        float v[V];
        if constexpr (V == 8) {
            load8(row, f, x0, v);
        } else {
            v[0] = row[x0 / f];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] = k == 0 ? v[e] : __fadd_rn(acc[e], v[e]);
    }
    float *o = out + r * W + x0;
    if constexpr (V == 8) {
        *reinterpret_cast<float4 *>(o) = make_float4(act(acc[0], relu), act(acc[1], relu), act(acc[2], relu), act(acc[3], relu));
        *reinterpret_cast<float4 *>(o + 4) = make_float4(act(acc[4], relu), act(acc[5], relu), act(acc[6], relu), act(acc[7], relu));
    } else {
        o[0] = act(acc[0], relu);
    }
}

// f x f block sums of the R x CW tile g (F <= R, F <= CW), each block row by row, every row left to right.
template <int F, int R, int CW>
__device__ inline void block_sums(const float (&g)[R][CW], float *dst, int64_t nc, int H, int W, int y0, int64_t x0) {
    const int64_t wf = W / F;
#pragma unroll
    for (int br = 0; br < R / F; ++br) {
        float *d = dst + (nc * (H / F) + y0 / F + br) * wf + x0 / F;
#pragma unroll
        for (int bc = 0; bc < CW / F; ++bc) {
            float s = 0.f;
#pragma unroll
            for (int rr = 0; rr < F; ++rr) {
                float rs = g[br * F + rr][bc * F];
#pragma unroll
                for (int cc = 1; cc < F; ++cc) rs = __fadd_rn(rs, g[br * F + rr][bc * F + cc]);
                s = rr == 0 ? rs : __fadd_rn(s, rs);
            }
            d[bc] = s;
        }
    }
}

// One lane: an R x CW tile (CW = 8 vectorised, R otherwise), R = the largest factor whose gradient is asked for.
template <int R, bool kVec>
__global__ __launch_bounds__(kThreads) void hrnet_fuse_bwd_kernel(const float *gy, const float *out, FuseGrads G, int64_t row_blocks,
                                                                   int H, int W, int relu) {
    constexpr int CW = kVec ? 8 : R;
    const int64_t per_row = W / CW;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= row_blocks * per_row) return;
    const int64_t rb = i / per_row;                 // (n * C + c) * (H / R) + y0 / R
    const int64_t x0 = (i - rb * per_row) * CW;
    const int64_t nc = rb / (H / R);
    const int y0 = (int)(rb - nc * (H / R)) * R;
    float g[R][CW];
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int64_t off = (nc * H + y0 + rr) * W + x0;
        float a[CW], b[CW];
        if constexpr (kVec) {
            const float4 a0 = *reinterpret_cast<const float4 *>(gy + off), a1 = *reinterpret_cast<const float4 *>(gy + off + 4);
            a[0] = a0.x; a[1] = a0.y; a[2] = a0.z; a[3] = a0.w; a[4] = a1.x; a[5] = a1.y; a[6] = a1.z; a[7] = a1.w;
            if (relu) {
                const float4 b0 = *reinterpret_cast<const float4 *>(out + off), b1 = *reinterpret_cast<const float4 *>(out + off + 4);
                b[0] = b0.x; b[1] = b0.y; b[2] = b0.z; b[3] = b0.w; b[4] = b1.x; b[5] = b1.y; b[6] = b1.z; b[7] = b1.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < CW; ++c) {
                a[c] = gy[off + c];
                if (relu) b[c] = out[off + c];
            }
        }
#pragma unroll
        for (int c = 0; c < CW; ++c) g[rr][c] = relu ? (b[c] > 0.f ? a[c] : 0.f) : a[c];
        if (G.g1) {
            if constexpr (kVec) {
                *reinterpret_cast<float4 *>(G.g1 + off) = make_float4(g[rr][0], g[rr][1], g[rr][2], g[rr][3]);
                *reinterpret_cast<float4 *>(G.g1 + off + 4) = make_float4(g[rr][4], g[rr][5], g[rr][6], g[rr][7]);
            } else {
#pragma unroll
                for (int c = 0; c < CW; ++c) G.g1[off + c] = g[rr][c];
            }
        }
    }
    if constexpr (R >= 2) if (G.g2) block_sums<2, R, CW>(g, G.g2, nc, H, W, y0, x0);
    if constexpr (R >= 4) if (G.g4) block_sums<4, R, CW>(g, G.g4, nc, H, W, y0, x0);
    if constexpr (R >= 8) if (G.g8) block_sums<8, R, CW>(g, G.g8, nc, H, W, y0, x0);
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline unsigned grid_1d(int64_t n) { return (unsigned)ceil_div<int64_t>(n, kThreads); }
inline bool valid_factor(int f) { return f == 1 || f == 2 || f == 4 || f == 8; }

template <int R>
int launch_bwd(const float *gy, const float *out, const FuseGrads &G, int64_t NC, int H, int W, int relu, hipStream_t st) {
    const bool vec = W % 8 == 0 && aligned16(gy) && (!relu || aligned16(out)) && (!G.g1 || aligned16(G.g1));
    const int64_t row_blocks = NC * (H / R);
    if (vec)
        hrnet_fuse_bwd_kernel<R, true><<<grid_1d(row_blocks * (W / 8)), kThreads, 0, st>>>(gy, out, G, row_blocks, H, W, relu);
    else
        hrnet_fuse_bwd_kernel<R, false><<<grid_1d(row_blocks * (W / R)), kThreads, 0, st>>>(gy, out, G, row_blocks, H, W, relu);
    return check_launch("hrnet_fuse_bwd_kernel");
}

}  // namespace
}  // namespace snvc

using namespace snvc;

extern "C" {

int snvc_hrnet_abi_version(void) { return 1; }

int snvc_hrnet_fuse_forward(const void *const *terms_host, const int32_t *factors_host, const int64_t *extents_host, float *out,
                            int64_t N, int64_t C, int64_t H, int64_t W, int relu, void *stream) {
    if (!terms_host || !factors_host || !extents_host)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_forward: null host array");
    if (!terms_host[0]) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_forward: term 0 must not be NULL");
    if (!out) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_forward: null out");
    if (N < 0 || C < 0 || H < 0 || W < 0 || H > INT32_MAX || W > INT32_MAX)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_forward: bad N / C / H / W");
    FuseTerms T{};
    for (int k = 0; k < kMaxTerms; ++k) {
        if (!terms_host[k]) continue;
        const int f = factors_host[k];
        if (!valid_factor(f)) {
            set_error("snvc_hrnet_fuse_forward: term %d has factor %d; factors are 1, 2, 4 or 8", k, f);
            return SNVC_ERR_INVALID_ARGUMENT;
        }
        const int64_t h = extents_host[2 * k], w = extents_host[2 * k + 1];
        if (h * f != H || w * f != W) {
            set_error("snvc_hrnet_fuse_forward: term %d of extent %lld x %lld upsampled by %d is not the output's %lld x %lld", k,
                      (long long)h, (long long)w, f, (long long)H, (long long)W);
            return SNVC_ERR_INVALID_ARGUMENT;
        }
        if (terms_host[k] == out && (k != 0 || f != 1))
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_forward: out may alias term 0 of factor 1 only");
        T.t[T.n] = static_cast<const float *>(terms_host[k]);
        T.f[T.n] = f;
        ++T.n;
    }
    const int64_t rows = N * C * H;
    if (rows == 0 || W == 0) return SNVC_OK;
    bool vec = W % 8 == 0 && aligned16(out);
    for (int k = 0; k < T.n; ++k) vec = vec && aligned16(T.t[k]);
    hipStream_t st = as_stream(stream);
    if (vec)
        hrnet_fuse_fwd_kernel<8><<<grid_1d(rows * (W / 8)), kThreads, 0, st>>>(T, out, rows, (int)H, (int)W, relu);
    else
        hrnet_fuse_fwd_kernel<1><<<grid_1d(rows * W), kThreads, 0, st>>>(T, out, rows, (int)H, (int)W, relu);
    return check_launch("hrnet_fuse_fwd_kernel");
}

int snvc_hrnet_fuse_backward(const float *gy, const float *out, float *grad1, float *grad2, float *grad4, float *grad8, int64_t N,
                             int64_t C, int64_t H, int64_t W, int relu, void *stream) {
    if (!gy || (relu && !out)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_backward: null gy / out");
    if (N < 0 || C < 0 || H < 0 || W < 0 || H > INT32_MAX || W > INT32_MAX)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_hrnet_fuse_backward: bad N / C / H / W");
    int R = 1;
    float *pooled[3] = {grad2, grad4, grad8};
    for (int k = 0; k < 3; ++k) {
        const int f = 2 << k;
        if (!pooled[k]) continue;
        if (H % f || W % f) {
            set_error("snvc_hrnet_fuse_backward: output %lld x %lld is not a multiple of factor %d", (long long)H, (long long)W, f);
            return SNVC_ERR_INVALID_ARGUMENT;
        }
        R = f;
    }
    if (N * C * H * W == 0 || (!grad1 && R == 1)) return SNVC_OK;
    const FuseGrads G{grad1, grad2, grad4, grad8};
    hipStream_t st = as_stream(stream);
    const int64_t NC = N * C;
    switch (R) {
        case 1: return launch_bwd<1>(gy, out, G, NC, (int)H, (int)W, relu, st);
        case 2: return launch_bwd<2>(gy, out, G, NC, (int)H, (int)W, relu, st);
        case 4: return launch_bwd<4>(gy, out, G, NC, (int)H, (int)W, relu, st);
        default: return launch_bwd<8>(gy, out, G, NC, (int)H, (int)W, relu, st);
    }
}

}  // extern "C"
