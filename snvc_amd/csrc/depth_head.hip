// The depth read-out and the pseudo-LiDAR projection (include/snvc_depth.h).
//
//   readout_fwd_kernel    a workgroup owns an 8 x 64 tile of output pixels.  The tile's low-resolution footprint (for x4: 4 x 18
//                         columns) is staged in LDS, as many planes at a time as fit in 32 KiB (113 at x4; the walk goes on
//                         from chunk to chunk); lane l of wave w owns the pixels (row w + 4 k, column l), k = 0, 1, and walks
//                         d_out with an online softmax.  A pixel keeps the bilinear values of its two current planes: a step
//                         of d_out that stays between the same planes reads no LDS, one that advances by a plane reads four
//                         words.  The lanes of a wave read consecutive or equal LDS words (a broadcast).  32 KiB and not the
//                         whole depth: the kernel is bound by latency, and five resident workgroups per CU beat two.
//   readout_bwd_kernel    gather form.  A workgroup owns 4 x 16 low-resolution columns and a range of planes; lane l owns column
//                         l, wave w a quarter of the planes.  A thread visits the output pixels that touch its column in
//                         row-major order, recomputes U along d_out from the restaged footprint, p from the forward's (m, z),
//                         and adds its share into its own accumulators: one owner per element of d cost, one fixed order.
//   points_kernel         one pixel per thread.
//   points_count / points_scan / points_write    the compaction: valid pixels per block of 256, an exclusive scan of the
//                         blocks per sample, then every block writes its points behind its offset in pixel order.
#include <cmath>

#include "common.hpp"
#include "snvc_depth.h"

namespace snvc {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / kWave;
constexpr int kTileH = 8, kTileW = 64, kRowsPerLane = kTileH / kWaves;       // forward: output pixels per workgroup
constexpr int kColsH = 4, kColsW = 16, kCols = kColsH * kColsW;              // backward: low-resolution columns per workgroup
constexpr int kFwdLdsWords = 8192, kBwdLdsWords = 8192;                      // 32 KiB: five workgroups per CU
constexpr int kBwdFootprint = (kColsH + 2) * (kColsW + 2);                   // columns + one of halo on every side
constexpr int kBlock = SNVC_DEPTH_POINTS_BLOCK;

// One axis of F.interpolate's coordinate rule; scale is computed on the host in float32, as torch does.
struct Axis {
    float scale;
    int in, out, align;
};

inline Axis make_axis(int64_t in, int64_t out, int align) {
    Axis a;
    a.in = (int)in;
    a.out = (int)out;
    a.align = align;
    if (align) a.scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.0f;
    else a.scale = (float)in / (float)out;
    return a;
}

// i0 <= i1 < a.in and t for output index o.  Nothing is contracted, so every caller gets the same bits: the footprint of
// a tile (taken from its corner pixels) then holds every lane's i0 and i1, both being monotone in o.
__device__ __forceinline__ void coord(const Axis a, int o, int &i0, int &i1, float &t) {
#pragma clang fp contract(off)
    const float src = a.align ? a.scale * (float)o : fmaxf(a.scale * ((float)o + 0.5f) - 0.5f, 0.0f);
    i0 = min((int)src, a.in - 1);
    i1 = min(i0 + 1, a.in - 1);
    t = src - (float)i0;
}

// The smallest o in [0, a.out] whose i1 (upper) or i0 (!upper) is >= p; a.out when there is none.
__device__ int first_reaching(const Axis a, int p, bool upper) {
    if (p <= 0) return 0;
    if (p > a.in - 1) return a.out;
    int o = a.scale > 0.0f ? (int)fminf((float)(p - 1) / a.scale, (float)a.out) : 0;
    o = max(0, min(o, a.out));
    int i0, i1;
    float t;
    while (o < a.out) {
        coord(a, o, i0, i1, t);
        if ((upper ? i1 : i0) >= p) break;
        ++o;
    }
    while (o > 0) {
        coord(a, o - 1, i0, i1, t);
        if ((upper ? i1 : i0) < p) break;
        --o;
    }
    return o;
}

// Planes [0, pn) of a footprint of fh x fw words into lds[p][fh][fw]; src points at the footprint's first word of its first
// plane.  With a footprint of fewer words than threads, groups of threads take a plane each and a thread keeps its word.
__device__ __forceinline__ void stage(float *lds, const float *__restrict__ src, int pn, int fh, int fw, int W, int64_t HW) {
    const int wpp = fh * fw;
    const int groups = wpp < kThreads ? kThreads / wpp : 1;
    int sub = 0, e = threadIdx.x, step = kThreads;
    if (groups > 1) {
        sub = threadIdx.x / wpp;
        e = threadIdx.x - sub * wpp;
        step = wpp;
        if (sub >= groups) return;
    }
    for (; e < wpp; e += step) {
        const int r = e / fw, c = e - r * fw;
        const float *s = src + (int64_t)r * W + c;
#pragma unroll 8
        for (int p = sub; p < pn; p += groups) lds[p * wpp + e] = s[(int64_t)p * HW];
    }
}

// The bilinear value of one staged plane: o00 .. o11 are the word offsets of the pixel's four neighbours in the footprint.
__device__ __forceinline__ float bilinear(const float *plane, int o00, int o01, int o10, int o11, float tx, float ty) {
    const float a = plane[o00], b = plane[o01], c = plane[o10], d = plane[o11];
    const float top = a + tx * (b - a), bot = c + tx * (d - c);
    return top + ty * (bot - top);
}

// ---------------------------------------------------------------------------------------------------- forward
__global__ void __launch_bounds__(kThreads)
readout_fwd_kernel(const float *__restrict__ cost, const float *__restrict__ levels, float *__restrict__ depth,
                   float *__restrict__ conf, float *__restrict__ mo, float *__restrict__ zo, int D, Axis ad, Axis ay, Axis ax) {
    extern __shared__ float lds[];
    const int H = ay.in, W = ax.in, Ho = ay.out, Wo = ax.out, Do = ad.out;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int oy0 = blockIdx.y * kTileH, ox0 = blockIdx.x * kTileW, n = blockIdx.z;
    const int64_t HW = (int64_t)H * W;
    // the footprint: from the first pixel's i0 to the last pixel's i1, per axis
    int lo_y, hi_y, lo_x, hi_x, unused;
    float tu;
    coord(ay, oy0, lo_y, unused, tu);
    coord(ay, min(oy0 + kTileH, Ho) - 1, unused, hi_y, tu);
    coord(ax, ox0, lo_x, unused, tu);
    coord(ax, min(ox0 + kTileW, Wo) - 1, unused, hi_x, tu);
    const int fh = hi_y - lo_y + 1, fw = hi_x - lo_x + 1, wpp = fh * fw;
    const int chunk = kFwdLdsWords / wpp;       // >= 2: the host admits up-sampling only, so wpp <= 10 * 66
    const float *src = cost + (int64_t)n * D * HW + (int64_t)lo_y * W + lo_x;

    // this lane's pixels: column x, rows y[k]; pixels past the edge compute the edge pixel and store nothing
    const int x = min(ox0 + lane, Wo - 1);
    int x0, x1;
    float tx;
    coord(ax, x, x0, x1, tx);
    x0 -= lo_x;
    x1 -= lo_x;
    int r0[kRowsPerLane], r1[kRowsPerLane];
    float ty[kRowsPerLane], m[kRowsPerLane], z[kRowsPerLane], s[kRowsPerLane], va[kRowsPerLane], vb[kRowsPerLane];
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) {
        const int y = min(oy0 + wave + kWaves * k, Ho - 1);
        int y0, y1;
        coord(ay, y, y0, y1, ty[k]);
        r0[k] = (y0 - lo_y) * fw;
        r1[k] = (y1 - lo_y) * fw;
        m[k] = -INFINITY;
        z[k] = s[k] = va[k] = vb[k] = 0.0f;
    }
    int pa = -1, pb = -1;        // the planes va and vb hold
    int d = 0;
    while (d < Do) {
        int i0, i1;
        float t;
        coord(ad, d, i0, i1, t);
        const int plo = i0, pn = min(chunk, D - plo);
        __syncthreads();         // the previous chunk has been read
        stage(lds, src + (int64_t)plo * HW, pn, fh, fw, W, HW);
        __syncthreads();
        for (; d < Do; ++d) {
            coord(ad, d, i0, i1, t);
            if (i1 >= plo + pn) break;
            const float lev = levels[d];
            const float *p0 = lds + (i0 - plo) * wpp, *p1 = lds + (i1 - plo) * wpp;
            const bool new_a = i0 != pa, a_from_b = i0 == pb, new_b = i1 != pb, b_from_a = i1 == i0;
#pragma unroll
            for (int k = 0; k < kRowsPerLane; ++k) {
                if (new_a) va[k] = a_from_b ? vb[k] : bilinear(p0, r0[k] + x0, r0[k] + x1, r1[k] + x0, r1[k] + x1, tx, ty[k]);
                if (new_b) vb[k] = b_from_a ? va[k] : bilinear(p1, r0[k] + x0, r0[k] + x1, r1[k] + x0, r1[k] + x1, tx, ty[k]);
                const float u = va[k] + t * (vb[k] - va[k]);
                const float e = __expf(-fabsf(u - m[k]));
                if (u > m[k]) {          // the running maximum moves: rescale what has been summed
                    z[k] = z[k] * e + 1.0f;
                    s[k] = s[k] * e + lev;
                    m[k] = u;
                } else {
                    z[k] += e;
                    s[k] += e * lev;
                }
            }
            pa = i0;
            pb = i1;
        }
    }
#pragma unroll
    for (int k = 0; k < kRowsPerLane; ++k) {
        const int y = oy0 + wave + kWaves * k;
        if (y < Ho && ox0 + lane < Wo) {
            const int64_t at = ((int64_t)n * Ho + y) * Wo + ox0 + lane;
            depth[at] = s[k] / z[k];
            if (conf) conf[at] = 1.0f / z[k];
            if (mo) mo[at] = m[k];
            if (zo) zo[at] = z[k];
        }
    }
}

// ---------------------------------------------------------------------------------------------------- backward
__global__ void __launch_bounds__(kThreads)
readout_bwd_kernel(const float *__restrict__ cost, const float *__restrict__ levels, const float *__restrict__ depth,
                   const float *__restrict__ mi, const float *__restrict__ zi, const float *__restrict__ gy,
                   float *__restrict__ dcost, int D, int planes_owned, int chunks, Axis ad, Axis ay, Axis ax) {
    extern __shared__ float lds[];
    const int H = ay.in, W = ax.in, Ho = ay.out, Wo = ax.out;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = blockIdx.z / chunks, ch = blockIdx.z - n * chunks;
    const int row0 = blockIdx.y * kColsH, col0 = blockIdx.x * kColsW;
    const int r = row0 + (lane >> 4), c = col0 + (lane & 15);
    const int64_t HW = (int64_t)H * W;
    // the planes this workgroup owns, [a, b), and this wave's quarter of them, [ak, bk)
    const int a = ch * planes_owned, b = min(a + planes_owned, D);
    const int quarter = (b - a + kWaves - 1) / kWaves, ak = a + wave * quarter, bk = min(ak + quarter, b);
    float *acc = lds + (planes_owned + 2) * kBwdFootprint;       // [planes_owned][kCols]
    for (int p = ak; p < bk; ++p) acc[(p - a) * kCols + lane] = 0.0f;

    // the output pixels that touch the tile's columns, [ya, yb) x [xa, xb), and the footprint they read
    const int ya_t = first_reaching(ay, row0, true), yb_t = first_reaching(ay, min(row0 + kColsH, H), false);
    const int xa_t = first_reaching(ax, col0, true), xb_t = first_reaching(ax, min(col0 + kColsW, W), false);
    const bool any = ya_t < yb_t && xa_t < xb_t;
    int lo_y = 0, lo_x = 0, fw = 0;
    const int plo = max(a - 1, 0), phi = min(b, D - 1);
    if (any) {
        int hi_y, hi_x, unused;
        float tu;
        coord(ay, ya_t, lo_y, unused, tu);
        coord(ay, yb_t - 1, unused, hi_y, tu);
        coord(ax, xa_t, lo_x, unused, tu);
        coord(ax, xb_t - 1, unused, hi_x, tu);
        const int fh = hi_y - lo_y + 1;          // <= kColsH + 2: a touching pixel's i0 is its column's row or the one before
        fw = hi_x - lo_x + 1;
        stage(lds, cost + ((int64_t)n * D + plo) * HW + (int64_t)lo_y * W + lo_x, phi - plo + 1, fh, fw, W, HW);
        __syncthreads();
        if (r < H && c < W && ak < bk) {
            const int wpp = fh * fw;
            const int ya = first_reaching(ay, r, true), yb = first_reaching(ay, r + 1, false);
            const int xa = first_reaching(ax, c, true), xb = first_reaching(ax, c + 1, false);
            const int da = first_reaching(ad, ak, true), db = first_reaching(ad, bk, false);
            for (int y = ya; y < yb; ++y) {
                int y0, y1;
                float ty;
                coord(ay, y, y0, y1, ty);
                const float wy = (y0 == r ? 1.0f - ty : 0.0f) + (y1 == r ? ty : 0.0f);
                const int o0 = (y0 - lo_y) * fw - lo_x, o1 = (y1 - lo_y) * fw - lo_x;
                for (int x = xa; x < xb; ++x) {
                    int x0, x1;
                    float tx;
                    coord(ax, x, x0, x1, tx);
                    const float wx = (x0 == c ? 1.0f - tx : 0.0f) + (x1 == c ? tx : 0.0f);
                    const int64_t at = ((int64_t)n * Ho + y) * Wo + x;
                    const float dep = depth[at], mx = mi[at], coef = gy[at] * (wy * wx) / zi[at];
                    int pa = -1, pb = -1, qa = -1;       // the planes of va, vb; the plane of a0 (a1 is the next one's)
                    float va = 0.0f, vb = 0.0f, a0 = 0.0f, a1 = 0.0f;
                    auto flush = [&](int p, float v) {
                        if (p >= ak && p < bk) acc[(p - a) * kCols + lane] += v;
                    };
                    for (int d = da; d < db; ++d) {
                        int i0, i1;
                        float t;
                        coord(ad, d, i0, i1, t);
                        if (i0 != pa) va = i0 == pb ? vb : bilinear(lds + (i0 - plo) * wpp, o0 + x0, o0 + x1, o1 + x0, o1 + x1, tx, ty);
                        if (i1 != pb) vb = i1 == i0 ? va : bilinear(lds + (i1 - plo) * wpp, o0 + x0, o0 + x1, o1 + x0, o1 + x1, tx, ty);
                        pa = i0;
                        pb = i1;
                        const float u = va + t * (vb - va);
                        const float g = coef * __expf(u - mx) * (levels[d] - dep);      // wy wx dU[d]
                        if (i0 != qa) {
                            flush(qa, a0);
                            if (i0 == qa + 1) {
                                a0 = a1;
                            } else {
                                flush(qa + 1, a1);
                                a0 = 0.0f;
                            }
                            a1 = 0.0f;
                            qa = i0;
                        }
                        a0 += g * (1.0f - t);
                        if (i1 == i0) a0 += g * t;
                        else a1 += g * t;
                    }
                    flush(qa, a0);
                    flush(qa + 1, a1);
                }
            }
        }
    }
    if (r < H && c < W)
        for (int p = ak; p < bk; ++p) dcost[((int64_t)n * D + p) * HW + (int64_t)r * W + c] = acc[(p - a) * kCols + lane];
}

// ---------------------------------------------------------------------------------------------------- points
struct PointArgs {
    float min_conf, z_lo, z_hi, origin_u, origin_v, stride_u, stride_v;
    int p_per_sample, H, W;
};

__device__ __forceinline__ bool point_valid(const float *__restrict__ depth, const float *__restrict__ conf, const PointArgs q,
                                            int64_t at) {
    const float z = depth[at];
    bool ok = isfinite(z) && z >= q.z_lo && z < q.z_hi;
    if (conf) ok = ok && conf[at] >= q.min_conf;
    return ok;
}

// project_image_to_rect in float32, one rounding per operation, in the reference's order.
__device__ __forceinline__ void project(const float *__restrict__ P, const PointArgs q, int n, int i, int j, float z, float &x,
                                        float &y) {
#pragma clang fp contract(off)
    const float *p = P + (q.p_per_sample ? (int64_t)n * 12 : 0);
    const float c_u = p[2], c_v = p[6], f_u = p[0], f_v = p[5];
    const float b_x = p[3] / (-f_u), b_y = p[7] / (-f_v);
    const float u = q.origin_u + (float)j * q.stride_u, v = q.origin_v + (float)i * q.stride_v;
    x = ((u - c_u) * z) / f_u + b_x;
    y = ((v - c_v) * z) / f_v + b_y;
}

__global__ void __launch_bounds__(kBlock)
points_kernel(const float *__restrict__ depth, const float *__restrict__ P, const float *__restrict__ conf, const PointArgs q,
              float *__restrict__ points, uint8_t *__restrict__ valid) {
    const int hw = q.H * q.W, px = blockIdx.x * kBlock + threadIdx.x, n = blockIdx.y;
    if (px >= hw) return;
    const int64_t at = (int64_t)n * hw + px;
    const bool ok = point_valid(depth, conf, q, at);
    float x = 0.0f, y = 0.0f, z = 0.0f;
    if (ok) {
        z = depth[at];
        project(P, q, n, px / q.W, px % q.W, z, x, y);
    }
    points[at * 3] = x;
    points[at * 3 + 1] = y;
    points[at * 3 + 2] = z;
    valid[at] = ok ? 1 : 0;
}

__global__ void __launch_bounds__(kBlock)
points_count_kernel(const float *__restrict__ depth, const float *__restrict__ conf, const PointArgs q, int *__restrict__ block_count) {
    __shared__ int waves[kBlock / kWave];
    const int hw = q.H * q.W, px = blockIdx.x * kBlock + threadIdx.x, n = blockIdx.y;
    const bool ok = px < hw && point_valid(depth, conf, q, (int64_t)n * hw + px);
    const unsigned long long mask = __ballot(ok);
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < kBlock / kWave; ++w) s += waves[w];
        block_count[(int64_t)n * gridDim.x + blockIdx.x] = s;
    }
}

// One workgroup per sample: block_count [blocks] becomes its exclusive scan in place; counts[n] = the total.
__global__ void __launch_bounds__(kBlock)
points_scan_kernel(int *__restrict__ block_count, int *__restrict__ counts, int blocks) {
    __shared__ int buf[kBlock];
    int *row = block_count + (int64_t)blockIdx.x * blocks;
    int carry = 0;
    for (int b0 = 0; b0 < blocks; b0 += kBlock) {
        const int b = b0 + threadIdx.x;
        const int mine = b < blocks ? row[b] : 0;
        buf[threadIdx.x] = mine;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {         // inclusive scan of buf
            const int add = threadIdx.x >= off ? buf[threadIdx.x - off] : 0;
            __syncthreads();
            buf[threadIdx.x] += add;
            __syncthreads();
        }
        if (b < blocks) row[b] = carry + buf[threadIdx.x] - mine;
        carry += buf[kBlock - 1];
        __syncthreads();         // buf is read before the next round overwrites it
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kBlock)
points_write_kernel(const float *__restrict__ depth, const float *__restrict__ P, const float *__restrict__ conf, const PointArgs q,
                    const int *__restrict__ block_offset, const int *__restrict__ counts, float *__restrict__ points) {
    __shared__ int waves[kBlock / kWave];
    const int hw = q.H * q.W, px = blockIdx.x * kBlock + threadIdx.x, n = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t at = (int64_t)n * hw + px;
    const bool ok = px < hw && point_valid(depth, conf, q, at);
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) waves[wave] = __popcll(mask);
    __syncthreads();
    if (ok) {
        int row = block_offset[(int64_t)n * gridDim.x + blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; ++w) row += waves[w];
        const float z = depth[at];
        float x, y;
        project(P, q, n, px / q.W, px % q.W, z, x, y);
        float *o = points + ((int64_t)n * hw + row) * 3;      // row < counts[n]
        o[0] = x;
        o[1] = y;
        o[2] = z;
    }
    if (px < hw && px >= counts[n]) {                         // the tail: rows no valid point lands in
        float *o = points + at * 3;
        o[0] = o[1] = o[2] = 0.0f;
    }
}

// ---------------------------------------------------------------------------------------------------- host checks
int readout_sizes_ok(const char *name, int64_t N, int64_t D, int64_t H, int64_t W, int64_t D_out, int64_t H_out, int64_t W_out,
                     bool *empty) {
    if (N < 0 || D < 0 || H < 0 || W < 0 || D_out < 0 || H_out < 0 || W_out < 0) {
        set_error("%s: negative extent", name);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    *empty = N == 0 || H_out == 0 || W_out == 0;
    if (*empty) return SNVC_OK;
    if (D < 1 || H < 1 || W < 1 || D_out < 1) {
        set_error("%s: an output from an empty cost volume or from no depth levels", name);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (D > SNVC_DEPTH_MAX_PLANES || D_out > SNVC_DEPTH_MAX_PLANES) {
        set_error("%s: D and D_out must be at most %d", name, (int)SNVC_DEPTH_MAX_PLANES);
        return SNVC_ERR_UNSUPPORTED;
    }
    if (H_out < H || W_out < W) {
        set_error("%s: the output is smaller than the input in H or W (the tiling assumes up-sampling)", name);
        return SNVC_ERR_UNSUPPORTED;
    }
    if (H_out > (1 << 17) || W_out > (1 << 17) || N > 65535) {
        set_error("%s: H_out and W_out must be at most 2^17, N at most 65535", name);
        return SNVC_ERR_UNSUPPORTED;
    }
    return SNVC_OK;
}

int points_args_ok(const char *name, const float *depth, const float *P, const void *out0, const void *out1, int64_t N, int64_t H,
                   int64_t W, bool *empty) {
    if (N < 0 || H < 0 || W < 0) {
        set_error("%s: negative extent", name);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (H * W >= INT32_MAX || N > 65535) {
        set_error("%s: H * W must be below 2^31, N at most 65535", name);
        return SNVC_ERR_UNSUPPORTED;
    }
    *empty = N == 0 || H == 0 || W == 0;
    if (*empty) return SNVC_OK;
    if (!depth || !P || !out0 || !out1) {
        set_error("%s: null pointer", name);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    return SNVC_OK;
}

}  // namespace
}  // namespace snvc

extern "C" {

int snvc_depth_abi_version(void) { return 1; }

int snvc_depth_readout_forward(const float *cost, const float *levels, float *depth, float *conf, float *m, float *z, int64_t N,
                               int64_t D, int64_t H, int64_t W, int64_t D_out, int64_t H_out, int64_t W_out, int align_corners,
                               void *stream) {
    using namespace snvc;
    bool empty = false;
    const int rc = readout_sizes_ok("snvc_depth_readout_forward", N, D, H, W, D_out, H_out, W_out, &empty);
    if (rc != SNVC_OK || empty) return rc;
    if (!cost || !levels || !depth) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_readout_forward: null pointer");
    if (!aligned(4, cost, levels, depth, conf, m, z))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_readout_forward: a pointer is not aligned");
    const dim3 grid((unsigned)ceil_div<int64_t>(W_out, kTileW), (unsigned)ceil_div<int64_t>(H_out, kTileH), (unsigned)N);
    launch_lds<readout_fwd_kernel>(grid, dim3(kThreads), sizeof(float) * kFwdLdsWords, as_stream(stream), cost, levels, depth, conf, m, z,
                                   (int)D, make_axis(D, D_out, align_corners), make_axis(H, H_out, align_corners),
                                   make_axis(W, W_out, align_corners));
    return check_launch("snvc_depth_readout_forward");
}

int snvc_depth_readout_backward(const float *cost, const float *levels, const float *depth, const float *m, const float *z,
                                const float *gy, float *dcost, int64_t N, int64_t D, int64_t H, int64_t W, int64_t D_out,
                                int64_t H_out, int64_t W_out, int align_corners, void *stream) {
    using namespace snvc;
    bool empty = false;
    const int rc = readout_sizes_ok("snvc_depth_readout_backward", N, D, H, W, D_out, H_out, W_out, &empty);
    if (rc != SNVC_OK) return rc;
    if (N == 0 || D == 0 || H == 0 || W == 0) return SNVC_OK;        // no element of d cost
    if (!dcost) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_readout_backward: null pointer");
    if (empty) {                                                      // no output pixel: the gradient is zero
        if (hipMemsetAsync(dcost, 0, sizeof(float) * (size_t)(N * D * H * W), as_stream(stream)) != hipSuccess)
            return fail(SNVC_ERR_HIP, "snvc_depth_readout_backward: hipMemsetAsync failed");
        return SNVC_OK;
    }
    if (!cost || !levels || !depth || !m || !z || !gy) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_readout_backward: null pointer");
    if (!aligned(4, cost, levels, depth, m, z, gy, dcost))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_readout_backward: a pointer is not aligned");
    // planes a workgroup owns: footprint planes (owned + 2 of halo) and one accumulator row per owned plane share the LDS
    const int most = (kBwdLdsWords - 2 * kBwdFootprint) / (kBwdFootprint + kCols);
    const int chunks = (int)ceil_div<int64_t>(D, most);
    const int owned = (int)ceil_div<int64_t>(D, chunks);
    if (N * chunks > 65535) return fail(SNVC_ERR_UNSUPPORTED, "snvc_depth_readout_backward: N times the plane chunks exceeds 65535");
    const dim3 grid((unsigned)ceil_div<int64_t>(W, kColsW), (unsigned)ceil_div<int64_t>(H, kColsH), (unsigned)(N * chunks));
    const size_t bytes = sizeof(float) * ((size_t)(owned + 2) * kBwdFootprint + (size_t)owned * kCols);
    launch_lds<readout_bwd_kernel>(grid, dim3(kThreads), bytes, as_stream(stream), cost, levels, depth, m, z, gy, dcost, (int)D, owned,
                                   chunks, make_axis(D, D_out, align_corners), make_axis(H, H_out, align_corners),
                                   make_axis(W, W_out, align_corners));
    return check_launch("snvc_depth_readout_backward");
}

static snvc::PointArgs point_args(int p_per_sample, float min_conf, float z_lo, float z_hi, float origin_u, float origin_v,
                                  float stride_u, float stride_v, int64_t H, int64_t W) {
    snvc::PointArgs q;
    q.min_conf = min_conf;
    q.z_lo = z_lo;
    q.z_hi = z_hi;
    q.origin_u = origin_u;
    q.origin_v = origin_v;
    q.stride_u = stride_u;
    q.stride_v = stride_v;
    q.p_per_sample = p_per_sample;
    q.H = (int)H;
    q.W = (int)W;
    return q;
}

int snvc_depth_to_points(const float *depth, const float *P, int p_per_sample, const float *conf, float min_conf, float z_lo,
                         float z_hi, float origin_u, float origin_v, float stride_u, float stride_v, float *points, uint8_t *valid,
                         int64_t N, int64_t H, int64_t W, void *stream) {
    using namespace snvc;
    bool empty = false;
    const int rc = points_args_ok("snvc_depth_to_points", depth, P, points, valid, N, H, W, &empty);
    if (rc != SNVC_OK || empty) return rc;
    if (!aligned(4, depth, P, conf, points)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_to_points: a pointer is not aligned");
    const PointArgs q = point_args(p_per_sample, min_conf, z_lo, z_hi, origin_u, origin_v, stride_u, stride_v, H, W);
    points_kernel<<<dim3((unsigned)ceil_div<int64_t>(H * W, kBlock), (unsigned)N), kBlock, 0, as_stream(stream)>>>(depth, P, conf, q,
                                                                                                                 points, valid);
    return check_launch("snvc_depth_to_points");
}

int64_t snvc_depth_points_workspace_bytes(int64_t N, int64_t HW) {
    if (N < 0 || HW < 0 || HW >= INT32_MAX) return -1;
    return N * snvc::ceil_div<int64_t>(HW, snvc::kBlock) * (int64_t)sizeof(int32_t);
}

int snvc_depth_to_points_compact(const float *depth, const float *P, int p_per_sample, const float *conf, float min_conf, float z_lo,
                                 float z_hi, float origin_u, float origin_v, float stride_u, float stride_v, void *workspace,
                                 float *points, int32_t *counts, int64_t N, int64_t H, int64_t W, void *stream) {
    using namespace snvc;
    bool empty = false;
    const int rc = points_args_ok("snvc_depth_to_points_compact", depth, P, points, counts, N, H, W, &empty);
    if (rc != SNVC_OK) return rc;
    if (N == 0) return SNVC_OK;
    if (empty) {                                                      // samples without pixels: every count is zero
        if (!counts) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_to_points_compact: null pointer");
        if (hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)N, as_stream(stream)) != hipSuccess)
            return fail(SNVC_ERR_HIP, "snvc_depth_to_points_compact: hipMemsetAsync failed");
        return SNVC_OK;
    }
    if (!workspace) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_to_points_compact: null pointer");
    if (!aligned(4, depth, P, conf, points, counts) || !aligned(4, static_cast<const char *>(workspace)))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_depth_to_points_compact: a pointer is not aligned");
    const PointArgs q = point_args(p_per_sample, min_conf, z_lo, z_hi, origin_u, origin_v, stride_u, stride_v, H, W);
    const int blocks = (int)ceil_div<int64_t>(H * W, kBlock);
    int *block_count = static_cast<int *>(workspace);
    const dim3 grid((unsigned)blocks, (unsigned)N);
    hipStream_t st = as_stream(stream);
    points_count_kernel<<<grid, kBlock, 0, st>>>(depth, conf, q, block_count);
    points_scan_kernel<<<dim3((unsigned)N), kBlock, 0, st>>>(block_count, counts, blocks);
    points_write_kernel<<<grid, kBlock, 0, st>>>(depth, P, conf, q, block_count, counts, points);
    return check_launch("snvc_depth_to_points_compact");
}

}  // extern "C"
