// Rotated-box overlap, IoU and NMS (include/snvc_iou3d.h) for gfx950.
//
// Reference: snvc/extension/iou3d_nms/src/iou3d_nms_kernel.cu (kernels), iou3d_nms.cpp (launchers, host greedy pass),
//            iou3d_cpu.cpp (host IoU), iou3d_nms_utils.py (3D IoU, differentiable IoU).
//
// The overlap is the reference's DEFINITION, written from it (see the header): proper crossings of the outlines plus
// the corners strictly inside the other box grown by 1e-2, shoelace area in angular order about the points' mean.
// Differences in the evaluation, none of which changes that definition:
//   - everything is computed relative to box a's centre (fp32 corners at 70 m lose ~4e-6 m in absolute coordinates);
//   - cos/sin, corner offsets, area, height range and volume are computed once per box (a prep pass), not per pair
//     and again inside every inside-test;
//   - points are ordered by one pseudo-angle key each (monotone in atan2), insertion sort, instead of a bubble sort
//     with two atan2 per comparison;
//   - pairs whose bounding circles (of the grown boxes) cannot meet return 0 before any polygon work.
// NMS computes only the upper-triangle mask tiles that the greedy pass reads, and the greedy pass runs on the
// device: only the kept count crosses to the host (in the Python layer, to size its result).
#include "common.hpp"
#include "snvc_iou3d.h"

#include <cmath>
#include <vector>

namespace snvc {
namespace {

constexpr float kMargin = 1e-2f;   // grown half-extent of the inside test (iou3d_nms_kernel.cu check_in_box2d)
constexpr float kEpsBev = 1e-8f;   // iou_bev denominator floor
constexpr float kEps3d = 1e-6f;    // iou3d denominator floor (iou3d_nms_utils.py:85)
constexpr int kMaxPts = 24;        // 16 edge pairs + 8 corners: no configuration can exceed it
constexpr int kTile = 64;          // NMS tile = one wave, one mask word

struct Prep {                      // 80 B per box
    float x, y, c, s;              // centre, cos / sin of the heading
    float hx, hy, area, rad;       // half extents, dx * dy, radius of the grown box's circumcircle
    float ox[4], oy[4];            // corner offsets from the centre, counter-clockwise
    float zlo, zhi, vol, pad;      // z -/+ dz / 2, dx * dy * dz
};

__host__ __device__ inline Prep prep_box(const float *b) {
    Prep p;
    p.x = b[0];
    p.y = b[1];
    p.c = cosf(b[6]);
    p.s = sinf(b[6]);
    p.hx = b[3] / 2;
    p.hy = b[4] / 2;
    p.area = b[3] * b[4];
    const float gx = fabsf(p.hx) + kMargin, gy = fabsf(p.hy) + kMargin;
    p.rad = sqrtf(gx * gx + gy * gy);
    const float sx[4] = {-1.f, 1.f, 1.f, -1.f}, sy[4] = {-1.f, -1.f, 1.f, 1.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float lx = sx[k] * p.hx, ly = sy[k] * p.hy;
        p.ox[k] = lx * p.c - ly * p.s;
        p.oy[k] = lx * p.s + ly * p.c;
    }
    p.zlo = b[2] - b[5] / 2;
    p.zhi = b[2] + b[5] / 2;
    p.vol = b[3] * b[4] * b[5];
    p.pad = 0.f;
    return p;
}

__host__ __device__ inline bool strictly_opposite(float u, float v) { return (u > 0.f && v < 0.f) || (u < 0.f && v > 0.f); }

// Point (px, py), given relative to the box centre, strictly inside the box grown by kMargin.
__host__ __device__ inline bool inside_grown(const Prep &b, float px, float py) {
    const float lx = px * b.c + py * b.s;      // rotate by -heading
    const float ly = -px * b.s + py * b.c;
    return fabsf(lx) < b.hx + kMargin && fabsf(ly) < b.hy + kMargin;
}

// Monotone in atan2(v, u) over [0, 2 pi): values in [0, 4).
__host__ __device__ inline float pseudo_angle(float u, float v) {
    const float a = fabsf(u) + fabsf(v);
    if (a == 0.f) return 0.f;
    const float r = u / a;
    return v >= 0.f ? 1.f - r : 3.f + r;
}

__host__ __device__ inline float bev_overlap(const Prep &A, const Prep &B) {
    const float dx = B.x - A.x, dy = B.y - A.y;
    const float reach = (A.rad + B.rad) * 1.001f + 1e-4f;   // superset of every pair with a crossing or a corner inside
    if (dx * dx + dy * dy > reach * reach) return 0.f;

    float ax[4], ay[4], bx[4], by[4];                       // corners relative to A's centre
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        ax[k] = A.ox[k];
        ay[k] = A.oy[k];
        bx[k] = dx + B.ox[k];
        by[k] = dy + B.oy[k];
    }
    float px[kMaxPts], py[kMaxPts];
    int n = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float p0x = ax[i], p0y = ay[i];
        const float ex = ax[(i + 1) & 3] - p0x, ey = ay[(i + 1) & 3] - p0y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float q0x = bx[j], q0y = by[j];
            const float fx = bx[(j + 1) & 3] - q0x, fy = by[(j + 1) & 3] - q0y;
            const float o1 = ex * (q0y - p0y) - ey * (q0x - p0x);             // side of q0 w.r.t. edge p
            const float o2 = ex * (q0y + fy - p0y) - ey * (q0x + fx - p0x);   // side of q1
            const float o3 = fx * (p0y - q0y) - fy * (p0x - q0x);             // side of p0 w.r.t. edge q
            const float o4 = fx * (p0y + ey - q0y) - fy * (p0x + ex - q0x);   // side of p1
            if (strictly_opposite(o1, o2) && strictly_opposite(o3, o4)) {
                const float t = o3 / (o3 - o4);
                px[n] = p0x + t * ex;
                py[n] = p0y + t * ey;
                ++n;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (inside_grown(A, bx[k], by[k])) {
            px[n] = bx[k];
            py[n] = by[k];
            ++n;
        }
        if (inside_grown(B, ax[k] - dx, ay[k] - dy)) {
            px[n] = ax[k];
            py[n] = ay[k];
            ++n;
        }
    }
    if (n < 3) return 0.f;

    float mx = 0.f, my = 0.f;
    for (int k = 0; k < n; ++k) {
        mx += px[k];
        my += py[k];
    }
    mx /= n;
    my /= n;
    float key[kMaxPts];
    for (int k = 0; k < n; ++k) {                           // one key per point, insertion sort on it
        const float u = px[k] - mx, v = py[k] - my, a = pseudo_angle(u, v);
        int m = k;
        while (m > 0 && key[m - 1] > a) {
            key[m] = key[m - 1];
            px[m] = px[m - 1];
            py[m] = py[m - 1];
            --m;
        }
        key[m] = a;
        px[m] = u;
        py[m] = v;
    }
    float area = px[n - 1] * py[0] - px[0] * py[n - 1];
    for (int k = 0; k + 1 < n; ++k) area += px[k] * py[k + 1] - px[k + 1] * py[k];
    return fabsf(area) * 0.5f;
}

__host__ __device__ inline float iou_bev(const Prep &A, const Prep &B) {
    const float ov = bev_overlap(A, B);
    return ov / fmaxf(A.area + B.area - ov, kEpsBev);
}

__host__ __device__ inline float iou_3d(const Prep &A, const Prep &B) {
    const float ov = bev_overlap(A, B);
    const float h = fmaxf(fminf(A.zhi, B.zhi) - fmaxf(A.zlo, B.zlo), 0.f);
    const float o3 = ov * h;
    return o3 / fmaxf(A.vol + B.vol - o3, kEps3d);
}

template <int WHAT>
__host__ __device__ inline float pair_value(const Prep &A, const Prep &B) {
    if (WHAT == SNVC_IOU3D_OVERLAP) return bev_overlap(A, B);
    if (WHAT == SNVC_IOU3D_IOU_BEV) return iou_bev(A, B);
    return iou_3d(A, B);
}

// Axis-aligned BEV IoU on the raw boxes, heading ignored (iou3d_nms_kernel.cu iou_normal).
__device__ inline float iou_normal(const float *a, const float *b) {
    const float left = fmaxf(a[0] - a[3] / 2, b[0] - b[3] / 2), right = fminf(a[0] + a[3] / 2, b[0] + b[3] / 2);
    const float top = fmaxf(a[1] - a[4] / 2, b[1] - b[4] / 2), bottom = fminf(a[1] + a[4] / 2, b[1] + b[4] / 2);
    const float inter = fmaxf(right - left, 0.f) * fmaxf(bottom - top, 0.f);
    return inter / fmaxf(a[3] * a[4] + b[3] * b[4] - inter, kEpsBev);
}

// ---------------------------------------------------------------------------------------------- pairwise
__global__ __launch_bounds__(256) void iou3d_prep_kernel(const float *__restrict__ boxes, int64_t n, Prep *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = prep_box(boxes + i * 7);
}

// block (64, 4): 64 consecutive columns (coalesced stores) x 4 rows; a 1-D grid of col_tiles x row groups
template <int WHAT>
__global__ __launch_bounds__(256) void iou3d_matrix_kernel(const Prep *__restrict__ pa, int64_t na, const Prep *__restrict__ pb,
                                                           int64_t nb, int64_t col_tiles, float *__restrict__ out) {
    const int64_t bid = blockIdx.x;
    const int64_t j = (bid % col_tiles) * kTile + threadIdx.x;
    const int64_t i = (bid / col_tiles) * 4 + threadIdx.y;
    if (i >= na || j >= nb) return;
    out[i * nb + j] = pair_value<WHAT>(pa[i], pb[j]);
}

template <int WHAT>
__global__ __launch_bounds__(256) void iou3d_onebyone_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t n,
                                                             float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = pair_value<WHAT>(prep_box(a + i * 7), prep_box(b + i * 7));
}

// ---------------------------------------------------------------------------------------------- NMS
// One wave per upper-triangle tile (column tile >= row tile), linear tile index t -> (row r, column c).
// mask [n][nblk]: bit j of word (i, c) <=> iou(box_i, box_{64c + j}) > thresh, only for 64c + j > i.
template <int KIND>
__global__ __launch_bounds__(kTile) void nms_mask_kernel(const float *__restrict__ boxes, const Prep *__restrict__ prep, int n,
                                                         int nblk, float thresh, unsigned long long *__restrict__ mask) {
    const int64_t t = blockIdx.x;
    // tiles before row r: S(r) = r * nblk - r * (r - 1) / 2
    const double b2 = 2.0 * nblk + 1.0;
    int r = (int)((b2 - sqrt(fmax(b2 * b2 - 8.0 * (double)t, 0.0))) * 0.5);
    auto S = [nblk](int64_t rr) { return rr * nblk - rr * (rr - 1) / 2; };
    if (r < 0) r = 0;
    if (r > nblk - 1) r = nblk - 1;
    while (r > 0 && S(r) > t) --r;
    while (r + 1 < nblk && S(r + 1) <= t) ++r;
    const int c = r + (int)(t - S(r));

    const int lane = threadIdx.x;
    const int row_size = min(n - r * kTile, kTile);
    const int col_size = min(n - c * kTile, kTile);
    __shared__ Prep col_prep[kTile];
    __shared__ float col_box[kTile * 7];
    if (lane < col_size) {
        if (KIND == SNVC_NMS_ROTATED) {
            col_prep[lane] = prep[c * kTile + lane];
        } else {
#pragma unroll
            for (int k = 0; k < 7; ++k) col_box[lane * 7 + k] = boxes[(int64_t)(c * kTile + lane) * 7 + k];
        }
    }
    __syncthreads();
    if (lane >= row_size) return;

    const int i = r * kTile + lane;
    const int start = r == c ? lane + 1 : 0;
    unsigned long long bits = 0;
    if (KIND == SNVC_NMS_ROTATED) {
        const Prep me = prep[i];
        for (int j = start; j < col_size; ++j)
            if (iou_bev(me, col_prep[j]) > thresh) bits |= 1ull << j;
    } else {
        float me[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) me[k] = boxes[(int64_t)i * 7 + k];
        for (int j = start; j < col_size; ++j)
            if (iou_normal(me, col_box + j * 7) > thresh) bits |= 1ull << j;
    }
    mask[(int64_t)i * nblk + c] = bits;
}

// One workgroup walks the nblk blocks of 64 boxes in rank order.  remv (LDS) holds the suppressed bits of every
// block.  Per block: wave 0 settles the 64 decisions serially from the diagonal words (the bits of row l only
// concern later rows of the block), writes the kept indices, and then all 16 waves OR the kept rows' words of the
// later blocks into remv.
constexpr int kGreedyThreads = 1024;
constexpr int kMaxBlocks = SNVC_NMS_MAX_BOXES / kTile;

__global__ __launch_bounds__(kGreedyThreads) void nms_greedy_kernel(const unsigned long long *__restrict__ mask, int n, int nblk,
                                                                    int64_t *__restrict__ keep, int32_t *__restrict__ num_keep) {
    __shared__ unsigned long long remv[kMaxBlocks];
    __shared__ unsigned long long s_kept;
    const int tid = threadIdx.x;
    for (int c = tid; c < nblk; c += kGreedyThreads) remv[c] = 0ull;
    __syncthreads();
    int count = 0;                                           // identical in every thread
    for (int b = 0; b < nblk; ++b) {
        const int rows = min(n - b * kTile, kTile);
        if (tid < kTile) {
            const unsigned long long d = tid < rows ? mask[(int64_t)(b * kTile + tid) * nblk + b] : 0ull;
            unsigned long long r = remv[b], kept = 0ull;
            for (int k = 0; k < rows; ++k) {                 // k is wave-uniform: the branch does not diverge
                const unsigned long long dk = __shfl(d, k);
                if (!((r >> k) & 1ull)) {
                    kept |= 1ull << k;
                    r |= dk;
                }
            }
            if ((kept >> tid) & 1ull) keep[count + __popcll(kept & ((1ull << tid) - 1ull))] = b * kTile + tid;
            if (tid == 0) s_kept = kept;
        }
        __syncthreads();
        const unsigned long long kept = s_kept;
        count += __popcll(kept);
        const int later = nblk - b - 1;
        if (later > 0 && kept) {
            const int total = kTile * later;
            for (int p = tid; p < total; p += kGreedyThreads) {
                const int l = p / later, c = b + 1 + (p - l * later);
                if ((kept >> l) & 1ull) atomicOr(&remv[c], mask[(int64_t)(b * kTile + l) * nblk + c]);
            }
        }
        __syncthreads();
    }
    if (tid == 0) *num_keep = count;
}

// ---------------------------------------------------------------------------------------------- backward
// One lane per pair: the reference's central differences over the 7 columns of box a, step by step in fp32.
__global__ __launch_bounds__(256) void iou3d_backward_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                             const float *__restrict__ grad, int64_t n, float eps,
                                                             float *__restrict__ grad_a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float box[7];
#pragma unroll
    for (int k = 0; k < 7; ++k) box[k] = a[i * 7 + k];
    const Prep B = prep_box(b + i * 7);
    const float g = grad[i], two_eps = 2.f * eps;
#pragma unroll
    for (int k = 0; k < 7; ++k) {
        const float orig = box[k];
        box[k] = orig - eps;
        const float lo = iou_3d(prep_box(box), B);
        box[k] = orig + eps;
        const float hi = iou_3d(prep_box(box), B);
        box[k] = orig;
        grad_a[i * 7 + k] = (hi - lo) / two_eps * g;
    }
}

inline unsigned grid_1d(int64_t n, int threads) { return (unsigned)ceil_div<int64_t>(n, threads); }

constexpr int64_t kMaxPairBoxes = int64_t(1) << 31;

}  // namespace
}  // namespace snvc

using namespace snvc;

extern "C" {

int snvc_iou3d_abi_version(void) { return 1; }

int64_t snvc_iou3d_pairwise_workspace_bytes(int64_t num_a, int64_t num_b) {
    if (num_a < 0 || num_b < 0) return -1;
    return (num_a + num_b) * (int64_t)sizeof(Prep);
}

int snvc_iou3d_pairwise(const float *boxes_a, int64_t num_a, const float *boxes_b, int64_t num_b, int what, int onebyone,
                        void *workspace, float *out, void *stream) {
    if (num_a < 0 || num_b < 0 || num_a >= kMaxPairBoxes || num_b >= kMaxPairBoxes)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_pairwise: box counts must be in [0, 2^31)");
    if (what < SNVC_IOU3D_OVERLAP || what > SNVC_IOU3D_IOU_3D)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_pairwise: what must be 0 (overlap), 1 (iou_bev) or 2 (iou3d)");
    if (onebyone && num_b != num_a)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_pairwise: one-by-one needs num_b == num_a");
    const int64_t outputs = onebyone ? num_a : num_a * num_b;
    if (outputs == 0) return SNVC_OK;
    if (!boxes_a || !boxes_b || !out || (!onebyone && !workspace))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_pairwise: null pointer");
    hipStream_t st = as_stream(stream);
    if (onebyone) {
        const unsigned g = grid_1d(num_a, 256);
        if (what == SNVC_IOU3D_OVERLAP) iou3d_onebyone_kernel<SNVC_IOU3D_OVERLAP><<<g, 256, 0, st>>>(boxes_a, boxes_b, num_a, out);
        else if (what == SNVC_IOU3D_IOU_BEV) iou3d_onebyone_kernel<SNVC_IOU3D_IOU_BEV><<<g, 256, 0, st>>>(boxes_a, boxes_b, num_a, out);
        else iou3d_onebyone_kernel<SNVC_IOU3D_IOU_3D><<<g, 256, 0, st>>>(boxes_a, boxes_b, num_a, out);
        return check_launch("iou3d_onebyone_kernel");
    }
    const int64_t col_tiles = ceil_div<int64_t>(num_b, kTile), blocks = col_tiles * ceil_div<int64_t>(num_a, 4);
    if (blocks > 0x7fffffff) return fail(SNVC_ERR_UNSUPPORTED, "snvc_iou3d_pairwise: more than 2^31 blocks of 64 x 4 pairs");
    Prep *pa = static_cast<Prep *>(workspace), *pb = pa + num_a;
    iou3d_prep_kernel<<<grid_1d(num_a, 256), 256, 0, st>>>(boxes_a, num_a, pa);
    iou3d_prep_kernel<<<grid_1d(num_b, 256), 256, 0, st>>>(boxes_b, num_b, pb);
    if (int rc = check_launch("iou3d_prep_kernel")) return rc;
    const dim3 grid((unsigned)blocks), block(kTile, 4);
    if (what == SNVC_IOU3D_OVERLAP) iou3d_matrix_kernel<SNVC_IOU3D_OVERLAP><<<grid, block, 0, st>>>(pa, num_a, pb, num_b, col_tiles, out);
    else if (what == SNVC_IOU3D_IOU_BEV) iou3d_matrix_kernel<SNVC_IOU3D_IOU_BEV><<<grid, block, 0, st>>>(pa, num_a, pb, num_b, col_tiles, out);
    else iou3d_matrix_kernel<SNVC_IOU3D_IOU_3D><<<grid, block, 0, st>>>(pa, num_a, pb, num_b, col_tiles, out);
    return check_launch("iou3d_matrix_kernel");
}

// layout: mask [n][nblk] u64, then prep [n]
int64_t snvc_iou3d_nms_workspace_bytes(int64_t num_boxes) {
    if (num_boxes < 0 || num_boxes > SNVC_NMS_MAX_BOXES) return -1;
    const int64_t nblk = ceil_div<int64_t>(num_boxes, kTile);
    return num_boxes * nblk * 8 + num_boxes * (int64_t)sizeof(Prep);
}

int snvc_iou3d_nms(const float *boxes, int64_t num_boxes, float thresh, int kind, void *workspace, int64_t *keep,
                   int32_t *num_keep, void *stream) {
    if (num_boxes < 0 || num_boxes > SNVC_NMS_MAX_BOXES)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_nms: num_boxes must be in [0, 65536]");
    if (kind != SNVC_NMS_ROTATED && kind != SNVC_NMS_NORMAL)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_nms: kind must be 0 (rotated) or 1 (normal)");
    if (!num_keep || (num_boxes > 0 && (!boxes || !keep || !workspace)))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_nms: null pointer");
    hipStream_t st = as_stream(stream);
    const int n = (int)num_boxes, nblk = (int)ceil_div<int64_t>(num_boxes, kTile);
    auto *mask = static_cast<unsigned long long *>(workspace);
    if (n > 0) {
        Prep *prep = reinterpret_cast<Prep *>(mask + (int64_t)n * nblk);
        const unsigned tiles = (unsigned)((int64_t)nblk * (nblk + 1) / 2);
        if (kind == SNVC_NMS_ROTATED) {
            iou3d_prep_kernel<<<grid_1d(n, 256), 256, 0, st>>>(boxes, n, prep);
            nms_mask_kernel<SNVC_NMS_ROTATED><<<tiles, kTile, 0, st>>>(boxes, prep, n, nblk, thresh, mask);
        } else {
            nms_mask_kernel<SNVC_NMS_NORMAL><<<tiles, kTile, 0, st>>>(boxes, prep, n, nblk, thresh, mask);
        }
        if (int rc = check_launch("nms_mask_kernel")) return rc;
    }
    nms_greedy_kernel<<<1, kGreedyThreads, 0, st>>>(mask, n, nblk, keep, num_keep);
    return check_launch("nms_greedy_kernel");
}

int snvc_iou3d_backward(const float *boxes_a, const float *boxes_b, const float *grad, int64_t num, float eps, float *grad_a,
                        void *stream) {
    if (num < 0 || num >= kMaxPairBoxes) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_backward: num must be in [0, 2^31)");
    if (!(eps > 0.f)) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_backward: eps must be positive");
    if (num == 0) return SNVC_OK;
    if (!boxes_a || !boxes_b || !grad || !grad_a) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_backward: null pointer");
    iou3d_backward_kernel<<<grid_1d(num, 256), 256, 0, as_stream(stream)>>>(boxes_a, boxes_b, grad, num, eps, grad_a);
    return check_launch("iou3d_backward_kernel");
}

int snvc_iou3d_boxes_iou_bev_cpu(const float *boxes_a_host, int64_t num_a, const float *boxes_b_host, int64_t num_b,
                                 float *iou_host) {
    if (num_a < 0 || num_b < 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_boxes_iou_bev_cpu: negative box count");
    if (num_a == 0 || num_b == 0) return SNVC_OK;
    if (!boxes_a_host || !boxes_b_host || !iou_host)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_iou3d_boxes_iou_bev_cpu: null pointer");
    std::vector<Prep> pb((size_t)num_b);
    for (int64_t j = 0; j < num_b; ++j) pb[(size_t)j] = prep_box(boxes_b_host + j * 7);
    for (int64_t i = 0; i < num_a; ++i) {
        const Prep A = prep_box(boxes_a_host + i * 7);
        for (int64_t j = 0; j < num_b; ++j) iou_host[i * num_b + j] = iou_bev(A, pb[(size_t)j]);
    }
    return SNVC_OK;
}

}  // extern "C"
