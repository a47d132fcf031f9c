// The stereo RoI crops of the local (Vernier) model, made on the device (include/snvc_roicrop.h).
//
// Reference (host, numpy + cv2, one sample and one side at a time): refinementDataset._generate_rois
// (snvc/dataset/KITTIRefinement_dataset.py:555-621) with _get_cam_cord / _construct_box_3d (:523-553), _crop_instance
// (:500-521), Calibration.project_rect_to_image (snvc/dataset/kitti_util.py:282-293), kpts2cs / resize_crop /
// get_affine_transform / affine_transform (snvc/utils/img_proc.py), cv2.warpAffine(INTER_LINEAR, zero border) and
// torchvision's ToTensor + Normalize.  The arithmetic that stands in for cv2 is specified in DESIGN.md ("RoI crops").
//
// Two kernels:
//   prologue_kernel   one thread per (sample, side), float64, contraction off: the nine projected points of the RoI box, the
//                     crop centre and size, `trans` (from the float32-rounded point triples the reference hands to its solver),
//                     the local key points, and the inverse transform, left in the workspace with the resolved frame index.
//   warp_kernel       one thread per output pixel, all three channels: four taps of three bytes each from the interleaved
//                     image (byte loads: neither the base nor the row stride is aligned), blended in integers (fixed5) or
//                     in float32 (exact), then either stored as uint8 or looked up in the 3 x 256 normalisation table (LDS).
//                     Lanes run along u, so each of the three plane stores of a wave is one contiguous run.
// The image is small and stays in cache; the warp is bound by its stores and, for few crops, by launch latency.
#include <cmath>

#include "grid_point.hpp"
#include "snvc_roicrop.h"

namespace snvc {
namespace {

struct CropWs {
    double m[6];     // inverse of trans: source = m . (u, v, 1)
    int64_t frame;   // descriptor index, or -1: nothing to read, the crop is zero
};
static_assert(sizeof(CropWs) % 8 == 0, "workspace rows stay 8-byte aligned");

struct Params {
    int out_w, out_h, mode, swap_rb, raw;
    double aspect, range[3];
};

constexpr double kEnlarge = 1.1;     // kpts2cs(enlarge=1.1)
constexpr double kSat = 0x1p60;      // fixed-point coordinates saturate here: far outside every image

// ---------------------------------------------------------------------------------------------------- prologue
__global__ void __launch_bounds__(64)
prologue_kernel(const double *__restrict__ samples, const double *__restrict__ P_left, const double *__restrict__ P_right,
                const int32_t *__restrict__ frame, CropWs *__restrict__ ws, double *__restrict__ trans_l,
                double *__restrict__ trans_r, double *__restrict__ kpts_l, double *__restrict__ kpts_r,
                float *__restrict__ local_l, float *__restrict__ local_r, Params g, int F, int N) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * N) return;
    const int64_t n = t >> 1;
    const int side = t & 1;
    const double *s = samples + n * 7;
    const int fr = frame ? frame[n] : 0;
    const bool known = fr >= 0 && fr < F;
    const double *P = (side == 0 ? P_left : P_right) + (int64_t)(known ? fr : 0) * 12;
    double *trans = (side == 0 ? trans_l : trans_r) + n * 6;
    double *kp = (side == 0 ? kpts_l : kpts_r) + n * 18;
    float *lc = (side == 0 ? local_l : local_r) + n * 18;

    // :589-591: the RoI box has the size grid_range and keeps the sample's centre height
    double y;
    {
#pragma clang fp contract(off)
        const double old_center_y = s[4] - s[0] * 0.5;
        y = old_center_y + g.range[0] * 0.5;
    }
    double pts[9][3], u[9], v[9];
    box_points(g.range[0], g.range[1], g.range[2], s[3], y, s[5], s[6], pts);
    double minx = 0, maxx = 0, miny = 0, maxy = 0;
    for (int k = 0; k < 9; ++k) {
        const double X = pts[k][0], Y = pts[k][1], Z = pts[k][2];
        // the projection of grid_projection.hip: k-ascending FMA chain, then the perspective divide
        const double pu = fma(1.0, P[3], fma(Z, P[2], fma(Y, P[1], X * P[0])));
        const double pv = fma(1.0, P[7], fma(Z, P[6], fma(Y, P[5], X * P[4])));
        const double pw = fma(1.0, P[11], fma(Z, P[10], fma(Y, P[9], X * P[8])));
        u[k] = pu / pw;
        v[k] = pv / pw;
        kp[2 * k] = u[k];
        kp[2 * k + 1] = v[k];
        if (k == 0) {
            minx = maxx = u[k]; miny = maxy = v[k];
        } else {
            minx = fmin(minx, u[k]); maxx = fmax(maxx, u[k]);
            miny = fmin(miny, v[k]); maxy = fmax(maxy, v[k]);
        }
    }
    double t00, t02, t11, t12;
    {
#pragma clang fp contract(off)
        // kpts2cs(method='boundary') and resize_crop
        const double cx = (minx + maxx) / 2, cy = (miny + maxy) / 2;
        const double w = (maxx - minx) * kEnlarge, h = (maxy - miny) * kEnlarge;
        const double src_w = (h / w > g.aspect) ? h * (1 / g.aspect) : w;
        // get_affine_transform(rot=0, absolute=True): the three source points as the float32 array holds them
        const float cxf = (float)cx, cyf = (float)cy;          // src[0]
        const float s1y = (float)(cy + src_w * -0.5);          // src[1] = (cxf, s1y)
        const float dy = cyf - s1y;                            // get_3rd_point: direct = src[0] - src[1], in float32
        const float c2x = cxf - dy;                            // src[2] = (c2x, s1y)
        // destination points: (Wr/2, Hr/2), (Wr/2, Hr/2 - Wr/2), (0, Hr/2 - Wr/2), exact in float32 for sides <= 32767.
        // The solve: x' = kx (x - cxf) + Wr/2 with kx from src[1] -> src[2], y' = ky (y - cyf) + Hr/2 with ky from src[0] -> src[1].
        const double half_w = 0.5 * (double)g.out_w, half_h = 0.5 * (double)g.out_h;
        t00 = half_w / ((double)cxf - (double)c2x);
        t11 = half_w / ((double)cyf - (double)s1y);
        t02 = half_w - t00 * (double)cxf;
        t12 = half_h - t11 * (double)cyf;
    }
    trans[0] = t00; trans[1] = 0.0; trans[2] = t02;
    trans[3] = 0.0; trans[4] = t11; trans[5] = t12;
    for (int k = 0; k < 9; ++k) {
        // affine_transform: trans @ [u; v; 1], cast to float32
        lc[2 * k] = (float)fma(t02, 1.0, fma(0.0, v[k], t00 * u[k]));
        lc[2 * k + 1] = (float)fma(t12, 1.0, fma(t11, v[k], 0.0 * u[k]));
    }
    CropWs &o = ws[t];
    {
#pragma clang fp contract(off)
        const double t01 = 0.0, t10 = 0.0;
        double D = t00 * t11 - t01 * t10;
        D = D != 0.0 ? 1.0 / D : 0.0;
        const double m00 = t11 * D, m11 = t00 * D, m01 = -t01 * D, m10 = -t10 * D;
        o.m[0] = m00; o.m[1] = m01; o.m[2] = -m00 * t02 - m01 * t12;
        o.m[3] = m10; o.m[4] = m11; o.m[5] = -m10 * t02 - m11 * t12;
    }
    o.frame = known ? fr : -1;
}

// ---------------------------------------------------------------------------------------------------- warp
// round-half-to-even of a double into 64 bits; beyond +-2^60 it saturates and NaN counts as -2^60
__device__ __forceinline__ long long round_fixed(double x) { return llrint(fmin(fmax(x, -kSat), kSat)); }

struct Image {
    const uint8_t *data;
    long long H, W, stride;
};

// the three bytes of pixel (r, c), or zeros outside the image
__device__ __forceinline__ void tap(const Image &im, long long r, long long c, int &p0, int &p1, int &p2) {
    p0 = p1 = p2 = 0;
    if (r >= 0 && r < im.H && c >= 0 && c < im.W) {
        const uint8_t *p = im.data + r * im.stride + c * 3;
        p0 = p[0]; p1 = p[1]; p2 = p[2];
    }
}

__device__ __forceinline__ int blend_exact(int p00, int p01, int p10, int p11, float ax, float ay) {
#pragma clang fp contract(off)
    const float bx = 1.0f - ax, by = 1.0f - ay;
    const float top = (float)p00 * bx + (float)p01 * ax;
    const float bot = (float)p10 * bx + (float)p11 * ax;
    const float val = top * by + bot * ay;
    return (int)fminf(fmaxf(rintf(val), 0.0f), 255.0f);
}

__global__ void __launch_bounds__(256)
warp_kernel(const snvc_roicrop_image *__restrict__ left_images, const snvc_roicrop_image *__restrict__ right_images,
            const CropWs *__restrict__ ws, const float *__restrict__ norm_table, void *__restrict__ left_rois,
            void *__restrict__ right_rois, Params g) {
    __shared__ float table[768];
    if (!g.raw) {
        for (int i = threadIdx.x; i < 768; i += blockDim.x) table[i] = norm_table[i];
        __syncthreads();
    }
    const int HW = g.out_w * g.out_h;               // <= 32767^2 < 2^31
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= HW) return;
    const int64_t n = blockIdx.y >> 1;
    const int side = blockIdx.y & 1;
    const CropWs w = ws[blockIdx.y];
    Image im = {nullptr, 0, 0, 0};
    if (w.frame >= 0) {
        const snvc_roicrop_image d = (side == 0 ? left_images : right_images)[w.frame];
        if (d.data && d.height > 0 && d.width > 0 && d.height <= SNVC_ROICROP_MAX_SIDE && d.width <= SNVC_ROICROP_MAX_SIDE &&
            d.row_stride >= 3ll * d.width)
            im = {d.data, d.height, d.width, d.row_stride};
    }
    const int u = p % g.out_w, v = p / g.out_w;
    int c[3];
    if (g.mode == SNVC_ROICROP_FIXED5) {
        long long X, Y;
        {
#pragma clang fp contract(off)
            X = (round_fixed((w.m[1] * v + w.m[2]) * 1024.0) + 16 + round_fixed(w.m[0] * u * 1024.0)) >> 5;
            Y = (round_fixed((w.m[4] * v + w.m[5]) * 1024.0) + 16 + round_fixed(w.m[3] * u * 1024.0)) >> 5;
        }
        const long long sx = X >> 5, sy = Y >> 5;
        const int ax = (int)(X & 31), ay = (int)(Y & 31);
        int a[3], b[3], d[3], e[3];
        tap(im, sy, sx, a[0], a[1], a[2]);
        tap(im, sy, sx + 1, b[0], b[1], b[2]);
        tap(im, sy + 1, sx, d[0], d[1], d[2]);
        tap(im, sy + 1, sx + 1, e[0], e[1], e[2]);
        const int w00 = (32 - ax) * (32 - ay), w01 = ax * (32 - ay), w10 = (32 - ax) * ay, w11 = ax * ay;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (32 * (w00 * a[k] + w01 * b[k] + w10 * d[k] + w11 * e[k]) + 16384) >> 15;
    } else {
        double xs, ys;
        {
#pragma clang fp contract(off)
            xs = w.m[0] * u + (w.m[1] * v + w.m[2]);
            ys = w.m[3] * u + (w.m[4] * v + w.m[5]);
        }
        c[0] = c[1] = c[2] = 0;
        if (fabs(xs) < 2147483648.0 && fabs(ys) < 2147483648.0) {      // false for NaN
            const double fx = floor(xs), fy = floor(ys);
            const float ax = (float)(xs - fx), ay = (float)(ys - fy);
            const long long sx = (long long)fx, sy = (long long)fy;
            int a[3], b[3], d[3], e[3];
            tap(im, sy, sx, a[0], a[1], a[2]);
            tap(im, sy, sx + 1, b[0], b[1], b[2]);
            tap(im, sy + 1, sx, d[0], d[1], d[2]);
            tap(im, sy + 1, sx + 1, e[0], e[1], e[2]);
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = blend_exact(a[k], b[k], d[k], e[k], ax, ay);
        }
    }
    if (g.swap_rb) {
        const int tmp = c[0]; c[0] = c[2]; c[2] = tmp;
    }
    const int64_t base = n * 3 * (int64_t)HW + p;
    if (g.raw) {
        uint8_t *out = static_cast<uint8_t *>(side == 0 ? left_rois : right_rois);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[base + (int64_t)k * HW] = (uint8_t)c[k];
    } else {
        float *out = static_cast<float *>(side == 0 ? left_rois : right_rois);
#pragma unroll
        for (int k = 0; k < 3; ++k) out[base + (int64_t)k * HW] = table[k * 256 + c[k]];
    }
}

}  // namespace
}  // namespace snvc

extern "C" {

int snvc_roicrop_abi_version(void) { return 1; }

int64_t snvc_roicrop_workspace_bytes(int64_t N) {
    if (N < 0 || N > SNVC_ROICROP_MAX_SAMPLES) return -1;
    return 2 * N * (int64_t)sizeof(snvc::CropWs);
}

int snvc_roicrop(const snvc_roicrop_config *cfg, const snvc_roicrop_image *left_images, const snvc_roicrop_image *right_images,
                 int64_t F, const int32_t *frame, const double *samples, const double *P_left, const double *P_right, int64_t N,
                 const float *norm_table, void *workspace, void *left_rois, void *right_rois, double *trans_l, double *trans_r,
                 double *kpts_l, double *kpts_r, float *local_l, float *local_r, void *stream) {
    using namespace snvc;
    if (!cfg) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: null config");
    if (cfg->out_w < 1 || cfg->out_h < 1 || cfg->out_w > SNVC_ROICROP_MAX_SIDE || cfg->out_h > SNVC_ROICROP_MAX_SIDE)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: the resolution must be within 1 .. 32767 a side");
    if ((cfg->interpolation != SNVC_ROICROP_FIXED5 && cfg->interpolation != SNVC_ROICROP_EXACT) || (cfg->swap_rb | 1) != 1 ||
        (cfg->raw | 1) != 1 || cfg->reserved != 0)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: bad interpolation, swap_rb, raw or reserved field");
    if (!(cfg->aspect_ratio > 0) || !std::isfinite(cfg->aspect_ratio))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: aspect_ratio must be positive and finite");
    for (int k = 0; k < 3; ++k)
        if (!(cfg->grid_range[k] > 0) || !std::isfinite(cfg->grid_range[k]))
            return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: grid_range must be positive and finite");
    if (N < 0 || F < 1 || F > INT32_MAX) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: bad sizes");
    if (N > SNVC_ROICROP_MAX_SAMPLES) return fail(SNVC_ERR_UNSUPPORTED, "snvc_roicrop: more than 32767 samples in one call");
    if (N == 0) return SNVC_OK;
    if (!left_images || !right_images || !samples || !P_left || !P_right || !workspace || !left_rois || !right_rois || !trans_l ||
        !trans_r || !kpts_l || !kpts_r || !local_l || !local_r || (!cfg->raw && !norm_table))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: null pointer");
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_roicrop: the workspace is not 8-byte aligned");
    Params g;
    g.out_w = cfg->out_w; g.out_h = cfg->out_h; g.mode = cfg->interpolation; g.swap_rb = cfg->swap_rb; g.raw = cfg->raw;
    g.aspect = cfg->aspect_ratio;
    for (int k = 0; k < 3; ++k) g.range[k] = cfg->grid_range[k];
    hipStream_t st = as_stream(stream);
    CropWs *ws = static_cast<CropWs *>(workspace);
    prologue_kernel<<<ceil_div<int>(2 * (int)N, 64), 64, 0, st>>>(samples, P_left, P_right, frame, ws, trans_l, trans_r, kpts_l, kpts_r,
                                                                  local_l, local_r, g, (int)F, (int)N);
    const int rc = check_launch("snvc_roicrop (prologue)");
    if (rc != SNVC_OK) return rc;
    const int HW = cfg->out_w * cfg->out_h;
    dim3 grid((unsigned)ceil_div(HW, 256), (unsigned)(2 * N));
    warp_kernel<<<grid, 256, 0, st>>>(left_images, right_images, ws, norm_table, left_rois, right_rois, g);
    return check_launch("snvc_roicrop (warp)");
}

}  // extern "C"
