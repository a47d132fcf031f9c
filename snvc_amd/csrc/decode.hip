// The box read-out of the local (Vernier) model, made on the device (include/snvc_decode.h).
//
// Reference (host, numpy, one instance at a time): VernierScale.ncf_to_update_2d (vernier.py:665-738) with _get_basis,
// get_cam_cord / construct_box_3d (:740-765), get_canonical (:612-620), register_BEV (:627-663) and
// utils/transformation.compute_rigid_transform (:153-188), and Filter (tools/inference_agnostic.py:94-106).  The arithmetic
// followed here is snvc_amd/decode.py's, which states the closed forms; DESIGN.md ("Box read-out") has the specification.
//
// Two kernels:
//   scan_kernel   one 256-thread workgroup per (instance, part) map of M floats.  One read of the map gives the first-maximum
//                 argmax under numpy's NaN rule (the better() predicate of elementwise.hip, restated), the minimum and a
//                 has-NaN flag.  16-byte loads from the first 16-byte boundary of the row on, scalar loads for the up to three
//                 elements in front of it and behind the last whole quad (a row starts r * M * 4 bytes into the tensor, so an
//                 odd M misaligns every second row).  Wave-64 shuffles, then a 4-entry LDS combine by thread 0.
//   fit_kernel    one thread per instance, float64, contraction off: the keep flag, the part targets, `one_part`, and for
//                 nine parts the two 2D Procrustes fits that give `all_parts`.
// The maps are read once at the rate a 256-thread block per row reaches; the fit is a few hundred flops per instance.
#include <cmath>

#include "common.hpp"
#include "snvc_decode.h"

namespace snvc {
namespace {

struct RowStat {
    float min;        // the map's minimum over its non-NaN values (+inf if there is none)
    int32_t has_nan;
};
static_assert(sizeof(RowStat) == 8, "workspace rows stay 8-byte aligned");

struct Params {
    double x0, xs, z0, zs;   // range start and extent
    float min_val, max_val;
    int source;
};

// ---------------------------------------------------------------------------------------------------- scan
// true if (va, ia) should replace (vb, ib): numpy's argmax order -- a NaN is the maximum, the first of equals wins
__device__ __forceinline__ bool better(float va, int64_t ia, float vb, int64_t ib) {
    const bool a_nan = va != va, b_nan = vb != vb;
    if (a_nan || b_nan) {
        if (a_nan && b_nan) return ia < ib;
        return a_nan;
    }
    if (va > vb) return true;
    if (va < vb) return false;
    return ia < ib;
}

struct Best {
    float v, mn;
    int64_t i;
    int nan;
    __device__ __forceinline__ void take(float x, int64_t at) {
        if (better(x, at, v, i)) { v = x; i = at; }
        mn = fminf(mn, x);          // fminf returns the other operand for a NaN
        nan |= (x != x);
    }
    __device__ __forceinline__ void merge(float ov, int64_t oi, float omn, int onan) {
        if (better(ov, oi, v, i)) { v = ov; i = oi; }
        mn = fminf(mn, omn);
        nan |= onan;
    }
};

__global__ void __launch_bounds__(256)
scan_kernel(const float *__restrict__ ncf, float *__restrict__ conf, int64_t *__restrict__ index, RowStat *__restrict__ stat,
            int64_t M) {
    const int64_t r = blockIdx.x;
    const float *row = ncf + r * M;
    // (-inf, INT64_MAX) is replaced by every element: a greater value, a NaN, or -inf at a lower index
    Best b = {-INFINITY, INFINITY, INT64_MAX, 0};
    const int64_t lead = (4 - (int64_t)((reinterpret_cast<uintptr_t>(row) >> 2) & 3)) & 3;   // floats up to the 16-byte boundary
    const int64_t head = lead < M ? lead : M;
    const int64_t quads = (M - head) >> 2;
    const int64_t tail0 = head + 4 * quads;
    if ((int64_t)threadIdx.x < head) b.take(row[threadIdx.x], threadIdx.x);
    const float4 *body = reinterpret_cast<const float4 *>(row + head);
    for (int64_t q = threadIdx.x; q < quads; q += blockDim.x) {
        const float4 x = body[q];
        const int64_t at = head + 4 * q;
        b.take(x.x, at);
        b.take(x.y, at + 1);
        b.take(x.z, at + 2);
        b.take(x.w, at + 3);
    }
    if (tail0 + (int64_t)threadIdx.x < M) b.take(row[tail0 + threadIdx.x], tail0 + threadIdx.x);

    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_down(b.v, off, 64), omn = __shfl_down(b.mn, off, 64);
        const long long oi = __shfl_down((long long)b.i, off, 64);
        const int onan = __shfl_down(b.nan, off, 64);
        b.merge(ov, oi, omn, onan);
    }
    __shared__ float sv[4], smn[4];
    __shared__ int64_t si[4];
    __shared__ int snan[4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { sv[wave] = b.v; smn[wave] = b.mn; si[wave] = b.i; snan[wave] = b.nan; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) b.merge(sv[k], si[k], smn[k], snan[k]);
        conf[r] = b.v;
        index[r] = b.i;
        stat[r].min = b.mn;
        stat[r].has_nan = b.nan;
    }
}

// ---------------------------------------------------------------------------------------------------- fit
// rigid_transform_2d: the rotation angle of the least-squares fit X -> Y of nine points, unweighted centroids (written to
// cx / cy), the centred source scaled by w (NULL: unweighted)
__device__ __forceinline__ double fit_angle(const double (&X)[2][9], const double (&Y)[2][9], const double *w, double (&cx)[2],
                                            double (&cy)[2]) {
#pragma clang fp contract(off)
    for (int a = 0; a < 2; ++a) {
        double sx = 0.0, sy = 0.0;
        for (int k = 0; k < 9; ++k) { sx += X[a][k]; sy += Y[a][k]; }
        cx[a] = sx / 9.0;
        cy[a] = sy / 9.0;
    }
    double h[2][2] = {{0.0, 0.0}, {0.0, 0.0}};
    for (int k = 0; k < 9; ++k) {
        const double wk = w ? w[k] : 1.0;
        const double x0 = (X[0][k] - cx[0]) * wk, x1 = (X[1][k] - cx[1]) * wk;
        const double y0 = Y[0][k] - cy[0], y1 = Y[1][k] - cy[1];
        h[0][0] += x0 * y0; h[0][1] += x0 * y1;
        h[1][0] += x1 * y0; h[1][1] += x1 * y1;
    }
    return atan2(h[0][1] - h[1][0], h[0][0] + h[1][1]);
}

// One instance.  `all_parts` is NULL with P = 1.
__device__ __forceinline__ void fit_instance(int64_t n, const double *__restrict__ samples, const void *__restrict__ source,
                                             const float *__restrict__ conf, const int64_t *__restrict__ index,
                                             const RowStat *__restrict__ stat, uint8_t *__restrict__ keep,
                                             double *__restrict__ one_part, double *__restrict__ all_parts, const Params &g, int P) {
#pragma clang fp contract(off)
    // the part fractions of get_cam_cord (centre, then the eight corners) and of get_canonical
    constexpr double kCamFx[9] = {0.5, 1.0, 1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0};
    constexpr double kCamFz[9] = {0.5, 1.0, 1.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0};
    constexpr double kCanFx[9] = {0.0, 0.5, 0.5, 0.5, 0.5, -0.5, -0.5, -0.5, -0.5};
    constexpr double kCanFz[9] = {0.0, 0.5, 0.5, -0.5, -0.5, 0.5, 0.5, -0.5, -0.5};
    double s[7];
    for (int k = 0; k < 7; ++k) s[k] = samples[n * 7 + k];
    bool kept = true;
    for (int p = 0; p < P; ++p) {
        const RowStat st = stat[n * P + p];
        // without a NaN the confidence is the map's maximum; comparisons with a NaN bound are false
        kept = kept && !st.has_nan && st.min >= g.min_val && conf[n * P + p] <= g.max_val;
    }
    keep[n] = kept ? 1 : 0;
    if (!kept) {
        for (int k = 0; k < 7; ++k) one_part[n * 7 + k] = s[k];
        if (all_parts)
            for (int k = 0; k < 7; ++k) all_parts[n * 7 + k] = s[k];
        return;
    }
    const double c = cos(s[6]), sn = sin(s[6]);
    // basis = rotation_y(ry) @ _OBJECT_AXES.T = [[-s, 0, c], [0, 1, 0], [-c, 0, -s]]; the offset's y is 0, so a part's
    // target is centre + (ox * -s + oz * c, 0, ox * -c + oz * -s)
    const double centre_x = s[3], centre_y = s[4] - 0.5 * s[0], centre_z = s[5];
    double dst[2][9];
    for (int p = 0; p < P; ++p) {
        double ox, oz;
        if (g.source == SNVC_DECODE_GRID) {
            const double *row = static_cast<const double *>(source) + index[n * P + p] * 3;
            ox = row[0];
            oz = row[2];
        } else {
            double u, v;
            if (g.source == SNVC_DECODE_COORDS_F32) {
                const float *q = static_cast<const float *>(source) + (n * P + p) * 2;
                u = (double)q[0]; v = (double)q[1];
            } else {
                const double *q = static_cast<const double *>(source) + (n * P + p) * 2;
                u = q[0]; v = q[1];
            }
            ox = g.x0 + u * g.xs;
            oz = g.z0 + v * g.zs;
        }
        dst[0][p] = centre_x + (ox * -sn + oz * c);
        dst[1][p] = centre_z + (ox * -c + oz * -sn);
    }
    // moved: the box carried to its centre part's target, y back to the bottom centre
    one_part[n * 7 + 0] = s[0]; one_part[n * 7 + 1] = s[1]; one_part[n * 7 + 2] = s[2];
    one_part[n * 7 + 3] = dst[0][0];
    one_part[n * 7 + 4] = (centre_y + 0.0) + 0.5 * s[0];
    one_part[n * 7 + 5] = dst[1][0];
    one_part[n * 7 + 6] = s[6];
    if (P != 9) return;

    // get_cam_cord rows x and z, with the float32-rounded extents the reference shifts its corner lists by
    const double half_l = (double)(float)s[2] / 2, half_w = (double)(float)s[1] / 2;
    double src[2][9], w[9];
    for (int k = 0; k < 9; ++k) {
        const double bx = kCamFx[k] * s[2] - half_l, bz = kCamFz[k] * s[1] - half_w;
        src[0][k] = (c * bx + sn * bz) + s[3];
        src[1][k] = (-sn * bx + c * bz) + s[5];
        w[k] = (double)conf[n * 9 + k];
    }
    double cx[2], cy[2];
    const double theta = fit_angle(src, dst, w, cx, cy);
    const double rc = cos(theta), rs = sin(theta);
    const double tx = cy[0] - (rc * cx[0] + -rs * cx[1]), tz = cy[1] - (rs * cx[0] + rc * cx[1]);
    double fitted[2][9], canon[2][9];
    for (int k = 0; k < 9; ++k) {
        fitted[0][k] = (rc * src[0][k] + -rs * src[1][k]) + tx;
        fitted[1][k] = (rs * src[0][k] + rc * src[1][k]) + tz;
        canon[0][k] = kCanFx[k] * s[2];
        canon[1][k] = kCanFz[k] * s[1];
    }
    const double theta_c = fit_angle(canon, fitted, nullptr, cx, cy);
    all_parts[n * 7 + 0] = s[0]; all_parts[n * 7 + 1] = s[1]; all_parts[n * 7 + 2] = s[2];
    all_parts[n * 7 + 3] = fitted[0][0];
    all_parts[n * 7 + 4] = s[4];
    all_parts[n * 7 + 5] = fitted[1][0];
    all_parts[n * 7 + 6] = -atan2(sin(theta_c), cos(theta_c));      // KITTI's yaw is positive clockwise
}

__global__ void __launch_bounds__(64)
fit_kernel(const double *__restrict__ samples, const void *__restrict__ source, const float *__restrict__ conf,
           const int64_t *__restrict__ index, const RowStat *__restrict__ stat, uint8_t *__restrict__ keep,
           double *__restrict__ one_part, double *__restrict__ all_parts, Params g, int P, int64_t N) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n < N) fit_instance(n, samples, source, conf, index, stat, keep, one_part, all_parts, g, P);
}

}  // namespace
}  // namespace snvc

extern "C" {

int snvc_decode_abi_version(void) { return 1; }

int64_t snvc_decode_workspace_bytes(int64_t N, int64_t P) {
    if (N < 0 || (P != 1 && P != 9) || N > INT32_MAX / P) return -1;
    return N * P * (int64_t)sizeof(snvc::RowStat);
}

int snvc_decode_boxes(const snvc_decode_config *cfg, const float *ncf, const double *samples, const void *grid_or_coordinates,
                      int64_t N, int64_t P, int64_t M, void *workspace, float *conf, int64_t *index, uint8_t *keep,
                      double *one_part, double *all_parts, void *stream) {
    using namespace snvc;
    if (!cfg) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: null config");
    if (cfg->source < SNVC_DECODE_GRID || cfg->source > SNVC_DECODE_COORDS_F64 || cfg->reserved != 0)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: bad source or reserved field");
    if (P != 1 && P != 9) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: the number of parts must be 1 or 9");
    if (N < 0 || M < 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: negative size");
    if (N > INT32_MAX / P) return fail(SNVC_ERR_UNSUPPORTED, "snvc_decode_boxes: more than 2^31 - 1 maps in one call");
    if (N == 0) return SNVC_OK;
    if (M == 0) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: attempt to get argmax of an empty sequence");
    if (!ncf || !samples || !grid_or_coordinates || !workspace || !conf || !index || !keep || !one_part || (P == 9 && !all_parts))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: null pointer");
    if (!aligned(8, samples, workspace, index, one_part, all_parts) || !aligned(4, ncf, conf) ||
        !aligned(cfg->source == SNVC_DECODE_COORDS_F32 ? 4 : 8, grid_or_coordinates))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_decode_boxes: a pointer is not aligned to its element size");
    Params g;
    g.x0 = cfg->x_range[0]; g.xs = cfg->x_range[1] - cfg->x_range[0];
    g.z0 = cfg->z_range[0]; g.zs = cfg->z_range[1] - cfg->z_range[0];
    g.min_val = cfg->min_val; g.max_val = cfg->max_val; g.source = cfg->source;
    hipStream_t st = as_stream(stream);
    RowStat *stat = static_cast<RowStat *>(workspace);
    scan_kernel<<<dim3((unsigned)(N * P)), 256, 0, st>>>(ncf, conf, index, stat, M);
    const int rc = check_launch("snvc_decode_boxes (scan)");
    if (rc != SNVC_OK) return rc;
    fit_kernel<<<dim3((unsigned)ceil_div<int64_t>(N, 64)), 64, 0, st>>>(samples, grid_or_coordinates, conf, index, stat, keep,
                                                                         one_part, all_parts, g, (int)P, N);
    return check_launch("snvc_decode_boxes (fit)");
}

}  // extern "C"
