// Oriented-box IoU / DIoU / GIoU losses (include/snvc_oiou.h, DESIGN.md "Oriented IoU"): the exact intersection of two
// quadrilaterals, the smallest enclosing rectangle and the composites, with analytic gradients.
//
// One device function, pair_eval<T>, holds the arithmetic.  The forward kernel runs it with T = float, one lane per pair.  The
// backward kernel runs it with T = Dual (value + one tangent): a group of 16 (boxes) or 32 (quads) lanes serves a pair, lane i
// carries the tangent of input scalar i, contracts the tangents of the eight outputs with gout and stores one gradient
// element.  Every comparison is taken on values, never on tangents, so the lanes of a pair run the same path and the
// gradient is the derivative of the forward that ran, the arg-min of the enclosing box included.
//
// Intersection: the subject is cut along the diagonal from its reflex vertex (diagonal 0-2 if it is convex) and each triangle is
// clipped by Sutherland-Hodgman against the clip shape's four half-planes (a point on a line is inside).  A clipped triangle
// has at most seven vertices; the two vertex lists of a lane live in LDS ([slot][component][lane], so a wave's access to one
// slot is conflict-free), because their length depends on the data.  Everything else stays in registers with constant indices.
//
// The arithmetic is __host__ __device__: tools/oriented_iou_host_check.hip includes this file and runs pair_eval on the host
// (degenerate and non-finite inputs, under a host sanitizer, vertex lists of exact size), without a device.
//
// Products must round the same way whichever order they are written in (cross(e, e) has to be exactly 0 for the duplicate
// corners of identical shapes), so contraction into FMAs is off for this file.
#pragma clang fp contract(off)

#include <cmath>

#include "common.hpp"
#include "snvc_oiou.h"

namespace snvc {
namespace {

constexpr int kBlock = 64;       // one wave; no lane reads another lane's LDS, so there is no barrier
constexpr int kSlots = 8;        // vertices per list (a triangle clipped four times has at most 7)
// Enclosing candidates whose areas differ by no more than this, relatively, are a tie and the first one stays: 32 float32
// epsilons (3.8e-6), five times the spread rounding gives the tied lines of a rectangular hull (measured 7.5e-7).
constexpr float kTie = 32.f * 1.1920929e-7f;

struct Dual {
    float v, d;
};
__host__ __device__ inline Dual operator+(Dual a, Dual b) { return {a.v + b.v, a.d + b.d}; }
__host__ __device__ inline Dual operator-(Dual a, Dual b) { return {a.v - b.v, a.d - b.d}; }
__host__ __device__ inline Dual operator-(Dual a) { return {-a.v, -a.d}; }
__host__ __device__ inline Dual operator*(Dual a, Dual b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__host__ __device__ inline Dual operator/(Dual a, Dual b) {
    const float q = a.v / b.v;
    return {q, (a.d - q * b.d) / b.v};
}
__host__ __device__ inline Dual operator*(float a, Dual b) { return {a * b.v, a * b.d}; }
__host__ __device__ inline Dual operator+(float a, Dual b) { return {a + b.v, b.d}; }
__host__ __device__ inline Dual operator-(float a, Dual b) { return {a - b.v, -b.d}; }

__host__ __device__ inline float val(float x) { return x; }
__host__ __device__ inline float val(Dual x) { return x.v; }
__host__ __device__ inline float t_sqrt(float x) { return sqrtf(x); }
__host__ __device__ inline Dual t_sqrt(Dual x) {
    const float r = sqrtf(x.v);
    return {r, x.d / (2.f * r)};
}
__host__ __device__ inline float t_abs(float x) { return fabsf(x); }
__host__ __device__ inline Dual t_abs(Dual x) { return x.v < 0.f ? Dual{-x.v, -x.d} : x; }
__host__ __device__ inline void t_sincos(float a, float &s, float &c) { s = sinf(a); c = cosf(a); }
__host__ __device__ inline void t_sincos(Dual a, Dual &s, Dual &c) {
    const float sv = sinf(a.v), cv = cosf(a.v);
    s = {sv, cv * a.d};
    c = {cv, -sv * a.d};
}
template <class T>
__host__ __device__ inline T sel(bool c, T a, T b) { return c ? a : b; }
template <class T>
__host__ __device__ inline T lit(float x);
template <>
__host__ __device__ inline float lit<float>(float x) { return x; }
template <>
__host__ __device__ inline Dual lit<Dual>(float x) { return {x, 0.f}; }

// A lane's two vertex lists in LDS.
template <class T>
struct Lists;
template <>
struct Lists<float> {
    float *p;   // this lane's column of [2][kSlots][2][kBlock]
    __host__ __device__ float get(int list, int k, int c) const { return p[((list * kSlots + k) * 2 + c) * kBlock]; }
    __host__ __device__ void put(int list, int k, int c, float x) const { p[((list * kSlots + k) * 2 + c) * kBlock] = x; }
};
template <>
struct Lists<Dual> {
    float *p;   // this lane's column of [2][kSlots][2][2][kBlock]
    __host__ __device__ Dual get(int list, int k, int c) const {
        const float *q = p + (((list * kSlots + k) * 2 + c) * 2) * kBlock;
        return {q[0], q[kBlock]};
    }
    __host__ __device__ void put(int list, int k, int c, Dual x) const {
        float *q = p + (((list * kSlots + k) * 2 + c) * 2) * kBlock;
        q[0] = x.v;
        q[kBlock] = x.d;
    }
};
template <class T>
constexpr int lists_floats() { return 2 * kSlots * 2 * kBlock * (int)(sizeof(T) / sizeof(float)); }

template <class T>
__host__ __device__ inline T cross(T ax, T ay, T bx, T by) { return ax * by - ay * bx; }

// |area| of the triangle (x, y)[0..2] clipped against the half-planes of the quadrilateral (cx, cy), walked in the direction
// `sgn` makes positive.
template <class T>
__host__ __device__ T clip_triangle(const Lists<T> &L, const T (&x)[3], const T (&y)[3], const T (&cx)[4], const T (&cy)[4], float sgn) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        L.put(0, k, 0, x[k]);
        L.put(0, k, 1, y[k]);
    }
    int n = 3;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int in = e & 1, out = in ^ 1;
        const T ax = cx[e], ay = cy[e];
        const T ex = cx[(e + 1) & 3] - ax, ey = cy[(e + 1) & 3] - ay;
        int m = 0;
        if (n > 0) {
            T px = L.get(in, n - 1, 0), py = L.get(in, n - 1, 1);
            T dp = sgn * cross(ex, ey, px - ax, py - ay);
            for (int k = 0; k < n; ++k) {
                const T qx = L.get(in, k, 0), qy = L.get(in, k, 1);
                const T dq = sgn * cross(ex, ey, qx - ax, qy - ay);
                const bool qin = val(dq) >= 0.f, pin = val(dp) >= 0.f;
                if (qin != pin && m < kSlots) {
                    const T t = dp / (dp - dq);
                    L.put(out, m, 0, px + t * (qx - px));
                    L.put(out, m, 1, py + t * (qy - py));
                    ++m;
                }
                if (qin && m < kSlots) {
                    L.put(out, m, 0, qx);
                    L.put(out, m, 1, qy);
                    ++m;
                }
                px = qx; py = qy; dp = dq;
            }
        }
        n = m;
    }
    // four clips: the result is in list 0
    T twice = lit<T>(0.f);
    if (n > 0) {
        T px = L.get(0, n - 1, 0), py = L.get(0, n - 1, 1);
        for (int k = 0; k < n; ++k) {
            const T qx = L.get(0, k, 0), qy = L.get(0, k, 1);
            twice = twice + cross(px, py, qx, qy);
            px = qx; py = qy;
        }
    }
    return 0.5f * t_abs(twice);
}

// Intersection area of the simple quadrilateral s with the convex quadrilateral c.
template <class T>
__host__ __device__ T intersection(const Lists<T> &L, const T (&sx)[4], const T (&sy)[4], const T (&cx)[4], const T (&cy)[4]) {
    float twice_c = 0.f, twice_s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        twice_c += val(cross(cx[k], cy[k], cx[(k + 1) & 3], cy[(k + 1) & 3]));
        twice_s += val(cross(sx[k], sy[k], sx[(k + 1) & 3], sy[(k + 1) & 3]));
    }
    const float sgn = twice_c >= 0.f ? 1.f : -1.f;
    // a reflex vertex turns against the subject's own orientation; the cut starts there
    const float turn1 = val(cross(sx[1] - sx[0], sy[1] - sy[0], sx[2] - sx[1], sy[2] - sy[1]));
    const float turn3 = val(cross(sx[3] - sx[2], sy[3] - sy[2], sx[0] - sx[3], sy[0] - sy[3]));
    const float os = twice_s >= 0.f ? 1.f : -1.f;
    const bool cut13 = os * turn1 < 0.f || os * turn3 < 0.f;
    T x1[3], y1[3], x2[3], y2[3];
    x1[0] = sel(cut13, sx[1], sx[0]); y1[0] = sel(cut13, sy[1], sy[0]);
    x1[1] = sel(cut13, sx[2], sx[1]); y1[1] = sel(cut13, sy[2], sy[1]);
    x1[2] = sel(cut13, sx[3], sx[2]); y1[2] = sel(cut13, sy[3], sy[2]);
    x2[0] = x1[0];                    y2[0] = y1[0];
    x2[1] = x1[2];                    y2[1] = y1[2];
    x2[2] = sel(cut13, sx[0], sx[3]); y2[2] = sel(cut13, sy[0], sy[3]);
    return clip_triangle(L, x1, y1, cx, cy, sgn) + clip_triangle(L, x2, y2, cx, cy, sgn);
}

// (w, h) of the enclosing rectangle of the eight points.
template <class T>
__host__ __device__ void enclosing(const T (&px)[8], const T (&py)[8], int type, T &w, T &h) {
    if (type == SNVC_OIOU_ALIGNED) {
        T x0 = px[0], x1 = px[0], y0 = py[0], y1 = py[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            x0 = sel(val(px[k]) < val(x0), px[k], x0);
            x1 = sel(val(px[k]) > val(x1), px[k], x1);
            y0 = sel(val(py[k]) < val(y0), py[k], y0);
            y1 = sel(val(py[k]) > val(y1), py[k], y1);
        }
        w = x1 - x0;
        h = y1 - y0;
        return;
    }
    w = lit<T>(0.f);
    h = lit<T>(0.f);
    float best = INFINITY;
#pragma unroll
    for (int i = 0; i < 7; ++i) {
#pragma unroll
        for (int j = i + 1; j < 8; ++j) {
            const T ex = px[j] - px[i], ey = py[j] - py[i];
            const T len2 = ex * ex + ey * ey;
            if (!(val(len2) > 0.f)) continue;          // the same point twice is no line
            // over the other points: the signed distance (times the length) and the projection (times the length)
            T cmin = lit<T>(0.f), cmax = lit<T>(0.f), dmin = lit<T>(0.f), dmax = len2;   // points i and j themselves
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (k == i || k == j) continue;
                const T rx = px[k] - px[i], ry = py[k] - py[i];
                const T c = cross(ex, ey, rx, ry), d = ex * rx + ey * ry;
                cmin = sel(val(c) < val(cmin), c, cmin);
                cmax = sel(val(c) > val(cmax), c, cmax);
                dmin = sel(val(d) < val(dmin), d, dmin);
                dmax = sel(val(d) > val(dmax), d, dmax);
            }
            const bool above = val(cmin) >= 0.f, below = val(cmax) <= 0.f;
            if (!(above || below)) continue;
            const T len = t_sqrt(len2);
            const T cw = (dmax - dmin) / len;
            const T ch = sel(above, cmax, -cmin) / len;
            const float area = val(cw) * val(ch);
            if (area < best * (1.f - kTie)) {
                best = area;
                w = cw;
                h = ch;
            }
        }
    }
}

// The eight outputs of pair m.  in[]: the pair's input scalars in the order of the descriptor (a, b, ctr_a, ctr_b).
template <class T>
__host__ __device__ void pair_eval(const Lists<T> &L, const T *in, int form, int kind, int enc, T (&out)[8]) {
    T sx[4], sy[4], cx[4], cy[4], area1, area2, d2;
    if (form == SNVC_OIOU_BOXES) {
        // the clip box's centre is the origin
        const T ox = in[0] - in[5], oy = in[1] - in[6];
        const float lx[4] = {0.5f, -0.5f, -0.5f, 0.5f}, ly[4] = {0.5f, 0.5f, -0.5f, -0.5f};
        T s1, c1, s2, c2;
        t_sincos(in[4], s1, c1);
        t_sincos(in[9], s2, c2);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const T ax = lx[k] * in[2], ay = ly[k] * in[3], bx = lx[k] * in[7], by = ly[k] * in[8];
            sx[k] = ax * c1 - ay * s1 + ox;
            sy[k] = ax * s1 + ay * c1 + oy;
            cx[k] = bx * c2 - by * s2;
            cy[k] = bx * s2 + by * c2;
        }
        area1 = in[2] * in[3];
        area2 = in[7] * in[8];
        d2 = ox * ox + oy * oy;
    } else {
        // the mean of the clip shape's corners is the origin
        const T ox = 0.25f * ((in[8] + in[10]) + (in[12] + in[14])), oy = 0.25f * ((in[9] + in[11]) + (in[13] + in[15]));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sx[k] = in[2 * k] - ox;
            sy[k] = in[2 * k + 1] - oy;
            cx[k] = in[8 + 2 * k] - ox;
            cy[k] = in[9 + 2 * k] - oy;
        }
        area1 = 0.5f * (t_abs(cross(sx[1] - sx[0], sy[1] - sy[0], sx[3] - sx[0], sy[3] - sy[0])) +
                        t_abs(cross(sx[1] - sx[2], sy[1] - sy[2], sx[3] - sx[2], sy[3] - sy[2])));
        area2 = 0.5f * (t_abs(cross(cx[1] - cx[0], cy[1] - cy[0], cx[3] - cx[0], cy[3] - cy[0])) +
                        t_abs(cross(cx[1] - cx[2], cy[1] - cy[2], cx[3] - cx[2], cy[3] - cy[2])));
        const T ddx = in[16] - in[18], ddy = in[17] - in[19];
        d2 = ddx * ddx + ddy * ddy;
    }
    const T inter = intersection(L, sx, sy, cx, cy);
    const T u = area1 + area2 - inter;
    const T iou = inter / u;
    T px[8], py[8], w, h;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[k] = sx[k]; py[k] = sy[k];
        px[4 + k] = cx[k]; py[4 + k] = cy[k];
    }
    enclosing(px, py, enc, w, h);
    T loss;
    if (kind == SNVC_OIOU_DIOU) {
        loss = 1.f - iou + d2 / (w * w + h * h);
    } else {
        const T wh = w * h;
        loss = 1.f - iou + (wh - u) / wh;
    }
    out[0] = inter; out[1] = area1; out[2] = area2; out[3] = u;
    out[4] = iou;   out[5] = w;     out[6] = h;     out[7] = loss;
}

struct Args {
    const float *a, *b, *ctr_a, *ctr_b, *gout;
    float *out, *ga, *gb, *gctr_a, *gctr_b;
    int64_t M;
    int form, kind, enc;
};

// Input scalar i of pair m (i < 10 for boxes, < 20 for quads).
__host__ __device__ inline float load_input(const Args &g, int64_t m, int i) {
    if (g.form == SNVC_OIOU_BOXES) return i < 5 ? g.a[m * 5 + i] : g.b[m * 5 + i - 5];
    if (i < 8) return g.a[m * 8 + i];
    if (i < 16) return g.b[m * 8 + i - 8];
    return i < 18 ? g.ctr_a[m * 2 + i - 16] : g.ctr_b[m * 2 + i - 18];
}

__global__ __launch_bounds__(kBlock) void oiou_forward_kernel(Args g) {
    __shared__ float lds[lists_floats<float>()];
    const int64_t m = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (m >= g.M) return;
    const int n = g.form == SNVC_OIOU_BOXES ? 10 : 20;
    float in[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) in[i] = i < n ? load_input(g, m, i) : 0.f;
    float out[8];
    pair_eval<float>(Lists<float>{lds + threadIdx.x}, in, g.form, g.kind, g.enc, out);
    float4 *o = reinterpret_cast<float4 *>(g.out + m * 8);
    o[0] = make_float4(out[0], out[1], out[2], out[3]);
    o[1] = make_float4(out[4], out[5], out[6], out[7]);
}

// kGroup lanes per pair: lane i of the group differentiates with respect to input scalar i.
template <int kGroup>
__global__ __launch_bounds__(kBlock) void oiou_backward_kernel(Args g) {
    __shared__ float lds[lists_floats<Dual>()];
    const int lane = threadIdx.x % kGroup;
    const int64_t m = (int64_t)blockIdx.x * (kBlock / kGroup) + threadIdx.x / kGroup;
    const int n = g.form == SNVC_OIOU_BOXES ? 10 : 20;
    if (m >= g.M || lane >= n) return;
    Dual in[20];
#pragma unroll
    for (int i = 0; i < 20; ++i) in[i] = {i < n ? load_input(g, m, i) : 0.f, i == lane ? 1.f : 0.f};
    Dual out[8];
    pair_eval<Dual>(Lists<Dual>{lds + threadIdx.x}, in, g.form, g.kind, g.enc, out);
    const float4 *go = reinterpret_cast<const float4 *>(g.gout + m * 8);
    const float4 g0 = go[0], g1 = go[1];
    // a zero upstream element takes no part, so an output that is not finite does not reach a gradient nobody asked for
    const float gk[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (gk[k] != 0.f) acc += gk[k] * out[k].d;
    if (g.form == SNVC_OIOU_BOXES) {
        (lane < 5 ? g.ga + m * 5 + lane : g.gb + m * 5 + lane - 5)[0] = acc;
    } else if (lane < 8) {
        g.ga[m * 8 + lane] = acc;
    } else if (lane < 16) {
        g.gb[m * 8 + lane - 8] = acc;
    } else {
        (lane < 18 ? g.gctr_a + m * 2 + lane - 16 : g.gctr_b + m * 2 + lane - 18)[0] = acc;
    }
}

int check_desc(const snvc_oiou_desc *d, bool backward, const char *who) {
    auto bad = [&](int code, const char *what) {
        set_error("%s: %s", who, what);
        return code;
    };
    if (!d) return bad(SNVC_ERR_INVALID_ARGUMENT, "null descriptor");
    if (d->form != SNVC_OIOU_BOXES && d->form != SNVC_OIOU_QUADS) return bad(SNVC_ERR_INVALID_ARGUMENT, "unknown form");
    if (d->kind != SNVC_OIOU_DIOU && d->kind != SNVC_OIOU_GIOU) return bad(SNVC_ERR_INVALID_ARGUMENT, "unknown kind");
    if (d->enclosing != SNVC_OIOU_SMALLEST && d->enclosing != SNVC_OIOU_ALIGNED)
        return bad(SNVC_ERR_INVALID_ARGUMENT, "unknown enclosing type");
    if (d->reserved != 0) return bad(SNVC_ERR_INVALID_ARGUMENT, "the reserved field must be 0");
    if (d->M < 0) return bad(SNVC_ERR_INVALID_ARGUMENT, "negative size");
    if (d->M == 0) return SNVC_OK;
    if (d->M > (int64_t)INT32_MAX) return bad(SNVC_ERR_UNSUPPORTED, "more than 2^31 - 1 pairs in one call");
    const bool quads = d->form == SNVC_OIOU_QUADS;
    if (!d->a || !d->b || (quads && (!d->ctr_a || !d->ctr_b))) return bad(SNVC_ERR_INVALID_ARGUMENT, "null pointer");
    if (backward ? (!d->gout || !d->ga || !d->gb || (quads && (!d->gctr_a || !d->gctr_b))) : !d->out)
        return bad(SNVC_ERR_INVALID_ARGUMENT, "null pointer");
    if (!aligned(4, d->a, d->b, d->ctr_a, d->ctr_b, d->ga, d->gb, d->gctr_a, d->gctr_b) || !aligned(16, d->out, d->gout))
        return bad(SNVC_ERR_INVALID_ARGUMENT, "a pointer is not aligned (4 bytes; 16 for out and gout)");
    return SNVC_OK;
}

Args args_of(const snvc_oiou_desc *d) {
    Args g;
    g.a = d->a; g.b = d->b; g.ctr_a = d->ctr_a; g.ctr_b = d->ctr_b; g.gout = d->gout;
    g.out = d->out; g.ga = d->ga; g.gb = d->gb; g.gctr_a = d->gctr_a; g.gctr_b = d->gctr_b;
    g.M = d->M; g.form = d->form; g.kind = d->kind; g.enc = d->enclosing;
    return g;
}

}  // namespace
}  // namespace snvc

extern "C" {

int snvc_oiou_abi_version(void) { return 1; }

int snvc_oiou_forward(const snvc_oiou_desc *desc, void *stream) {
    using namespace snvc;
    const int rc = check_desc(desc, false, "snvc_oiou_forward");
    if (rc != SNVC_OK || desc->M == 0) return rc;
    oiou_forward_kernel<<<dim3((unsigned)ceil_div<int64_t>(desc->M, kBlock)), kBlock, 0, as_stream(stream)>>>(args_of(desc));
    return check_launch("snvc_oiou_forward");
}

int snvc_oiou_backward(const snvc_oiou_desc *desc, void *stream) {
    using namespace snvc;
    const int rc = check_desc(desc, true, "snvc_oiou_backward");
    if (rc != SNVC_OK || desc->M == 0) return rc;
    const Args g = args_of(desc);
    if (desc->form == SNVC_OIOU_BOXES)
        oiou_backward_kernel<16><<<dim3((unsigned)ceil_div<int64_t>(desc->M, kBlock / 16)), kBlock, 0, as_stream(stream)>>>(g);
    else
        oiou_backward_kernel<32><<<dim3((unsigned)ceil_div<int64_t>(desc->M, kBlock / 32)), kBlock, 0, as_stream(stream)>>>(g);
    return check_launch("snvc_oiou_backward");
}

}  // extern "C"
