// Training targets of the local (Vernier) model, generated on the device (include/snvc_targets.h).
//
// Reference (host, numpy float64, one sample at a time): refinementDataset._generate_displacement_field
// (snvc/dataset/KITTIRefinement_dataset.py:870-903), which calls _construct_neural_confidence_field (:722-777),
// _draw_heatmaps_3d / _draw_heatmaps_2d (:623-702), _get_point_cloud (:779-826), _get_cam_cord / _construct_box_3d
// (:523-553), _get_basis (:704-720), construct_mesh_cuboid / Mesh.in_mesh (snvc/utils/bounding_box.py:286-297,360-390) and
// Calibration.project_velo_to_rect (snvc/dataset/kitti_util.py:252-277).
//
// Three parts:
//   prologue_kernel   one thread per sample: the nine box points of the proposal's RoI box and of the label, their twelve
//                     outward planes, the label's part positions in the proposal's frame (written as float32), the voxel
//                     index of every part and the clipped +-3 sigma window around it.  Left in a small workspace.
//   fields_kernel     streams the heat maps: every output element is written once, 0 or exp(-d^2 / (2 sigma^2)), 16 bytes
//                     per lane where the address allows it and single floats at the unaligned ends of a channel.
//   voxel_kernel      pass A: -1 where the voxel's grid point (the one grid_projection.hip produces) is inside the label's
//                     box, 0 where it is outside; streamed like the heat maps.
//   point_kernel      pass B: one thread per (sample, point): the twelve plane tests, the two membership masks, and 1.0f into
//                     the voxel of a foreground point unless pass A left 0 there (the reference writes the background last).
// All decisions are float64.  They agree with numpy's unless a value sits within rounding noise (about 1e-14 relative) of a
// plane or of a cell border; the summation order of numpy's matrix products is not reproduced.
// The passes are bound by their stores; nothing is reused, so there is no LDS.
#include <cmath>

#include "grid_point.hpp"
#include "snvc_targets.h"

namespace snvc {
namespace {

constexpr int kParts = SNVC_TARGETS_MAX_PARTS;

struct SampleWs {
    double roi[6][4];      // outward planes of the RoI box (the proposal with its size replaced by grid_range)
    double gt[6][4];       // outward planes of the label
    double sn, cs;         // sin, cos of the proposal's ry: the basis of _get_basis
    double ctr[3];         // centre point of the RoI box (kpts_3d[0] in _get_point_cloud)
    int32_t mu[kParts][3]; // part index along the field's axes, slowest first
    int32_t lo[kParts][3]; // window [lo, hi) along the same axes; lo == hi == 0 when the window misses the field
    int32_t hi[kParts][3];
    int32_t pad;
};
static_assert(sizeof(SampleWs) % 8 == 0, "workspace rows stay 8-byte aligned");

struct Params {
    int nh, nw, nl, parts, sigma, type;
    double spa[3], range[3];
};

// ---------------------------------------------------------------------------------------------------- prologue
// box_points (_construct_box_3d + _get_cam_cord: the centre and the eight corners) lives in grid_point.hpp, shared with roi_crop.hip.

// construct_mesh_cuboid: per face (p1, p2, p3, .), normal = (p2 - p1) x (p3 - p2), offset = -p1 . normal
__device__ void box_planes(const double (*pts)[3], double (*planes)[4]) {
    const int face[6][3] = {{2, 1, 3}, {8, 7, 5}, {6, 5, 1}, {4, 3, 7}, {1, 5, 7}, {8, 6, 2}};
    for (int f = 0; f < 6; ++f) {
#pragma clang fp contract(off)
        const double *p1 = pts[face[f][0]], *p2 = pts[face[f][1]], *p3 = pts[face[f][2]];
        const double ax = p2[0] - p1[0], ay = p2[1] - p1[1], az = p2[2] - p1[2];
        const double bx = p3[0] - p2[0], by = p3[1] - p2[1], bz = p3[2] - p2[2];
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        planes[f][0] = nx; planes[f][1] = ny; planes[f][2] = nz;
        planes[f][3] = -(p1[0] * nx + p1[1] * ny + p1[2] * nz);
    }
}

// floor((c + 0.5 (re - 1) spa) / spa), the index of _construct_neural_confidence_field :751-755 and _get_point_cloud :801-805
__device__ __forceinline__ double cell_of(double c, int re, double spa) {
#pragma clang fp contract(off)
    const double half = 0.5 * (double)(re - 1);
    return floor((c + half * spa) / spa);
}

__global__ void __launch_bounds__(64)
prologue_kernel(const double *__restrict__ samples, const double *__restrict__ labels, SampleWs *__restrict__ ws,
                float *__restrict__ corners_local, Params g, int N) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const double *s = samples + (int64_t)n * 7, *t = labels + (int64_t)n * 7;
    SampleWs &o = ws[n];
    double sp[9][3], gp[9][3];
    box_points(t[0], t[1], t[2], t[3], t[4], t[5], t[6], gp);
    box_planes(gp, o.gt);
    // roi_3d = sample.copy(); roi_3d[:3] = range  (:784-785): the bottom centre stays where the proposal has it
    box_points(g.range[0], g.range[1], g.range[2], s[3], s[4], s[5], s[6], sp);
    box_planes(sp, o.roi);
    o.ctr[0] = sp[0][0]; o.ctr[1] = sp[0][1]; o.ctr[2] = sp[0][2];
    const double sn = sin(s[6]), cs = cos(s[6]);
    o.sn = sn; o.cs = cs;
    // the heat maps are relative to the centre of the proposal itself (:736-737)
    box_points(s[0], s[1], s[2], s[3], s[4], s[5], s[6], sp);
    const int size[3] = {g.type == 3 ? g.nh : 1, g.type == 3 ? g.nw : g.nl, g.type == 3 ? g.nl : g.nw};
    for (int p = 0; p < g.parts; ++p) {
        double ox, oy, oz;
        {
#pragma clang fp contract(off)
            ox = gp[p][0] - sp[0][0]; oy = gp[p][1] - sp[0][1]; oz = gp[p][2] - sp[0][2];
        }
        // offset @ basis, basis = rot_y(ry) @ [[0,0,1],[0,1,0],[-1,0,0]]
        const double lx = fma(oz, -cs, fma(oy, 0.0, ox * (-sn)));
        const double ly = fma(oz, 0.0, fma(oy, 1.0, ox * 0.0));
        const double lz = fma(oz, -sn, fma(oy, 0.0, ox * cs));
        if (corners_local) {
            float *c = corners_local + ((int64_t)n * g.parts + p) * 3;
            c[0] = (float)lx; c[1] = (float)ly; c[2] = (float)lz;
        }
        const double iy = cell_of(ly, g.nh, g.spa[0]), ix = cell_of(lx, g.nw, g.spa[1]), iz = cell_of(lz, g.nl, g.spa[2]);
        const double idx[3] = {g.type == 3 ? iy : 0.0, g.type == 3 ? ix : iz, g.type == 3 ? iz : ix};
        bool any = true;
        int lo[3], hi[3], mu[3];
        for (int a = 0; a < 3; ++a) {
            // far-away parts: any index beyond +-2^30 misses every field this library accepts (a NaN index too)
            const double d = idx[a] >= -1073741824.0 && idx[a] <= 1073741824.0 ? idx[a] : -1073741824.0;
            mu[a] = (int)d;
            const int reach = (g.type == 2 && a == 0) ? 0 : 3 * g.sigma;
            lo[a] = max(0, mu[a] - reach);
            hi[a] = min(mu[a] + reach + 1, size[a]);
            any = any && hi[a] > lo[a];
        }
        for (int a = 0; a < 3; ++a) {
            o.mu[p][a] = mu[a];
            o.lo[p][a] = any ? lo[a] : 0;
            o.hi[p][a] = any ? hi[a] : 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------------- streaming stores
// A channel of S floats that starts `base` floats into a 16-byte aligned buffer: `head` single floats up to the first
// aligned address, nvec 16-byte groups, `tail` single floats.  Thread t < nvec owns group t; the next head + tail threads
// own one float each.
struct Span {
    int head, nvec, tail;
    __device__ Span(int64_t base, int S) {
        head = (int)((4 - (base & 3)) & 3);
        if (head > S) head = S;
        nvec = (S - head) >> 2;
        tail = S - head - 4 * nvec;
    }
    __device__ int threads() const { return nvec + head + tail; }
    // first element and element count (4 or 1) of thread t; count 0 if t owns nothing
    __device__ int first(int t, int &count) const {
        if (t < nvec) { count = 4; return head + 4 * t; }
        const int k = t - nvec;
        count = k < head + tail ? 1 : 0;
        return k < head ? k : 4 * nvec + k;
    }
};

__host__ __device__ inline int span_threads_bound(int S) { return S / 4 + 6; }

template <typename F>
__device__ __forceinline__ void stream_channel(float *__restrict__ out, int64_t base, int S, int t, F value) {
    const Span sp(base, S);
    int count;
    const int r = sp.first(t, count);
    if (count == 4) {
        float4 v;
        v.x = value(r); v.y = value(r + 1); v.z = value(r + 2); v.w = value(r + 3);
        *reinterpret_cast<float4 *>(out + base + r) = v;
    } else if (count == 1) {
        out[base + r] = value(r);
    }
}

__global__ void __launch_bounds__(256)
fields_kernel(const SampleWs *__restrict__ ws, float *__restrict__ out, int parts, int D1, int D2, int S, float denom) {
    const int ch = blockIdx.y, n = ch / parts, p = ch - n * parts;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const SampleWs &w = ws[n];
    const int m0 = w.mu[p][0], m1 = w.mu[p][1], m2 = w.mu[p][2];
    const int l0 = w.lo[p][0], l1 = w.lo[p][1], l2 = w.lo[p][2];
    const int h0 = w.hi[p][0], h1 = w.hi[p][1], h2 = w.hi[p][2];
    stream_channel(out, (int64_t)ch * S, S, t, [&](int r) -> float {
        const int q = r / D2, i2 = r - q * D2, i0 = q / D1, i1 = q - i0 * D1;
        if (i0 < l0 || i0 >= h0 || i1 < l1 || i1 >= h1 || i2 < l2 || i2 >= h2) return 0.0f;
        // numpy: exp(-(dx^2 + dy^2 + dz^2) / (2 sigma^2)) on float32 arrays; the exponent is rounded to float32 there
        const int d0 = i0 - m0, d1 = i1 - m1, d2 = i2 - m2;
        const float e = -(float)(d0 * d0 + d1 * d1 + d2 * d2) / denom;
        return (float)exp((double)e);
    });
}

__device__ __forceinline__ bool inside(const double (*pl)[4], double x, double y, double z) {
    bool in = true;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        // query @ plane with query = (x, y, z, 1)
        const double v = fma(1.0, pl[f][3], fma(z, pl[f][2], fma(y, pl[f][1], x * pl[f][0])));
        in = in && v < 0.0;
    }
    return in;
}

__global__ void __launch_bounds__(256)
voxel_kernel(const double *__restrict__ samples, const SampleWs *__restrict__ ws, float *__restrict__ occ, GridSpec g, int V) {
    const int n = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const GridPose pose = grid_pose(samples + (int64_t)n * 7);
    const SampleWs &w = ws[n];
    stream_channel(occ, (int64_t)n * V, V, t, [&](int r) -> float {
        const int q = r / g.nl, il = r - q * g.nl, ih = q / g.nw, iw = q - ih * g.nw;
        double X, Y, Z;
        grid_point_cam(g, pose, ih, iw, il, X, Y, Z);
        return inside(w.gt, X, Y, Z) ? -1.0f : 0.0f;
    });
}

template <typename T>
__global__ void __launch_bounds__(256)
point_kernel(const T *__restrict__ points, int64_t num_points, const int64_t *__restrict__ slices, int64_t max_points,
             const double *__restrict__ v2r, const SampleWs *__restrict__ ws, float *__restrict__ occ,
             uint8_t *__restrict__ in_roi, uint8_t *__restrict__ in_fg, Params g) {
    const int n = blockIdx.y;
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= max_points) return;
    const int64_t first = slices ? slices[2 * n] : 0, count = slices ? slices[2 * n + 1] : max_points;
    const int64_t row = first + k;
    bool roi = false, fg = false;
    if (k < count && first >= 0 && row < num_points) {
        const SampleWs &w = ws[n];
        double x = (double)points[row * 3], y = (double)points[row * 3 + 1], z = (double)points[row * 3 + 2];
        if (v2r) {
            // ref = [x y z 1] @ V2C^T; rect = R0 @ ref
            const double a = fma(1.0, v2r[3], fma(z, v2r[2], fma(y, v2r[1], x * v2r[0])));
            const double b = fma(1.0, v2r[7], fma(z, v2r[6], fma(y, v2r[5], x * v2r[4])));
            const double c = fma(1.0, v2r[11], fma(z, v2r[10], fma(y, v2r[9], x * v2r[8])));
            x = fma(v2r[14], c, fma(v2r[13], b, v2r[12] * a));
            y = fma(v2r[17], c, fma(v2r[16], b, v2r[15] * a));
            z = fma(v2r[20], c, fma(v2r[19], b, v2r[18] * a));
        }
        roi = inside(w.roi, x, y, z);
        fg = roi && inside(w.gt, x, y, z);
        if (fg) {
            double ox, oy, oz;
            {
#pragma clang fp contract(off)
                ox = x - w.ctr[0]; oy = y - w.ctr[1]; oz = z - w.ctr[2];
            }
            const double lx = fma(oz, -w.cs, fma(oy, 0.0, ox * (-w.sn)));
            const double ly = fma(oz, 0.0, fma(oy, 1.0, ox * 0.0));
            const double lz = fma(oz, -w.sn, fma(oy, 0.0, ox * w.cs));
            const double idx[3] = {cell_of(ly, g.nh, g.spa[0]), cell_of(lx, g.nw, g.spa[1]), cell_of(lz, g.nl, g.spa[2])};
            const int re[3] = {g.nh, g.nw, g.nl};
            int cell[3];
            bool ok = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // at or above the extent: the last cell (:806-814); below zero: counted from the end, as numpy indexes;
                // below -extent numpy raises IndexError: nothing is written for such a point
                const double d = idx[a];
                int c = d >= (double)re[a] ? re[a] - 1 : (d >= -(double)re[a] ? (int)d : -1 - re[a]);
                if (c < 0) c += re[a];
                ok = ok && c >= 0;
                cell[a] = c;
            }
            if (ok) {
                float *o = occ + (int64_t)n * g.nh * g.nw * g.nl + ((int64_t)cell[0] * g.nw + cell[1]) * g.nl + cell[2];
                // pass A left -1 or 0; the background (0) is written last in the reference and wins.  Every thread that
                // reaches this voxel stores the same 1.0f, and -1 and 1 both read as "not background".
                if (*o != 0.0f) *o = 1.0f;
            }
        }
    }
    if (in_roi) {
        in_roi[(int64_t)n * max_points + k] = roi ? 1 : 0;
        in_fg[(int64_t)n * max_points + k] = fg ? 1 : 0;
    }
}

int check_grid(const snvc_targets_grid *g, const char *who, Params &p) {
    if (!g) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets: null grid description");
    if (g->nh < 1 || g->nw < 1 || g->nl < 1 || (int64_t)g->nh * g->nw * g->nl > 0x7fffffe0ll) {
        set_error("%s: grid_resolution (%d, %d, %d) must be positive with fewer than 2^31 cells", who, g->nh, g->nw, g->nl);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (g->num_parts < 1 || g->num_parts > kParts) {
        set_error("%s: Only support less than or equal to 9 object parts (got %d)", who, g->num_parts);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    if (g->sigma < 1 || g->sigma > 1000 || (g->grid_type != 2 && g->grid_type != 3)) {
        set_error("%s: sigma must be an integer in 1 .. 1000 and grid_type 2 or 3 (got %d, %d)", who, g->sigma, g->grid_type);
        return SNVC_ERR_INVALID_ARGUMENT;
    }
    for (int a = 0; a < 3; ++a)
        if (!(g->spacing[a] > 0.0) || !std::isfinite(g->spacing[a]) || !std::isfinite(g->grid_range[a])) {
            set_error("%s: spacing must be positive and finite, grid_range finite", who);
            return SNVC_ERR_INVALID_ARGUMENT;
        }
    p.nh = g->nh; p.nw = g->nw; p.nl = g->nl; p.parts = g->num_parts; p.sigma = g->sigma; p.type = g->grid_type;
    for (int a = 0; a < 3; ++a) { p.spa[a] = g->spacing[a]; p.range[a] = g->grid_range[a]; }
    return SNVC_OK;
}

int check_count(int64_t N, const char *who) {
    if (N < 0) { set_error("%s: negative sample count", who); return SNVC_ERR_INVALID_ARGUMENT; }
    if (N > SNVC_TARGETS_MAX_SAMPLES) {
        set_error("%s: %lld samples is above SNVC_TARGETS_MAX_SAMPLES (%d)", who, (long long)N, SNVC_TARGETS_MAX_SAMPLES);
        return SNVC_ERR_UNSUPPORTED;
    }
    return SNVC_OK;
}

void launch_prologue(const double *samples, const double *labels, void *workspace, float *corners, const Params &p, int N,
                     hipStream_t st) {
    prologue_kernel<<<ceil_div(N, 64), 64, 0, st>>>(samples, labels, static_cast<SampleWs *>(workspace), corners, p, N);
}

}  // namespace
}  // namespace snvc

extern "C" {

int snvc_targets_abi_version(void) { return 1; }

int64_t snvc_targets_workspace_bytes(int64_t N) {
    if (N < 0 || N > SNVC_TARGETS_MAX_SAMPLES) return -1;
    return N * (int64_t)sizeof(snvc::SampleWs);
}

int snvc_targets_fields(const snvc_targets_grid *grid, const double *samples, const double *labels, int64_t N,
                        void *workspace, float *fields, float *corners_local, void *stream) {
    using namespace snvc;
    const char *who = "snvc_targets_fields";
    Params p;
    int rc = check_grid(grid, who, p);
    if (rc == SNVC_OK) rc = check_count(N, who);
    if (rc != SNVC_OK) return rc;
    if (N == 0) return SNVC_OK;
    if (!samples || !labels || !workspace || !fields || !corners_local) return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets_fields: null pointer");
    if ((reinterpret_cast<uintptr_t>(fields) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets_fields: fields must be 16-byte aligned and workspace 8-byte aligned");
    hipStream_t st = as_stream(stream);
    launch_prologue(samples, labels, workspace, corners_local, p, (int)N, st);
    rc = check_launch(who);
    if (rc != SNVC_OK) return rc;
    const int D1 = p.type == 3 ? p.nw : p.nl, D2 = p.type == 3 ? p.nl : p.nw;
    const int S = (p.type == 3 ? p.nh : 1) * D1 * D2;
    dim3 g((unsigned)ceil_div(span_threads_bound(S), 256), (unsigned)(N * p.parts));
    fields_kernel<<<g, 256, 0, st>>>(static_cast<const SampleWs *>(workspace), fields, p.parts, D1, D2, S,
                                     (float)(2 * p.sigma * p.sigma));
    return check_launch(who);
}

int snvc_targets_occupancy(const snvc_targets_grid *grid, const double *samples, const double *labels, int64_t N,
                           const void *points, int points_f64, int64_t num_points, const int64_t *slices, int64_t max_points,
                           const double *velo_to_rect, void *workspace, float *occupancy, uint8_t *in_roi, uint8_t *in_fg,
                           void *stream) {
    using namespace snvc;
    const char *who = "snvc_targets_occupancy";
    Params p;
    int rc = check_grid(grid, who, p);
    if (rc == SNVC_OK) rc = check_count(N, who);
    if (rc != SNVC_OK) return rc;
    if (num_points < 0 || max_points < 0 || max_points > num_points || max_points > 0x7fffff00ll)
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets_occupancy: need 0 <= max_points <= num_points, max_points < 2^31");
    if ((in_roi == nullptr) != (in_fg == nullptr))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets_occupancy: in_roi and in_fg come together or not at all");
    if (N == 0) return SNVC_OK;
    if (!samples || !labels || !workspace || !occupancy || (max_points > 0 && !points))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets_occupancy: null pointer");
    if ((reinterpret_cast<uintptr_t>(occupancy) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 7))
        return fail(SNVC_ERR_INVALID_ARGUMENT, "snvc_targets_occupancy: occupancy must be 16-byte aligned and workspace 8-byte aligned");
    hipStream_t st = as_stream(stream);
    launch_prologue(samples, labels, workspace, nullptr, p, (int)N, st);
    rc = check_launch(who);
    if (rc != SNVC_OK) return rc;
    const GridSpec gs = make_grid_spec(grid->ranges, p.nh, p.nw, p.nl);
    const int V = p.nh * p.nw * p.nl;
    const SampleWs *ws = static_cast<const SampleWs *>(workspace);
    dim3 ga((unsigned)ceil_div(span_threads_bound(V), 256), (unsigned)N);
    voxel_kernel<<<ga, 256, 0, st>>>(samples, ws, occupancy, gs, V);
    rc = check_launch(who);
    if (rc != SNVC_OK || max_points == 0) return rc;
    dim3 gb((unsigned)ceil_div<int64_t>(max_points, 256), (unsigned)N);
    if (points_f64)
        point_kernel<double><<<gb, 256, 0, st>>>(static_cast<const double *>(points), num_points, slices, max_points, velo_to_rect, ws,
                                                 occupancy, in_roi, in_fg, p);
    else
        point_kernel<float><<<gb, 256, 0, st>>>(static_cast<const float *>(points), num_points, slices, max_points, velo_to_rect, ws,
                                                occupancy, in_roi, in_fg, p);
    return check_launch(who);
}

}  // extern "C"
