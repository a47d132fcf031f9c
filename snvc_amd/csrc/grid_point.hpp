// The Vernier sampling grid in camera coordinates, shared by grid_projection.hip (the projected coordinates) and
// targets.hip (the occupancy background test), so that both see the same float64 grid point; and the nine points of a box,
// shared by targets.hip and roi_crop.hip.
//
// Reference: refinementDataset._init_3d_grid / _to_cam (snvc/dataset/KITTIRefinement_dataset.py:267-282,828-846).
// Arithmetic is fp64 in the reference's operation order (products summed k-ascending the way a BLAS micro-kernel does,
// with FMA; the translation is a separately rounded add).
#pragma once
#include "common.hpp"

namespace snvc {

struct GridSpec {
    double x0, xs, x1, y0, ys, y1, z0, zs, z1;   // start, step, stop per axis (numpy.linspace)
    int nh, nw, nl;
};

// ranges_host = (x_min, x_max, y_min, y_max, z_min, z_max); numpy.linspace: step = (stop - start) / (num - 1)
inline GridSpec make_grid_spec(const double *ranges_host, int nh, int nw, int nl) {
    GridSpec g;
    g.nh = nh; g.nw = nw; g.nl = nl;
    g.x0 = ranges_host[0]; g.x1 = ranges_host[1]; g.xs = nw > 1 ? (g.x1 - g.x0) / (double)(nw - 1) : 0.0;
    g.y0 = ranges_host[2]; g.y1 = ranges_host[3]; g.ys = nh > 1 ? (g.y1 - g.y0) / (double)(nh - 1) : 0.0;
    g.z0 = ranges_host[4]; g.z1 = ranges_host[5]; g.zs = nl > 1 ? (g.z1 - g.z0) / (double)(nl - 1) : 0.0;
    return g;
}

__device__ __forceinline__ double lin(int i, int n, double start, double step, double stop) {
#pragma clang fp contract(off)
    if (n > 1 && i == n - 1) return stop;     // numpy pins the end point
    return (double)i * step + start;
}

// Rotation (cos, sin of ry + pi/2) and translation of _to_cam for the proposal `s` = (h, w, l, x, y, z, ry).
struct GridPose {
    double c, sn, cx, cy, cz;
};

__device__ __forceinline__ GridPose grid_pose(const double *__restrict__ s) {
    GridPose p;
    double ry;
    {
#pragma clang fp contract(off)
        ry = s[6] + 0.5 * 3.141592653589793;
        p.cx = s[3];
        p.cy = s[4] - s[0] * 0.5;
        p.cz = s[5];
    }
    p.c = cos(ry);
    p.sn = sin(ry);
    return p;
}

// Grid point (ih, iw, il) of the [nh][nw][nl] grid in camera coordinates.
__device__ __forceinline__ void grid_point_cam(const GridSpec &g, const GridPose &p, int ih, int iw, int il, double &X, double &Y,
                                               double &Z) {
    const double gx = lin(iw, g.nw, g.x0, g.xs, g.x1);
    const double gy = lin(ih, g.nh, g.y0, g.ys, g.y1);
    const double gz = lin(il, g.nl, g.z0, g.zs, g.z1);
    // rot @ pts (k-ascending FMA chain), then + translation (separately rounded add)
    X = fma(p.sn, gz, fma(0.0, gy, p.c * gx));
    Y = fma(0.0, gz, fma(1.0, gy, 0.0 * gx));
    Z = fma(p.c, gz, fma(0.0, gy, (-p.sn) * gx));
    {
#pragma clang fp contract(off)
        X = X + p.cx; Y = Y + p.cy; Z = Z + p.cz;
    }
}

// Shared by targets.hip (the RoI box, the label and the proposal) and roi_crop.hip (the RoI box whose projection is the crop).
// _construct_box_3d + _get_cam_cord: the centre and the eight corners.  The reference subtracts numpy.float32(l) / 2,
// numpy.float32(h) and numpy.float32(w) / 2 from float64 lists, so the box is displaced by the float32 rounding of its size.
__device__ inline void box_points(double h, double w, double l, double x, double y, double z, double ry, double (*pts)[3]) {
    const double lf = (double)((float)l * 0.5f), hf = (double)(float)h, wf = (double)((float)w * 0.5f);
    const double xs[9] = {0.5 * l, l, l, l, l, 0, 0, 0, 0};
    const double ys[9] = {0.5 * h, 0, h, 0, h, 0, h, 0, h};
    const double zs[9] = {0.5 * w, w, w, 0, 0, w, w, 0, 0};
    const double c = cos(ry), s = sin(ry);
    for (int k = 0; k < 9; ++k) {
        double cx, cy, cz;
        {
#pragma clang fp contract(off)
            cx = xs[k] - lf; cy = ys[k] - hf; cz = zs[k] - wf;
        }
        double X = fma(s, cz, fma(0.0, cy, c * cx));
        double Y = fma(0.0, cz, fma(1.0, cy, 0.0 * cx));
        double Z = fma(c, cz, fma(0.0, cy, (-s) * cx));
        {
#pragma clang fp contract(off)
            pts[k][0] = X + x; pts[k][1] = Y + y; pts[k][2] = Z + z;
        }
    }
}

}  // namespace snvc
