"""numpy restatement of the RoI cropper's specification ("RoI crops"; include/snvc_roicrop.h): float64 geometry,
the 5-fractional-bit integer warp, the 'exact' warp and torch-CPU normalisation.  Written from the specification, not routed
through snvc_amd; the host test holds it to the golden geometry and to hand answers, the GPU test holds the kernels to it.
"""
import numpy as np
import torch

ENLARGE = 1.1
SAT = 2.0 ** 60


def rotation_y(ry):
    c, s = np.cos(ry), np.sin(ry)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def box_points(box):
    """[9,3]: centre + 8 corners of (h, w, l, x, y, z, ry); the extents are displaced by their float32 rounding."""
    h, w, l = box[0], box[1], box[2]
    sx = np.array([0.5, 1, 1, 1, 1, 0, 0, 0, 0]) * l - float(np.float32(l)) / 2
    sy = np.array([0.5, 0, 1, 0, 1, 0, 1, 0, 1]) * h - float(np.float32(h))
    sz = np.array([0.5, 1, 1, 0, 0, 1, 1, 0, 0]) * w - float(np.float32(w)) / 2
    return (rotation_y(box[6]) @ np.stack([sx, sy, sz]) + np.asarray(box[3:6], dtype=np.float64).reshape(3, 1)).T


def keypoints(sample, P, grid_range):
    """[9,2] float64: the projected points of the RoI box (the sample with its size replaced by grid_range)."""
    box = np.array(sample, dtype=np.float64)
    centre_y = box[4] - box[0] * 0.5
    box[:3] = grid_range
    box[4] = centre_y + box[0] * 0.5
    hom = np.hstack([box_points(box), np.ones((9, 1))]) @ np.asarray(P, dtype=np.float64).reshape(3, 4).T
    return hom[:, :2] / hom[:, 2:3]


def centre_size(kpts, aspect_ratio):
    lo, hi = kpts.min(axis=0), kpts.max(axis=0)
    centre = (lo + hi) / 2
    w, h = (hi - lo) * ENLARGE
    if h / w > aspect_ratio:
        w = h * (1 / aspect_ratio)
    else:
        h = w * aspect_ratio
    return centre, (w, h)


def affine(centre, src_w, resolution):
    """The closed form of the three-point solve, from the float32-rounded points.  float64 [2,3]."""
    f32 = np.float32
    wr, hr = resolution
    cxf, cyf = f32(centre[0]), f32(centre[1])
    s1y = f32(centre[1] + src_w * -0.5)
    dy = f32(cyf - s1y)
    c2x = f32(cxf - dy)
    kx = (0.5 * wr) / (float(cxf) - float(c2x))
    ky = (0.5 * wr) / (float(cyf) - float(s1y))
    return np.array([[kx, 0.0, 0.5 * wr - kx * float(cxf)], [0.0, ky, 0.5 * hr - ky * float(cyf)]])


def geometry(sample, P, grid_range, aspect_ratio, resolution):
    """(kpts_2d [9,2] float64, trans [2,3] float64, kpts_2d_local [9,2] float32)."""
    kpts = keypoints(sample, P, grid_range)
    centre, size = centre_size(kpts, aspect_ratio)
    trans = affine(centre, size[0], resolution)
    local = (trans @ np.hstack([kpts, np.ones((9, 1))]).T).astype(np.float32).T
    return kpts, trans, local


def invert(trans):
    """The six inverse coefficients, in the specification's order of operations."""
    (t00, t01, t02), (t10, t11, t12) = np.asarray(trans, dtype=np.float64).tolist()
    D = t00 * t11 - t01 * t10
    D = 1.0 / D if D != 0 else 0.0
    m00, m11, m01, m10 = t11 * D, t00 * D, -t01 * D, -t10 * D
    return m00, m01, -m00 * t02 - m01 * t12, m10, m11, -m10 * t02 - m11 * t12


def fixed_arguments(trans, resolution):
    """The four arrays handed to R(.) for a crop: two per axis, (per row [Hr], per column [Wr])."""
    m00, m01, m02, m10, m11, m12 = invert(trans)
    u, v = np.arange(resolution[0], dtype=np.float64), np.arange(resolution[1], dtype=np.float64)
    return (m01 * v + m02) * 1024, m00 * u * 1024, (m11 * v + m12) * 1024, m10 * u * 1024


def _round(x):
    x = np.where(np.isnan(x), -SAT, np.clip(x, -SAT, SAT))
    return np.rint(x).astype(np.int64)


def _taps(img, sy, sx):
    """img[sy, sx] as int64 [Hr,Wr,3], zero where the index is outside."""
    h, w = img.shape[:2]
    ok = (sy >= 0) & (sy < h) & (sx >= 0) & (sx < w)
    out = img[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)].astype(np.int64)
    out[~ok] = 0
    return out


def warp_fixed5(img, trans, resolution):
    """uint8 [Hr,Wr,3]."""
    bx, ax_, by, ay_ = (_round(a) for a in fixed_arguments(trans, resolution))
    X = (bx[:, None] + 16 + ax_[None, :]) >> 5
    Y = (by[:, None] + 16 + ay_[None, :]) >> 5
    sx, ax, sy, ay = X >> 5, (X & 31)[..., None], Y >> 5, (Y & 31)[..., None]
    acc = ((32 - ax) * (32 - ay) * _taps(img, sy, sx) + ax * (32 - ay) * _taps(img, sy, sx + 1)
           + (32 - ax) * ay * _taps(img, sy + 1, sx) + ax * ay * _taps(img, sy + 1, sx + 1))
    return ((32 * acc + 16384) >> 15).astype(np.uint8)


def exact_coordinates(trans, resolution):
    m00, m01, m02, m10, m11, m12 = invert(trans)
    u, v = np.arange(resolution[0], dtype=np.float64)[None, :], np.arange(resolution[1], dtype=np.float64)[:, None]
    return m00 * u + (m01 * v + m02), m10 * u + (m11 * v + m12)


def warp_exact(img, trans, resolution):
    """uint8 [Hr,Wr,3]: float64 source coordinates, float32 blend, round to nearest (ties to even), clamp."""
    xs, ys = exact_coordinates(trans, resolution)
    ok = (np.abs(xs) < 2.0 ** 31) & (np.abs(ys) < 2.0 ** 31)       # False for NaN
    xs, ys = np.where(ok, xs, 0.0), np.where(ok, ys, 0.0)
    fx, fy = np.floor(xs), np.floor(ys)
    ax, ay = (xs - fx).astype(np.float32)[..., None], (ys - fy).astype(np.float32)[..., None]
    sx, sy = fx.astype(np.int64), fy.astype(np.int64)
    one = np.float32(1)
    p = [_taps(img, sy + j, sx + i).astype(np.float32) for j in (0, 1) for i in (0, 1)]
    top = p[0] * (one - ax) + p[1] * ax
    bot = p[2] * (one - ax) + p[3] * ax
    val = top * (one - ay) + bot * ay
    assert val.dtype == np.float32
    out = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    out[~ok] = 0
    return out


def warp(img, trans, resolution, interpolation="fixed5"):
    return {"fixed5": warp_fixed5, "exact": warp_exact}[interpolation](np.asarray(img), trans, resolution)


def normalise(crop_u8, mean, std):
    """ToTensor + Normalize with torch's CPU operations: uint8 [Hr,Wr,3] -> float32 tensor [3,Hr,Wr]."""
    t = torch.from_numpy(np.ascontiguousarray(crop_u8)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32).reshape(3, 1, 1)
    s = torch.as_tensor(std, dtype=torch.float32).reshape(3, 1, 1)
    return t.sub_(m).div_(s)


def crop(sample, img, P, cfg, interpolation="fixed5", channel_order="rgb"):
    """One side of one sample: (uint8 planar [3,Hr,Wr], kpts, trans, local)."""
    kpts, trans, local = geometry(sample, P, cfg.grid_range, cfg.aspect_ratio, cfg.resolution)
    img = np.asarray(img)
    if channel_order == "bgr":
        img = img[:, :, ::-1]
    out = warp(img, trans, cfg.resolution, interpolation)
    return np.ascontiguousarray(out.transpose(2, 0, 1)), kpts, trans, local
