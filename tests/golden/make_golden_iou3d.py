#!/usr/bin/env python3
"""Golden vectors of the rotated-box IoU / NMS family from the REFERENCE'S OWN compiled C++.

Run where the reference checkout exists (default /root/reference, or $SNVC_REFERENCE):
    python tests/golden/make_golden_iou3d.py
It compiles snvc/extension/iou3d_nms/src/iou3d_cpu.cpp WHERE IT LIES (never copied) into a temporary directory with g++
against this image's libtorch, with `-D__device__=` and two empty stand-ins for cuda.h / cuda_runtime_api.h, binds its
`boxes_iou_bev_cpu` through a three-line pybind TU written here, and writes tests/golden/iou3d_ref.npz (data only):

  bev_<case>_{a,b,iou,overlap,iou3d,valid}   BEV IoU matrices of the reference; overlap and 3D IoU derived from it in
                                            float64 (s = iou (sa + sb) / (1 + iou), then the height formula of
                                            iou3d_nms_utils.py:53-85); `valid` = pair not rounding-level (below)
  nms_<N>_<thresh>_{boxes,scores}          a scene of N boxes, distinct scores
  nms_<N>_<thresh>_<kind>_keep              indices into boxes kept by greedy NMS (rank order); rotated takes its IoU
                                            from the reference's CPU function, `normal` is computed in fp32 numpy from
                                            the axis-aligned formula (iou3d_nms_kernel.cu:343-355); row convention:
                                            box i (higher score) suppresses j when iou(box_i, box_j) > thresh
  jac_{a,b,grad,bev,valid}                  one-by-one pairs, the reference's BEV IoU of the 15 configurations each
                                            (0: as given; 1 + 2k: a[:, k] = fp32(a - 1e-3); 2 + 2k: fp32(a + 1e-3))
  dropped_*                                 how many cases were dropped as rounding-level

Rounding-level: a pair any of whose corners lies within 1e-5 (float64) of the other box's grown (1e-2) boundary, in any
evaluated configuration, is marked invalid, and so is a pair whose reference IoU is more than 1e-5 (Jacobian pairs: 1e-6)
off a float64 evaluation of the same definition (the reference rounds corners in absolute fp32 coordinates: up to
~2.6e-5 for pedestrian-sized boxes at 50-70 m); a box is removed from an NMS scene (drawn with 64 spare
boxes) when its decision depends on such a pair or on an IoU within 1e-4 of the threshold (a kept box i above it, and
no other kept box that suppresses it beyond doubt); the scene is then its N best-ranked boxes.
"""
import os
import subprocess
import sys
import sysconfig
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")
SRC = os.path.join(REF, "snvc", "extension", "iou3d_nms", "src", "iou3d_cpu.cpp")
MARGIN, NEAR, THRESH_GAP, EPS = 1e-2, 1e-5, 1e-4, 1e-3
THRESHOLDS = (0.01, 0.1, 0.5, 0.7)
NMS_SIZES = (1, 63, 64, 65, 200, 1000, 4096)

BIND = """#include <torch/extension.h>
int boxes_iou_bev_cpu(at::Tensor boxes_a_tensor, at::Tensor boxes_b_tensor, at::Tensor ans_iou_tensor);
PYBIND11_MODULE(ref_iou3d_cpu, m) { m.def("boxes_iou_bev_cpu", &boxes_iou_bev_cpu); }
"""


def build_reference(tmp):
    import torch.utils.cpp_extension as ce
    for stub in ("cuda.h", "cuda_runtime_api.h"):
        open(os.path.join(tmp, stub), "w").close()
    bind = os.path.join(tmp, "bind.cpp")
    with open(bind, "w") as f:
        f.write(BIND)
    out = os.path.join(tmp, "ref_iou3d_cpu" + sysconfig.get_config_var("EXT_SUFFIX"))
    inc = [f"-I{p}" for p in ce.include_paths() + [sysconfig.get_paths()["include"]]]
    libs = [x for p in ce.library_paths() for x in (f"-L{p}", f"-Wl,-rpath,{p}")]
    cmd = (["g++", "-O2", "-shared", "-fPIC", "-std=c++17", "-w", "-D__device__=", "-DTORCH_API_INCLUDE_EXTENSION_H", f"-I{tmp}"]
           + inc + [SRC, bind, "-o", out] + libs + ["-ltorch", "-ltorch_cpu", "-lc10", "-ltorch_python"])
    subprocess.check_call(cmd)
    sys.path.insert(0, tmp)
    import torch  # noqa: F401  (libtorch symbols for the module)
    import ref_iou3d_cpu
    return ref_iou3d_cpu


def ref_iou(mod, a, b):
    import torch
    out = torch.zeros((len(a), len(b)), dtype=torch.float32)
    if len(a) and len(b):
        mod.boxes_iou_bev_cpu(torch.from_numpy(np.ascontiguousarray(a, np.float32)),
                              torch.from_numpy(np.ascontiguousarray(b, np.float32)), out)
    return out.numpy()


# ------------------------------------------------------------------------------------------------------ float64 helpers
def corners(b):
    """(n, 7) -> (n, 4, 2) float64 corners."""
    b = b.astype(np.float64)
    sx, sy = np.array([-1, 1, 1, -1.0]), np.array([-1, -1, 1, 1.0])
    lx, ly = sx[None] * b[:, 3:4] / 2, sy[None] * b[:, 4:5] / 2
    c, s = np.cos(b[:, 6:7]), np.sin(b[:, 6:7])
    return np.stack([b[:, 0:1] + lx * c - ly * s, b[:, 1:2] + lx * s + ly * c], -1)


def near_boundary(a, b):
    """(n, 7), (m, 7) -> (n, m) bool: some corner of one box within NEAR of the other's grown boundary."""
    def one_way(p, q):   # corners of q in p's frame
        cq = corners(q)                                          # (m, 4, 2)
        p = p.astype(np.float64)
        rx = cq[None, :, :, 0] - p[:, None, None, 0]
        ry = cq[None, :, :, 1] - p[:, None, None, 1]
        c, s = np.cos(p[:, 6])[:, None, None], np.sin(p[:, 6])[:, None, None]
        lx, ly = np.abs(rx * c + ry * s), np.abs(-rx * s + ry * c)
        gx, gy = (p[:, 3] / 2 + MARGIN)[:, None, None], (p[:, 4] / 2 + MARGIN)[:, None, None]
        nx = (np.abs(lx - gx) < NEAR) & (ly < gy + NEAR)
        ny = (np.abs(ly - gy) < NEAR) & (lx < gx + NEAR)
        return (nx | ny).any(-1)
    return one_way(a, b) | one_way(b, a).T


def overlap64(p, q):
    """The BEV overlap DEFINITION (crossings + corners inside the grown box, shoelace in angular order) in float64."""
    cp, cq = corners(p[None])[0], corners(q[None])[0]
    cr = lambda u, v: u[0] * v[1] - u[1] * v[0]   # noqa: E731
    pts = []
    for i in range(4):
        p0, p1 = cp[i], cp[(i + 1) % 4]
        for j in range(4):
            q0, q1 = cq[j], cq[(j + 1) % 4]
            o1, o2 = cr(p1 - p0, q0 - p0), cr(p1 - p0, q1 - p0)
            o3, o4 = cr(q1 - q0, p0 - q0), cr(q1 - q0, p1 - q0)
            if o1 * o2 < 0 and o3 * o4 < 0:
                pts.append(p0 + o3 / (o3 - o4) * (p1 - p0))

    def inside(bx, pt):
        bx = bx.astype(np.float64)
        d = pt - bx[:2]
        c, s = np.cos(bx[6]), np.sin(bx[6])
        return abs(d[0] * c + d[1] * s) < bx[3] / 2 + MARGIN and abs(-d[0] * s + d[1] * c) < bx[4] / 2 + MARGIN
    for k in range(4):
        if inside(p, cq[k]):
            pts.append(cq[k])
        if inside(q, cp[k]):
            pts.append(cp[k])
    if len(pts) < 3:
        return 0.0
    P = np.array(pts)
    P = P - P.mean(0)
    P = P[np.argsort(np.arctan2(P[:, 1], P[:, 0]))]
    return abs(np.sum(P[:, 0] * np.roll(P[:, 1], -1) - np.roll(P[:, 0], -1) * P[:, 1])) / 2


def ref_rounding(a, b, iou, cand, tol):
    """(n, m) bool: pairs among `cand` where the reference's fp32 IoU is more than `tol` off the float64 evaluation of its
    own definition (small boxes far from the origin: its corners are absolute fp32 coordinates)."""
    out = np.zeros(iou.shape, bool)
    for i, j in zip(*np.nonzero(cand)):
        s = overlap64(a[i], b[j])
        sa, sb = float(a[i, 3]) * float(a[i, 4]), float(b[j, 3]) * float(b[j, 4])
        out[i, j] = abs(iou[i, j] - s / max(sa + sb - s, 1e-8)) > tol
    return out


def iou_ours_upper_bound(a, b):
    """> 0 where the grown boxes' circumcircles meet (a superset of the pairs with any overlap)."""
    r = lambda x: np.hypot(x[:, 3] / 2 + MARGIN, x[:, 4] / 2 + MARGIN).astype(np.float64)   # noqa: E731
    d = np.hypot(a[:, None, 0] - b[None, :, 0], a[:, None, 1] - b[None, :, 1])
    return (d <= (r(a)[:, None] + r(b)[None]) * 1.01 + 1e-3).astype(np.float64)


def derived(a, b, iou):
    """float64 overlap and 3D IoU from the reference's BEV IoU (iou3d_nms_utils.py:53-85)."""
    a, b, iou = a.astype(np.float64), b.astype(np.float64), iou.astype(np.float64)
    sa, sb = (a[:, 3] * a[:, 4])[:, None], (b[:, 3] * b[:, 4])[None]
    ov = iou * (sa + sb) / (1 + iou)
    hmax = np.minimum((a[:, 2] + a[:, 5] / 2)[:, None], (b[:, 2] + b[:, 5] / 2)[None])
    hmin = np.maximum((a[:, 2] - a[:, 5] / 2)[:, None], (b[:, 2] - b[:, 5] / 2)[None])
    o3 = ov * np.clip(hmax - hmin, 0, None)
    va, vb = (a[:, 3] * a[:, 4] * a[:, 5])[:, None], (b[:, 3] * b[:, 4] * b[:, 5])[None]
    return ov, o3 / np.maximum(va + vb - o3, 1e-6)


def iou_normal_f32(a, b):
    a, b = a.astype(np.float32), b.astype(np.float32)
    h = np.float32(2)
    left = np.maximum((a[:, 0] - a[:, 3] / h)[:, None], (b[:, 0] - b[:, 3] / h)[None])
    right = np.minimum((a[:, 0] + a[:, 3] / h)[:, None], (b[:, 0] + b[:, 3] / h)[None])
    top = np.maximum((a[:, 1] - a[:, 4] / h)[:, None], (b[:, 1] - b[:, 4] / h)[None])
    bottom = np.minimum((a[:, 1] + a[:, 4] / h)[:, None], (b[:, 1] + b[:, 4] / h)[None])
    inter = np.maximum(right - left, np.float32(0)) * np.maximum(bottom - top, np.float32(0))
    union = (a[:, 3] * a[:, 4])[:, None] + (b[:, 3] * b[:, 4])[None] - inter
    return inter / np.maximum(union, np.float32(1e-8))


# ------------------------------------------------------------------------------------------------------ scenes
DIMS = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]])


def kitti_scene(rng, n, dup=6):
    """n boxes: n / dup KITTI-sized objects (car / pedestrian / cyclist) in front of the sensor, each box a jittered
    duplicate of one of them (what a detector's proposals look like before NMS)."""
    k = max(1, n // dup)
    cls = rng.choice(3, k, p=[0.7, 0.2, 0.1])
    obj = np.concatenate([rng.uniform(0, 70, (k, 1)), rng.uniform(-40, 40, (k, 1)), rng.uniform(-2.5, 0.5, (k, 1)),
                          DIMS[cls], rng.uniform(-np.pi, np.pi, (k, 1))], 1)
    pick = obj[rng.integers(0, k, n)]
    jit = np.concatenate([rng.normal(0, 0.25, (n, 2)), rng.normal(0, 0.1, (n, 1)),
                          pick[:, 3:6] * rng.normal(0, 0.08, (n, 3)), rng.normal(0, 0.15, (n, 1))], 1)
    return (pick + jit).astype(np.float32)


def edge_boxes():
    """Hand-made configurations: identical boxes, quarter turns, nested, touching, 5 mm gaps, corners 9e-3 / 1.1e-2
    outside the other box, zero size, far apart."""
    e = []
    base = [0, 0, 0, 2, 2, 2, 0]
    e += [base, [0, 0, 0, 2, 2, 2, 0], [10, 10, 1, 4, 2, 1.5, 0.7], [10, 10, 1, 4, 2, 1.5, 0.7]]       # identical pairs
    e += [[20, 0, 0, 4, 2, 1.5, q * np.pi / 2] for q in range(5)]                                      # quarter turns
    e += [[30, 0, 0, 6, 4, 2, 0.3], [30.2, 0.1, 0, 2, 1, 1, 1.1], [30, 0, 0, 1, 1, 3, 0]]               # nested
    e += [[2, 0, 0, 2, 2, 2, 0], [2, 2, 0, 2, 2, 2, 0], [0, 2, 0.5, 2, 2, 1, 0]]                         # touching base
    e += [[2.005, 0, 0, 2, 2, 2, 0], [0, -2.005, 0, 2, 2, 2, 0]]                                         # 5 mm gaps
    for off in (9e-3, 1.1e-2):                                                                           # corner probes
        d = 1 + off + np.sqrt(2) / 2                      # a unit square turned 45 deg, its corner `off` outside base
        e += [[d, 0.3, 0, 1, 1, 1, np.pi / 4], [-0.3, -d, 0, 1, 1, 1, np.pi / 4]]
    e += [[0, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 2, 2, 0], [0.05, 0.05, 0, 1e-2, 1e-2, 1e-2, 0.2]]           # zero / tiny
    e += [[1000, -1000, 5, 2, 2, 2, 0], [-70, 40, 0, 4, 2, 1.5, 3.0]]                                    # far apart
    e += [[45.3, -12.1, -1, 3.9, 1.6, 1.5, 1.2], [45.9, -11.8, -0.8, 4.1, 1.7, 1.6, 1.35]]               # far, overlapping
    return np.array(e, np.float32)


def greedy(iou_sorted, thresh):
    n = len(iou_sorted)
    removed = np.zeros(n, bool)
    keep = []
    for i in range(n):
        if not removed[i]:
            keep.append(i)
            removed[i + 1:] |= iou_sorted[i, i + 1:] > thresh
    return np.array(keep, np.int64)


def harmful(iou_sorted, uncertain_pair, keep, thresh):
    """Ranks j whose NMS decision depends on a rounding-level pair: a kept box i above j whose pair is uncertain (IoU
    within THRESH_GAP of the threshold, or a rounding-level corner) while no other kept box suppresses j beyond doubt."""
    n = len(iou_sorted)
    kept = np.zeros(n, bool)
    kept[keep] = True
    unc = (np.abs(iou_sorted - thresh) <= THRESH_GAP) | uncertain_pair
    rel = np.triu(np.ones((n, n), bool), 1) & kept[:, None]       # pairs (kept i, later j)
    robust_sup = (rel & ~unc & (iou_sorted > thresh)).any(0)
    return np.nonzero((rel & unc).any(0) & ~robust_sup)[0]


def main():
    if not os.path.exists(SRC):
        sys.exit(f"{SRC} missing: this script needs the reference checkout")
    tmp = tempfile.mkdtemp(prefix="snvc_iou3d_ref_")
    mod = build_reference(tmp)
    blob, dropped = {}, {}

    # BEV IoU matrices: edge set against itself, seeded scenes (sizes not multiples of 64, N != M)
    cases = {"edge": (edge_boxes(), edge_boxes())}
    rng = np.random.default_rng(20261015)
    for name, (n, m) in {"kitti0": (300, 300), "kitti1": (200, 130), "kitti2": (97, 250)}.items():
        a = kitti_scene(rng, n)
        b = np.concatenate([a[: m // 2], kitti_scene(rng, m - m // 2)]) if m > 1 else a[:m]
        cases[name] = (a, b)
    nd = nr = 0
    for name, (a, b) in cases.items():
        iou = ref_iou(mod, a, b)
        ov, i3 = derived(a, b, iou)
        rounding = ref_rounding(a, b, iou, (iou > 0) | (iou_ours_upper_bound(a, b) > 0), 1e-5)
        valid = ~near_boundary(a, b) & ~rounding
        nr += int(rounding.sum())
        nd += int((~valid).sum())
        blob.update({f"bev_{name}_a": a, f"bev_{name}_b": b, f"bev_{name}_iou": iou, f"bev_{name}_overlap": ov.astype(np.float32),
                     f"bev_{name}_iou3d": i3.astype(np.float32), f"bev_{name}_valid": valid})
        print(f"bev {name}: {a.shape[0]}x{b.shape[0]}, {int((iou > 0).sum())} overlapping, {int((~valid).sum())} dropped")
    dropped["dropped_bev_pairs"] = nd
    dropped["dropped_bev_pairs_reference_rounding"] = nr

    # NMS scenes, one per (N, threshold), valid for both kinds: draw N + 64 boxes, remove every box whose decision depends
    # on a rounding-level pair (decisions above it do not change; below it they are re-checked), keep the N best-ranked
    nd = 0
    for n in NMS_SIZES:
        for t in THRESHOLDS:
            boxes = kitti_scene(rng, n + 64)
            scores = (rng.permutation(n + 64) + rng.uniform(0.1, 0.9, n + 64)).astype(np.float32) / (n + 64)   # distinct
            order = np.argsort(-scores, kind="stable")
            removed = 0
            while True:
                sb = boxes[order]
                unc = near_boundary(sb, sb) if len(sb) <= 1100 else near_boundary_sparse(sb)
                mats = {"rotated": (ref_iou(mod, sb, sb), unc), "normal": (iou_normal_f32(sb, sb), np.zeros_like(unc))}
                bad = np.unique(np.concatenate([harmful(m, u, greedy(m, t), t) for m, u in mats.values()]))
                bad = bad[bad < n]                                  # ranks past n are cut anyway
                if not len(bad):
                    break
                order = np.delete(order, bad)
                removed += len(bad)
                if len(order) < n:
                    sys.exit(f"nms {n} @ {t}: too many rounding-level decisions")
            keep_set = order[:n]
            keeps = {}
            for kind, (m, u) in mats.items():
                m, u = m[:n, :n], u[:n, :n]
                k = greedy(m, t)
                assert not len(harmful(m, u, k, t))
                keeps[f"nms_{n}_{t}_{kind}_keep"] = k                  # ranks within the kept set for now
            idx = np.sort(keep_set)                                   # stored in draw order, not rank order
            pos = {int(o): p for p, o in enumerate(idx)}
            for key, k in keeps.items():
                keeps[key] = np.array([pos[int(keep_set[r])] for r in k], np.int64)
            nd += removed
            blob[f"nms_{n}_{t}_boxes"], blob[f"nms_{n}_{t}_scores"] = boxes[idx], scores[idx]
            blob.update(keeps)
            print(f"nms {n} @ {t}: kept " + ", ".join(f"{k.split('_')[3]}={len(v)}" for k, v in keeps.items())
                  + f" ({removed} boxes removed)")
    dropped["dropped_nms_boxes"] = nd

    # Jacobian pairs: b near a (the reference's own self-test draws rand * 6 and + rand * 0.1), plus KITTI-like pairs
    k = kitti_scene(rng, 48)
    k[:, :2] -= k[:, :2].mean(0)                          # KITTI-sized boxes, centred within a few metres of the origin
    k[:, :2] *= 0.1
    a = np.concatenate([rng.random((48, 7)) * 6, k]).astype(np.float32)
    a[:48, 3:6] += 0.5
    b = (a + np.concatenate([rng.random((48, 7)) * 0.1, rng.normal(0, 0.2, (48, 7))]) * np.float32(1)).astype(np.float32)
    b[:, 3:6] = np.abs(b[:, 3:6])
    configs = [a]
    for k in range(7):
        for sign in (-1, 1):
            x = a.copy()
            x[:, k] = (a[:, k] + np.float32(sign * EPS)).astype(np.float32)   # fp32 orig -/+ eps, as the torch code
            configs.append(x)
    bev = np.stack([np.diag(ref_iou(mod, x, b)) for x in configs], 1)          # (n, 15)
    valid = ~np.stack([np.diag(near_boundary(x, b)) for x in configs], 1).any(1)
    eye = np.eye(len(a), dtype=bool)
    for c, x in enumerate(configs):      # central differences amplify the reference's rounding by 1 / (2 eps)
        valid &= ~np.diag(ref_rounding(x, b, np.diag(bev[:, c]), eye, 1e-6))
    blob.update({"jac_a": a, "jac_b": b, "jac_grad": rng.normal(0, 1, len(a)).astype(np.float32), "jac_bev": bev, "jac_valid": valid})
    dropped["dropped_jac_pairs"] = int((~valid).sum())
    print(f"jac: {len(a)} pairs, {int((bev[:, 0] > 0).sum())} overlapping, {int((~valid).sum())} dropped")

    blob.update({k: np.int64(v) for k, v in dropped.items()})
    path = os.path.join(ROOT, "tests", "golden", "iou3d_ref.npz")
    np.savez_compressed(path, **blob)
    print("wrote", path, os.path.getsize(path), "bytes;", dropped)


def near_boundary_sparse(b):
    """near_boundary(b, b) for large n, evaluated only where the grown boxes' circumcircles meet."""
    n = len(b)
    out = np.zeros((n, n), bool)
    r = np.hypot(b[:, 3] / 2 + MARGIN, b[:, 4] / 2 + MARGIN).astype(np.float64)
    for i in range(0, n, 256):
        d = np.hypot(b[i:i + 256, None, 0] - b[None, :, 0], b[i:i + 256, None, 1] - b[None, :, 1])
        ii, jj = np.nonzero(d <= (r[i:i + 256, None] + r[None]) * 1.01 + 1e-3)
        ii += i
        if len(ii):
            out[ii, jj] = np.diagonal(near_boundary(b[ii], b[jj])) if len(ii) < 2000 else _pairwise_near(b, ii, jj)
    return out


def _pairwise_near(b, ii, jj):
    return np.concatenate([np.diagonal(near_boundary(b[ii[k:k + 1000]], b[jj[k:k + 1000]])) for k in range(0, len(ii), 1000)])


if __name__ == "__main__":
    main()
