"""Seeded inputs of the device read-out's cases (snvc_amd.decode.refine_boxes), shared by tests/test_decode_device_host.py,
which checks with the host route that each case means what it is there for, and tests/test_gpu_decode.py, which runs them on
the GPU.  Nothing here imports snvc_amd.

The shapes are the smallest at which each part of csrc/decode.hip can go wrong: M = nl * nw = 35 is odd, so every second map
starts 4 bytes off a 16-byte boundary; M = 1 has neither a whole quad nor a fit from the grid (all parts would share one
cell, so the offsets come from `coordinates`); M = 1247 = 43 * 29 is more than one trip of a 256-thread loop over quads,
with a tail of three; N = 300 is more than one 64-thread block of the fit.
"""
import types

import numpy as np

X_RANGE, Z_RANGE = (-1.6, 1.6), (-2.4, 2.4)
F32 = np.float32

NAMES = ("m35", "m1_coords", "m1247_ties", "edges", "n1", "n300", "p1", "coords_f32", "coords_f64")
_SHAPES = {  # name: (n, parts, nl, nw, seed, coordinates dtype or None)
    "m35": (6, 9, 7, 5, 11, None), "m1_coords": (4, 9, 1, 1, 12, np.float64), "m1247_ties": (3, 9, 43, 29, 13, None),
    "edges": (7, 9, 7, 5, 14, None), "n1": (1, 9, 7, 5, 15, None), "n300": (300, 9, 7, 5, 16, None), "p1": (5, 1, 7, 5, 17, None),
    "coords_f32": (5, 9, 7, 5, 18, np.float32), "coords_f64": (5, 9, 7, 5, 19, np.float64)}

# the two tied maxima of "m1247_ties", (instance, part) -> (lower index, higher index).  Quad q of a map is read by thread
# q % 256 (the up to three leading scalars shift that by less than one quad): 41 -> thread 10 (first wave), 1002 -> 250 (last),
# 800 -> 199 or 200 (last), 1043 -> 260 % 256 = 4 (first).  The lower index lies in the first wave's share once and in the last
# wave's once.
TIES = {(0, 1): (41, 1002), (0, 2): (800, 1043)}
TIE_VALUE = F32(1.5)
NAN_AT = (5, 4, (9, 20))      # "edges": instance, part, the two NaN cells


def case(name):
    """dict: cfg (x_range, z_range), ncf float32 [N,parts,nl,nw], samples float64 [N,7], grid float64 [nl*nw,3], coordinates
    ([N,parts,2] or None), expect_keep (bool [N]: what the case is built to give under the default Filter)."""
    n, parts, nl, nw, seed, ctype = _SHAPES[name]
    r = np.random.default_rng(seed)
    cfg = types.SimpleNamespace(x_range=X_RANGE, z_range=Z_RANGE)
    ncf = r.uniform(0.0, 1.0, (n, parts, nl, nw)).astype(F32)
    samples = np.stack([r.uniform(1.4, 1.7, n), r.uniform(1.5, 1.8, n), r.uniform(3.5, 4.5, n), r.uniform(-10, 10, n),
                        r.uniform(1.5, 1.9, n), r.uniform(6, 50, n), r.uniform(-np.pi, np.pi, n)], axis=1)
    zs, xs = np.meshgrid(np.linspace(Z_RANGE[0], Z_RANGE[1], nl), np.linspace(X_RANGE[0], X_RANGE[1], nw), indexing="ij")
    grid = np.stack([xs.ravel(), r.uniform(-0.5, 0.5, nl * nw), zs.ravel()], axis=1)      # y is dropped by the decode
    coordinates = r.uniform(0.05, 0.95, (n, parts, 2)).astype(ctype) if ctype is not None else None
    keep = np.ones(n, dtype=bool)
    flat = ncf.reshape(n, parts, nl * nw)
    if name == "edges":
        flat[0, 2, 17], flat[0, 7, 3] = 2.0, -1.0                       # exactly the bounds: kept
        flat[1, 3, 34] = np.nextafter(F32(2.0), F32(np.inf))            # one float32 step beyond either: rejected
        flat[2, 8, 0] = np.nextafter(F32(-1.0), F32(-np.inf))
        flat[3, 0, 5], flat[4, 6, 33] = np.inf, -np.inf
        flat[NAN_AT[0], NAN_AT[1], list(NAN_AT[2])] = np.nan            # two NaNs in one map: the first is the arg-max
        flat[6, 5, :] = 0.0                                             # a part of weight 0 in the fit; kept
        keep[1:6] = False
    elif n > 1:
        for i in range(1, n, 3):                                        # every third instance fails the filter
            flat[i, r.integers(parts), r.integers(nl * nw)] = 2.5 if i % 2 else -1.5
            keep[i] = False
    if name == "m1247_ties":
        for (i, p), cells in TIES.items():
            flat[i, p, list(cells)] = TIE_VALUE
    return dict(cfg=cfg, ncf=ncf, samples=samples, grid=grid, coordinates=coordinates, expect_keep=keep)
