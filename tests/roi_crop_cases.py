"""Small cases of the RoI cropper, shared by tests/test_roi_crop_host.py, tests/test_gpu_roi_crop.py and
tests/golden/make_golden_roi_crop.py.  Everything is generated from seeds; nothing here imports snvc_amd.

Images are odd-sized (37 x 53 and 41 x 29, rows of 159 and 87 bytes: no multiple of 4), the smallest shapes at which a wrong
stride or an alignment assumption shows.  Noise pixels lie in 1 .. 255, so a 0 in a raw crop is the border and nothing else.
The projections are synthetic pinhole cameras (focal length 40 px, principal point at the image centre, 0.54 m baseline) that
put boxes a few metres away into these images.

Each sample carries the tags the host test asserts from the restatement alone (left camera):
  inside    every tap of the crop lies in the image          border_lt  the crop hangs over the left and the top edge
  outside   no tap lies in the image: the raw crop is zero   border_rb  over the right and the bottom edge
  k>1 / k<1 the crop magnifies / minifies
"""
import os
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_NPZ = os.path.join(HERE, "golden", "roi_crop_ref.npz")

FOCAL, BASELINE = 40.0, 0.54
GRID_RANGE = (1.6, 1.8, 4.0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
ROUND_MARGIN = 1e-6      # every value handed to R(.) is at least this far from a half-integer
FLOOR_MARGIN = 1e-6      # 'exact' mode: every source coordinate is at least this far from an integer


def noise_image(h, w, seed):
    return np.random.default_rng(seed).integers(1, 256, (h, w, 3), dtype=np.uint8)


def gradient_image(h, w):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([20 + 3.5 * x + 0.5 * y, 230 - 2.0 * x - 1.5 * y, 40 + 2.0 * y + 1.0 * x], axis=2).round().astype(np.uint8)


def projections(h, w):
    """(P_left, P_right) [3,4] float64 for an h x w image."""
    P = np.array([[FOCAL, 0, 0.5 * w + 0.25, 0], [0, FOCAL, 0.5 * h - 0.125, 0], [0, 0, 1, 0]], dtype=np.float64)
    Pr = P.copy()
    Pr[0, 3] = -FOCAL * BASELINE
    return P, Pr


def cfg(resolution):
    return types.SimpleNamespace(resolution=resolution, aspect_ratio=resolution[1] / resolution[0], grid_range=GRID_RANGE,
                                 img_mean=MEAN, img_std=STD)


# (h, w, l, x, y, z, ry) and the tags of the left crop.  The sample's own size only moves the box's centre height.
_WIDE = [  # for the 37 x 53 image
    ((1.5, 1.6, 3.9, 0.31, 0.83, 17.3, 0.3), ("inside", "k>1")),
    ((1.4, 1.7, 4.2, -7.9, -4.9, 14.2, -0.4), ("border_lt", "k>1")),
    ((1.7, 1.6, 3.7, 9.6, 8.2, 16.1, 1.1), ("border_rb", "k>1")),
    ((1.5, 1.6, 4.0, 33.0, 1.0, 15.7, 0.2), ("outside",)),
    ((1.6, 1.7, 4.1, 0.4, 0.9, 5.3, 0.15), ("k<1",)),
]
_TALL = [  # for the 41 x 29 image
    ((1.5, 1.6, 3.9, 0.12, 0.77, 21.3, 1.4), ("inside", "k>1")),
    ((1.4, 1.7, 4.2, -5.1, -6.3, 15.2, 1.2), ("border_lt", "k>1")),
    ((1.7, 1.6, 3.7, 4.4, 7.9, 14.1, 1.9), ("border_rb", "k>1")),
    ((1.5, 1.6, 4.0, -2.0, 29.0, 15.7, 0.2), ("outside",)),
    ((1.6, 1.7, 4.1, 0.1, 0.9, 4.9, 1.5), ("k<1",)),
]
_BIG = [  # for the 40 x 56 gradient image at 64 x 64
    ((1.5, 1.6, 3.9, 0.31, 0.83, 17.3, 0.3), ("inside", "k>1")),
    ((1.4, 1.7, 4.2, -9.9, -6.1, 14.2, -0.4), ("border_lt", "k>1")),
    ((1.7, 1.6, 3.7, 10.6, 7.2, 16.1, 1.1), ("border_rb", "k>1")),
    ((1.6, 1.7, 4.1, 0.2, 0.7, 2.9, 1.45), ("k<1",)),
]

NAMES = ("noise_24x16", "noise_16x24", "gradient_64", "two_frames")


def case(name):
    """dict: cfg, samples [N,7], tags, left / right (lists of uint8 [H,W,3]), P_left / P_right [F,3,4], frame (None or [N])."""
    if name == "noise_24x16":
        shapes, res, rows = [(37, 53)], (24, 16), [_WIDE]
    elif name == "noise_16x24":
        shapes, res, rows = [(41, 29)], (16, 24), [_TALL]
    elif name == "gradient_64":
        shapes, res, rows = [(40, 56)], (64, 64), [_BIG]
    elif name == "two_frames":
        shapes, res, rows = [(37, 53), (41, 29)], (24, 16), [_WIDE[:3], _TALL[:3]]
    else:
        raise KeyError(name)
    if name == "gradient_64":
        left, right = [gradient_image(*shapes[0])], [gradient_image(*shapes[0])[:, ::-1].copy()]
    else:
        left = [noise_image(h, w, 10 + i) for i, (h, w) in enumerate(shapes)]
        right = [noise_image(h, w, 20 + i) for i, (h, w) in enumerate(shapes)]
    P = [projections(h, w) for h, w in shapes]
    samples, tags, frame = [], [], []
    for f, rws in enumerate(rows):
        for s, t in rws:
            samples.append(s)
            frame.append(f)
            if name == "two_frames" and f == 1:
                t = tuple(x for x in t if not x.startswith("k"))       # another resolution: only where the crop lies is tagged
            tags.append(t)
    if name == "two_frames":            # interleave, so that neighbouring samples read different frames
        order = [0, 3, 1, 4, 2, 5]
        samples, tags, frame = [samples[i] for i in order], [tags[i] for i in order], [frame[i] for i in order]
    return {"cfg": cfg(res), "samples": np.array(samples, dtype=np.float64), "tags": tags, "left": left, "right": right,
            "P_left": np.stack([p[0] for p in P]), "P_right": np.stack([p[1] for p in P]),
            "frame": np.array(frame, dtype=np.int64) if len(shapes) > 1 else None}


def frame_of(c, n):
    return 0 if c["frame"] is None else int(c["frame"][n])


def load_golden():
    with np.load(GOLDEN_NPZ) as z:
        return {k: z[k] for k in z.files}
