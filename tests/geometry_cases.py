"""Cases of the geometry ops -- cost volume (csrc/cost_volume.hip), feature -> voxel gather (csrc/voxel_gather.hip) and its adjoint
(csrc/voxel_gather_bwd.hip) -- one row per launcher form: the smallest shape that takes the form, the form it must take and the
launch numbers it must get, as ``include/snvc_forms.h`` reports them.  tests/test_geometry_forms_host.py holds the table to the
query (no GPU); tests/test_gpu_geometry_forms.py asks the query on the device, runs the op and compares with the references below.

Nothing in the table depends on the device: the only CU-dependent number, the gather's run length, is 4096 for these V at any
CU count from 8 up.

Shapes.  Cost volume: (N, C, H, W, D, downsample) with H, W the feature map's, as in test_gpu_parity.CV_CASES.  Gather: (N, F, Hf, Wf, V)
and the crop resolution (rows, columns).
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

from split_format import split_pair  # noqa: F401  (the split format's one definition; the gather tests take it from here)

F32, F64 = 0, 1                           # snvc_dtype
KIND = {"f32": 0, "c8": 1, "split": 2}    # snvc_voxel_gather_kind
UNSUPPORTED = 2                           # SNVC_ERR_UNSUPPORTED
POW2, ODD = (64, 128), (28, 36)           # crop resolutions: reciprocal-multiply and division forms of the normalisation


@dataclass(frozen=True, repr=False)
class Case:
    name: str
    entry: str                            # cv_fwd, cv_bwd, gather_fwd, gather_bwd
    shape: Tuple[int, ...]
    form: Optional[str]                   # enumerator of the entry's enum in snvc_forms.h without its prefix; None: a refusal
    info: dict = field(default_factory=dict, hash=False, compare=False)   # launch numbers the query must report
    dtype: int = F32                      # cost volume
    right: bool = False                   # cost volume: the right-half entry points
    kind: str = "f32"                     # gather forward: f32, c8, split
    res: Tuple[int, int] = POW2           # gather
    det: bool = False                     # gather backward: the sorted form
    refusal: Optional[Tuple[int, str]] = None      # (status, text the message starts with)
    place: int = 16                       # guard-band suite: the second placement that keeps the form (bytes off 256)
    inf_pixel: bool = True                # gather forward: an inf feature pixel at (0, 0)

    def __str__(self):
        return self.name

    __repr__ = __str__


# Depths: a row's shift array must hold _cv_inputs' three shifts and all of cv_shift's own (3 forward, 10 backward), so no row has
# N * D below 6 (forward) or 13 (backward); where the smallest shape that takes a form had fewer planes, D was raised to that.
def _cv_fwd():
    rel = dict(RB=4, hblocks=2, dsplit=2, dchunk=9, grid_x=4, grid_y=2, threads=320, lds=5 * 312 * 4)
    fb = dict(RB=5, hblocks=1, dsplit=1, dchunk=3, grid_x=2, grid_y=1, threads=64, lds=6 * 12 * 4)
    return [
        # released width W/4 = 78: a row spans two waves; RB = 4 of H = 6 leaves a ragged row block; D = 17 splits 9 + 8
        Case("cvf_rows_released", "cv_fwd", (1, 2, 6, 312, 17, 1), "ROWS", rel),
        Case("cvf_rows_released_right", "cv_fwd", (1, 2, 6, 312, 17, 1), "ROWS_RIGHT", rel, right=True),
        # no r <= H = 5 makes r * 48 bytes a multiple of 128: RB = min(256 / 3 -> 8, H)
        Case("cvf_rows_rb_fallback", "cv_fwd", (2, 1, 5, 12, 3, 1), "ROWS", fb),
        Case("cvf_rows_rb_fallback_right", "cv_fwd", (2, 1, 5, 12, 3, 1), "ROWS_RIGHT", fb, right=True),
        Case("cvf_right_refuses_odd_w", "cv_fwd", (1, 2, 4, 13, 6, 1), None, right=True,
             refusal=(UNSUPPORTED, "snvc_cost_volume_forward_right: needs fp32, downsample 1, W % 4 == 0")),
        Case("cvf_f32x4", "cv_fwd", (1, 1, 2, 2052, 6, 1), "F32X4", dict(grid_x=5, grid_y=12, threads=256)),
        # N*2*C*D = 65600 planes > 65535: the plane walk takes a second step for 65 of them
        Case("cvf_generic_f32_plane_walk", "cv_fwd", (2, 4, 1, 3, 4100, 1), "GENERIC_F32", dict(grid_x=1, grid_y=65535), place=4),
        Case("cvf_f64x2_plane_walk", "cv_fwd", (2, 4, 1, 2, 4100, 1), "F64X2", dict(grid_x=1, grid_y=65535), dtype=F64),
        Case("cvf_generic_f64_odd_w", "cv_fwd", (1, 2, 3, 7, 6, 1), "GENERIC_F64", dict(grid_y=24), dtype=F64, place=4),
        Case("cvf_generic_f64_ds2", "cv_fwd", (1, 2, 4, 6, 6, 2), "GENERIC_F64", dict(grid_y=24), dtype=F64, place=4),
    ]


def _cv_bwd():
    return [
        Case("cvb_rows_w2", "cv_bwd", (1, 1, 2, 2, 13, 1), "ROWS", dict(grid_x=1), place=4),          # the contract's minimum width
        Case("cvb_rows_w2_right", "cv_bwd", (1, 1, 2, 2, 13, 1), "ROWS_RIGHT", dict(grid_x=1), right=True, place=4),
        Case("cvb_rows_released", "cv_bwd", (1, 2, 6, 312, 17, 1), "ROWS", dict(grid_x=15), place=4),
        Case("cvb_rows_released_right", "cv_bwd", (1, 2, 6, 312, 17, 1), "ROWS_RIGHT", dict(grid_x=15), right=True, place=4),
        Case("cvb_gather_f32_w1", "cv_bwd", (1, 1, 3, 1, 13, 1), "GATHER_F32", dict(grid_x=1), place=4),
        Case("cvb_right_refuses_w1", "cv_bwd", (1, 1, 3, 1, 13, 1), None, right=True,
             refusal=(UNSUPPORTED, "snvc_cost_volume_backward_right: needs 2 <= W")),
        Case("cvb_gather_f64_ds2", "cv_bwd", (1, 2, 4, 6, 13, 2), "GATHER_F64", dict(grid_x=1), dtype=F64, place=4),
    ]


def _gather_fwd():
    t = [Case("gf_plain", "gather_fwd", (2, 5, 7, 9, 30), "PLAIN", dict(grid_x=1, grid_yz=2), res=ODD, place=4)]
    small = (2, 8, 7, 9)
    t += [Case("gf_cl", "gather_fwd", small + (333,), "CL", dict(grid_x=2, grid_yz=2), res=ODD, place=4),       # V % 4 != 0
          Case("gf_cl_x4", "gather_fwd", small + (332,), "CL_X4", dict(grid_x=1, grid_yz=2), res=ODD),
          Case("gf_cl_c8_v333", "gather_fwd", small + (333,), "CL_C8", dict(grid_x=2), kind="c8", res=ODD, place=4),
          Case("gf_cl_c8_v332", "gather_fwd", small + (332,), "CL_C8", dict(grid_x=2), kind="c8", res=ODD, place=4)]
    lds = {"f32": ("LDS", 4, 512), "c8": ("LDS_C8", 8, 1024), "split": ("LDS_SPLIT", 8, 1024)}
    for kind, (form, cs, bs) in lds.items():
        for res, tag in ((POW2, "pow2"), (ODD, "div")):
            slices = 8 // cs
            # the largest plane of the LDS forms: 4608 pixels, 73 744 / 147 488 bytes of dynamic LDS
            t += [Case(f"gf_lds_boundary_{kind}_{tag}", "gather_fwd", (1, 8, 64, 72, 4096), form,
                       dict(run=4096, nruns=1, pow2=int(res == POW2), slices=slices, grid_x=8 * slices, threads=bs,
                            lds=4608 * cs * 4 + (cs // 4) * 16), kind=kind, res=res, inf_pixel=kind != "split"),
                  # ten runs, the last of 8 voxels: blocks 8.. of an XCD take the second round of the (run, slice) map
                  Case(f"gf_lds_ten_runs_{kind}_{tag}", "gather_fwd", (1, 8, 5, 6, 9 * 4096 + 8), form,
                       dict(run=4096, nruns=10, pow2=int(res == POW2), slices=slices, grid_x=16 * slices, threads=bs), kind=kind, res=res)]
    # one plane past the boundary (4620 pixels): the channels-last forms, and the split entry point has none
    past = (1, 8, 60, 77, 4096)
    t += [Case("gf_past_boundary_f32", "gather_fwd", past, "CL_X4", dict(grid_x=4), res=ODD),
          Case("gf_past_boundary_c8", "gather_fwd", past, "CL_C8", dict(grid_x=16), kind="c8", res=ODD, place=4),
          Case("gf_split_refuses_plane", "gather_fwd", past, None, kind="split", res=ODD,
               refusal=(UNSUPPORTED, "snvc_voxel_gather_forward_split: needs the LDS-staged form")),
          Case("gf_split_refuses_v4092", "gather_fwd", (1, 8, 64, 72, 4092), None, kind="split", res=ODD,
               refusal=(UNSUPPORTED, "snvc_voxel_gather_forward_split: needs the LDS-staged form"))]
    return t


def _gather_bwd():
    return [
        # 2 * 91 * 91 * 4 = 66 248 bytes > 64 KiB: no LDS copy of two planes
        Case("gb_global_atomics", "gather_bwd", (1, 2, 91, 91, 500), "GLOBAL_ATOMICS", dict(grid_x=2, grid_y=1), res=ODD, place=4),
        # two voxel chunks (the flush adds across workgroups), odd F (the second plane of the last pair is idle)
        Case("gb_lds_atomics_two_chunks", "gather_bwd", (1, 3, 6, 6, 65536 + 300), "LDS_ATOMICS",
             dict(vchunk=65536, nvchunks=2, grid_y=2, lds=288), res=ODD, place=4),
        # F = 72: a second, ragged channel pass of 8; segments beyond 1024 voxels next to short ones
        Case("gb_sorted_two_passes", "gather_bwd", (3, 72, 7, 9, 2000), "SORTED", dict(passes=2), res=ODD, det=True, place=4),
    ]


CASES = _cv_fwd() + _cv_bwd() + _gather_fwd() + _gather_bwd()
BY_ENTRY = {e: [c for c in CASES if c.entry == e] for e in ("cv_fwd", "cv_bwd", "gather_fwd", "gather_bwd")}
ENUM_PREFIX = {"cv_fwd": "CVF", "cv_bwd": "CVB", "gather_fwd": "GF", "gather_bwd": "GB"}
assert len({c.name for c in CASES}) == len(CASES)
BY_NAME = {c.name: c for c in CASES}
# the guard-band suite (tests/test_gpu_guard_ops.py) reruns these: every form once, and each path of a form that stages or walks
# differently (the ragged row block, the plane walk's second step, the LDS boundary, the second round of runs); PLAIN has its
# guarded run in that suite's own table (gather_edges)
GUARDED = [BY_NAME[n] for n in (
    "cvf_rows_released", "cvf_rows_released_right", "cvf_rows_rb_fallback", "cvf_f32x4", "cvf_generic_f32_plane_walk", "cvf_f64x2_plane_walk",
    "cvf_generic_f64_odd_w", "cvb_rows_w2", "cvb_rows_released_right", "cvb_gather_f32_w1", "cvb_gather_f64_ds2",
    "gf_cl", "gf_cl_x4", "gf_cl_c8_v333", "gf_past_boundary_f32", "gf_lds_boundary_f32_pow2", "gf_lds_boundary_c8_pow2",
    "gf_lds_boundary_split_pow2", "gf_lds_ten_runs_f32_div", "gf_lds_ten_runs_c8_div", "gf_lds_ten_runs_split_div",
    "gb_global_atomics", "gb_lds_atomics_two_chunks", "gb_sorted_two_passes")]
TEST_OF_ENTRY = {"cv_fwd": "test_cost_volume_forward", "cv_bwd": "test_cost_volume_backward", "gather_fwd": "test_voxel_gather_forward",
                 "gather_bwd": "test_voxel_gather_backward"}


def query(c: Case, aligned: int = 3):
    """(form id / 0 / -status, info dict, error text) of the case's shape from the library's own decision function."""
    from snvc_amd import _forms
    if c.entry == "cv_fwd":
        n, ch, h, w, d, ds = c.shape
        return _forms.cost_volume_forward(n, ch, h, w, d, ds, c.dtype, c.right, aligned)
    if c.entry == "cv_bwd":
        n, ch, h, w, d, ds = c.shape
        return _forms.cost_volume_backward(n, ch, h // ds, w // ds, d, ds, c.dtype, c.right)
    n, f, hf, wf, v = c.shape
    if c.entry == "gather_fwd":
        return _forms.voxel_gather_forward(KIND[c.kind], n, f, hf, wf, v, c.res, aligned)
    return _forms.voxel_gather_backward(n, f, hf, wf, v, c.det)


# ------------------------------------------------------------------------------------------------------------------ inputs
def np_dtype(c: Case):
    return np.float64 if c.dtype == F64 else np.float32


def cv_shift(c: Case, seed: int, backward: bool):
    """Shifts as test_gpu_parity._cv_inputs draws them (0, the integer 2 and W + 5 at [0, :3]), with the tail of the array overwritten
    by this table's own: W - 1 exactly (the right-edge clamp: x_lo == img_w - 1), the value just below 1 (column 1 lands a hair
    right of pixel 0, wide columns round onto the pixel), W + 5; for the backward also the shifts outside the forward's
    contract (NaN, negative, fractional negative, +-1e9).  Every row carries the whole set behind _cv_inputs's three."""
    from test_gpu_parity import _cv_inputs
    n, ch, h, w, d, _ = c.shape
    dt = np_dtype(c)
    s = _cv_inputs(n, ch, h, w, d, dt, seed)[2]
    extra = [w - 1.0, np.nextafter(dt(1.0), dt(0.0)), w + 5.0]
    if backward:
        extra += [np.nan, -0.5, 1e9, -2.75, -1e9, -1.0, -30.0]
    assert s.size - 3 >= len(extra), f"{c.name}: N * D = {s.size} leaves no room for {len(extra)} shifts behind _cv_inputs' three"
    s.reshape(-1)[s.size - len(extra):] = np.array(extra, dtype=dt)
    return s


def cv_forward_inputs(c: Case):
    from test_gpu_parity import _cv_inputs
    n, ch, h, w, d, _ = c.shape
    left, right, _ = _cv_inputs(n, ch, h, w, d, np_dtype(c), 5)
    return left, right, cv_shift(c, 5, False)


def cv_backward_inputs(c: Case):
    n, ch, h, w, d, ds = c.shape
    g = np.random.default_rng(7).standard_normal((n, 2 * ch, d, h // ds, w // ds)).astype(np_dtype(c))
    return g, cv_shift(c, 6, True)


def gather_forward_inputs(c: Case):
    """Feature maps and coordinates as test_voxel_gather_lds_path_bit_exact_with_edge_coordinates builds them: uniform over
    [-0.2, 1.2] x the crop, then exact borders, far outside, +-inf, NaN, a run of subnormals, and an inf feature pixel at (0, 0) -- the
    pixel a select form parks its out-of-range taps on.  The scale of a split pair comes from the maps' maximum and is 1 for a
    non-finite map: the split rows at the LDS boundary leave the inf pixel out, so that the multiply by a scale other than 1 is
    tested, and the ten-run split rows keep it, for the non-finite-scale path (hi = inf, lo = NaN where the pixel is sampled)."""
    n, f, hf, wf, v = c.shape
    res = c.res
    r = np.random.default_rng(19)
    lf = r.standard_normal((n, f, hf, wf)).astype(np.float32)
    rf = r.standard_normal((n, f, hf, wf)).astype(np.float32)
    if c.inf_pixel:
        lf[0, :, 0, 0] = np.inf
    pts = np.stack([r.uniform(-0.2 * res[1], 1.2 * res[1], (n, v)), r.uniform(-0.2 * res[0], 1.2 * res[0], (n, v))], 1).astype(np.float32)
    pts[0, 0, :8] = [0.0, res[1], -2.0, 1e9, np.inf, -np.inf, np.nan, 0.5 * res[1]]
    pts[0, 1, :8] = [0.0, res[0], 0.5 * res[0], 3.0, 1.0, 2.0, 3.0, np.nan]
    pts[n - 1, :, v // 2:v // 2 + min(100, v // 4)] = 1e-41          # subnormal coordinates: x / 2^k and x * 2^-k round alike
    pts[0, :, v - 1] = [res[1], res[0]]                               # the last voxel of the ragged last run: the far corner
    return lf, rf, pts, pts[:, :, ::-1].copy()


def to_c8(x: np.ndarray):
    """[N, C, V] -> the C8 layout [N, C/8, V, 8]."""
    n, ch, v = x.shape
    return np.ascontiguousarray(x.reshape(n, ch // 8, 8, v).transpose(0, 1, 3, 2))


def gather_backward_inputs(c: Case):
    """Coordinates uniform over [-0.1, 1.1] x the crop with the edge set of test_voxel_gather_backward_deterministic (borders, far
    outside, NaN).  The sorted case draws three quarters of its voxels on a line one feature pixel long that starts a tenth of a pixel
    before a column: about 1350 of a sample's 2000 voxels share one base pixel -- two pieces, the second ragged -- 150 the next, and
    the rest are spread thin.  (Half the voxels over two pixels, 500 a segment, would stay inside one piece of 1024.)"""
    n, f, hf, wf, v = c.shape
    res = c.res
    r = np.random.default_rng(23)
    pts = r.uniform(-0.1 * res[1], 1.1 * res[1], (n, 2, v)).astype(np.float32)
    pts[:, 1] = r.uniform(-0.1 * res[0], 1.1 * res[0], (n, v)).astype(np.float32)
    if c.det:
        k = 3 * v // 4
        t = np.linspace(0.0, 1.0, k, dtype=np.float32)
        pts[:, 0, :k] = (res[1] / wf) * (3.6 + t)                   # feature x from 3.1 to 4.1
        pts[:, 1, :k] = (res[0] / hf) * 4.0                         # feature y = 3.5
    pts[0, 0, -5:] = [0.0, res[1], -3.0, 1e9, np.nan]
    pts[0, 1, -5:] = [0.0, res[0], 14.0, 3.0, 5.0]
    g = r.standard_normal((n, 2 * f, v)).astype(np.float32)
    return g, pts, pts[:, :, ::-1].copy()


def grid_sample_grads(c: Case, g: np.ndarray, l_pts: np.ndarray, r_pts: np.ndarray, dtype):
    """Gradients of the two feature maps by torch autograd through F.grid_sample on the CPU in ``dtype``, built as in
    test_voxel_gather_backward_deterministic; NaN coordinates are replaced by far-outside ones (no tap, no gradient, as in the
    kernels), every voxel takes part."""
    import torch
    import torch.nn.functional as F
    n, f, hf, wf, v = c.shape
    res = c.res
    out = []
    for side, p in enumerate((l_pts, r_pts)):
        x = torch.zeros((n, f, hf, wf), dtype=dtype, requires_grad=True)
        pn = torch.nan_to_num(torch.from_numpy(p), nan=-1e6).to(dtype)
        grid = torch.stack([pn[:, 0] / res[1] * 2 - 1, pn[:, 1] / res[0] * 2 - 1], dim=-1).view(n, 1, v, 2)
        y = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[:, :, 0]   # [n, f, v]
        (y * torch.from_numpy(g[:, side * f:(side + 1) * f]).to(dtype)).sum().backward()
        out.append(x.grad.double().numpy())
    return out
