"""Cases of the first-layer kernels (csrc/sheared_conv.hip) -- the sheared and the any-shift first convolution -- one row per value of
the launch geometry that a small launch can reach: rows per workgroup (RB) with a short last row block and idle threads in the last
wave, depth chunks of the split producers (a short chunk, a chunk without planes), column chunks of the weight gradient, more slots
than threads in the adjoint, one lane and all 64 lanes in the fused backward.  Each row states what ``include/snvc_forms.h``'s query
must report for it; tests/test_first_layer_forms_host.py holds the table to the query (no GPU) and pins what no small launch reaches
(RB 5 and 7, the refusals) and checks the references below on tiny shapes; tests/test_gpu_first_layer_forms.py asks the query, runs the
op and compares with the references below.

The numbers follow the launchers' rule: RB starts at min(8, 512 / (W / 4)) and is halved by (RB + 1) / 2 while ceil(H / RB) * C * N
< 1024, then lowered while RB rows need more than 150 KiB of LDS; the split producers double their depth chunks up to 16 while
H * ceil(C / 8) * N * chunks < 512 (sheared) or 768 (warped) and D / (2 * chunks) >= 8; the weight gradient takes two column chunks
when WU > 320, each a multiple of 64 columns.

The references are plain numpy restatements of the ops' definitions (``ops.sheared_expand``'s docstring), in float32 where the kernel's
result is a single rounding and in float64 otherwise; none of them calls the library.
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

INVALID, UNSUPPORTED = 1, 2               # snvc_status
RELU, STREAM_OUT, R3 = 1, 32, 256         # SNVC_EPI_RELU, SNVC_EPI_STREAM_OUT, SNVC_WARPED_EXPAND_R3 (asserted against ops by the host test)
# snvc_first_layer_entry
(SHEARED_EXPAND, SHEARED_EXPAND_AMAX, SHEARED_EXPAND_STATS, SHEARED_EXPAND_SPLIT, SHEARED_BACKWARD_REDUCE, SHEARED_REDUCE, WARPED_EXPAND,
 WARPED_EXPAND_SPLIT, WARPED_EXPAND_BACKWARD) = range(9)


def sheared_geometry(q, m0, d, w):
    """(off, wu, off_col, wu_col) as the model lays G and G' out."""
    from snvc_amd.models.submodule import sheared_geometry as geo
    return geo(q, m0, d, w)


@dataclass(frozen=True, repr=False)
class Case:
    name: str
    shape: Tuple[int, ...]
    info: dict = field(default_factory=dict, hash=False, compare=False)      # what the query must report
    last: int = 0                         # rows of the last row block / planes of the last chunk that has any / columns of the last chunk
    active: int = 0                       # threads of a full row block that have a quad to work on

    def __str__(self):
        return self.name

    __repr__ = __str__


# ------------------------------------------------------------------------------------------------ fp32 sheared expand: (N, C, H, W, D, q, m0)
EXPAND = [
    Case("rb8_short_block", (2, 64, 60, 24, 6, 2, 3), dict(RB=8, blocks=8, threads=64, grid_x=8, grid_yz=128), last=4, active=48),
    Case("rb4_q1", (1, 64, 62, 24, 6, 1, 0), dict(RB=4, blocks=16, threads=64, grid_x=16, grid_yz=64), last=2, active=24),
    Case("rb4_q4", (1, 64, 62, 24, 6, 4, 1), dict(RB=4, blocks=16, threads=64, grid_x=16, grid_yz=64), last=2, active=24),
    Case("rb2_one_row_left", (1, 32, 63, 24, 7, 2, 0), dict(RB=2, blocks=32, threads=64, grid_x=32, grid_yz=32), last=1, active=12),
    Case("rb2_w44", (1, 128, 15, 44, 5, 4, 2), dict(RB=2, blocks=8, threads=64, grid_x=8, grid_yz=128), last=1, active=22),
    Case("rb3_w320", (1, 64, 48, 320, 4, 1, 2), dict(RB=3, blocks=16, threads=256, grid_x=16, grid_yz=64), last=3, active=240),
    Case("rb6_w320", (2, 64, 48, 320, 4, 2, 1), dict(RB=6, blocks=8, threads=512, grid_x=8, grid_yz=128), last=6, active=480),
]
EXPAND_BY_NAME = {c.name: c for c in EXPAND}
STATS = [c for c in EXPAND if c.shape[5] in (1, 2)]          # snvc_sheared_expand_stats takes q in {1, 2}

# ------------------------------------------------------------------------------------------------------ fp32 warped expand: (N, C, H, W, D)
WARPED = [
    Case("rb8_short_block", (2, 64, 60, 24, 6), dict(RB=8, blocks=8, threads=64), last=4, active=48),
    Case("rb4", (1, 64, 62, 24, 6), dict(RB=4, blocks=16, threads=64), last=2, active=24),
    Case("rb2_one_row_left", (1, 32, 63, 24, 6), dict(RB=2, blocks=32, threads=64), last=1, active=12),
]

# ----------------------------------------------------------------------------------------------------- split producers: (N, C, H, W, D)
# name, shape, (chunks, planes per chunk) of the sheared and of the warped producer
SPLIT = [
    ("d35", (1, 12, 1, 68, 35), (4, 9), (4, 9)),               # 9, 9, 9, 8
    ("d67", (1, 12, 1, 68, 67), (8, 9), (8, 9)),               # seven of 9, the last has 4
    ("d128", (1, 12, 1, 68, 128), (16, 8), (16, 8)),
    ("d131", (1, 12, 1, 68, 131), (16, 9), (16, 9)),           # the 15th has 5 planes (an end plane among them), the 16th none
    ("d200_wgs", (2, 64, 8, 20, 200), (4, 50), (8, 25)),       # stopped by the workgroup count: 128 * 4 = 512, 128 * 8 = 1024 >= 768
    ("d241_end_plane_alone", (1, 12, 1, 68, 241), (16, 16), (16, 16)),      # the 16th chunk holds plane 240, the end plane, and nothing else
]
SPLIT_BY_NAME = {s[0]: s for s in SPLIT}
SPLIT_SHEARED_Q = {"d35": (1, 2, 4), "d131": (1, 2, 4)}      # the other rows run q = 2


def chunk_planes(d, chunks, per_chunk):
    """Planes of every chunk, in order: what the kernels' ``d_lo = k * per_chunk, d_hi = min(D, d_lo + per_chunk)`` leaves."""
    return [max(0, min(d, (k + 1) * per_chunk) - k * per_chunk) for k in range(chunks)]


# ------------------------------------------------------------------------------------------------- sheared weight gradient: WU -> geometry
WGRAD_N, WGRAD_H, WGRAD_CO = 2, 3, 40
WGRAD_C = (5, 32)
WGRAD = [                                                      # last: columns of the last chunk
    Case("wu320", (320,), dict(chunks=1, per_chunk=320, grid_x=3, grid_yz=4, threads=256), last=320),
    Case("wu321", (321,), dict(chunks=2, per_chunk=192, grid_x=6, grid_yz=4, threads=256), last=129),
    Case("wu384", (384,), dict(chunks=2, per_chunk=192, grid_x=6, grid_yz=4, threads=256), last=192),
    Case("wu388", (388,), dict(chunks=2, per_chunk=256, grid_x=6, grid_yz=4, threads=256), last=132),
]

# ------------------------------------------------------------------------------------------------------- adjoint: (N, C, D, H, W, q); m0 = 1
REDUCE = [
    Case("slots_308", (1, 2, 9, 2, 300, 1), dict(RB=1, threads=256, grid_x=2, grid_yz=2)),        # ceil(WG / q) = 308 > 256 threads
    Case("wg2_260", (1, 1, 250, 1, 24, 2), dict(RB=1, threads=256, grid_x=1, grid_yz=1)),         # WG2 = (250 + 13) // 4 * 4 = 260 > 256 threads
]
REDUCE_M0 = 1
REDUCE_SLOTS = {"slots_308": (308, 20), "wg2_260": (28, 260)}          # (ceil(WG / q), WG2): which of the kernel's two strided loops takes a second trip

# ------------------------------------------------------------------------------------------ fused backward: (N, C, D, H, W, q); m0 = q + 1
BACKWARD = [Case(f"w{w}_q{q}", (2, 2, 6, 5, w, q), dict(RB=4, blocks=2, threads=256, grid_x=2, grid_yz=4), last=1)
            for w in (512, 8) for q in (1, 2)]


# ------------------------------------------------------------------------------- what only the query reaches: (entry, arguments, expectation)
# arguments: (N, C, D, H, W, q, m0, WG, WG2, flags).  RB 5 and 7 need q * LW + D > 4800 floats per row (LW = ceil(WG / q) + 4): 8 rows would
# pass the 150 KiB = 38400 floats that a workgroup may ask for.  With W = 24, C = 128, H = 64 the coverage rule leaves RB = 8.
def _rows(wg):
    return (1, 128, 8, 64, 24, 1, 0, wg, 16, 0)


PINNED = [
    ("rb7_lds_cap", SHEARED_EXPAND, _rows(5000), dict(RB=7, blocks=10, threads=64, lds=4 * 7 * (5004 + 8))),          # 7 * 5012 <= 38400 < 8 * 5012
    ("rb5_lds_cap", SHEARED_EXPAND, _rows(7000), dict(RB=5, blocks=13, threads=64, lds=4 * 5 * (7004 + 8))),          # 5 * 7012 <= 38400 < 6 * 7012
    ("rb7_lds_cap_stats", SHEARED_EXPAND_STATS, _rows(5000), dict(RB=7, blocks=10, threads=64)),
    ("rb1_lds_cap", SHEARED_EXPAND, _rows(38000), dict(RB=1, blocks=64, threads=64, lds=4 * (38004 + 8))),
]
REFUSALS = [
    ("expand_lds", SHEARED_EXPAND, _rows(40000), UNSUPPORTED, "snvc_sheared_expand: rows do not fit the LDS"),
    ("expand_amax_lds", SHEARED_EXPAND_AMAX, _rows(40000), UNSUPPORTED, "snvc_sheared_expand: rows do not fit the LDS"),
    ("stats_lds", SHEARED_EXPAND_STATS, _rows(40000), UNSUPPORTED, "snvc_sheared_expand_stats: rows do not fit the LDS"),
    ("split_lds", SHEARED_EXPAND_SPLIT, (1, 8, 8, 4, 24, 1, 0, 5000, 16, 0), UNSUPPORTED, "snvc_sheared_expand_split: the row does not fit the LDS"),
    ("backward_lds", SHEARED_BACKWARD_REDUCE, (1, 2, 8, 4, 24, 1, 0, 4000, 16, 0), UNSUPPORTED, "snvc_sheared_backward_reduce: rows do not fit the LDS"),
    ("backward_w520", SHEARED_BACKWARD_REDUCE, (1, 2, 8, 4, 520, 1, 0, 530, 16, 0), INVALID,
     "snvc_sheared_backward_reduce: bad sizes (W % 8 == 0, W <= 512, q in {1,2}, D >= 2)"),
    ("backward_w20", SHEARED_BACKWARD_REDUCE, (1, 2, 8, 4, 20, 1, 0, 32, 16, 0), INVALID,
     "snvc_sheared_backward_reduce: bad sizes (W % 8 == 0, W <= 512, q in {1,2}, D >= 2)"),
    ("backward_q4", SHEARED_BACKWARD_REDUCE, (1, 2, 8, 4, 24, 4, 0, 100, 16, 0), INVALID,
     "snvc_sheared_backward_reduce: bad sizes (W % 8 == 0, W <= 512, q in {1,2}, D >= 2)"),
    ("split_w516", SHEARED_EXPAND_SPLIT, (1, 8, 8, 4, 516, 1, 0, 530, 16, 0), UNSUPPORTED,
     "snvc_sheared_expand_split: row too wide (W <= 512) or too many channels"),
    ("expand_w2052", SHEARED_EXPAND, (1, 8, 8, 4, 2052, 1, 0, 2060, 16, 0), UNSUPPORTED, "snvc_sheared_expand: row too wide or too many channels"),
    ("expand_w22", SHEARED_EXPAND, (1, 8, 8, 4, 22, 1, 0, 32, 16, 0), INVALID, "snvc_sheared_expand: bad sizes (W % 4 == 0, q in {1,2,4}, D >= 2)"),
    ("expand_flags", SHEARED_EXPAND, (1, 8, 8, 4, 24, 1, 0, 32, 16, STREAM_OUT), UNSUPPORTED, "snvc_sheared_expand: only SNVC_EPI_RELU"),
    ("stats_q4", SHEARED_EXPAND_STATS, (1, 8, 8, 4, 24, 4, 0, 100, 16, 0), INVALID,
     "snvc_sheared_expand_stats: bad sizes (W % 4 == 0, q in {1,2}, D >= 2)"),
    ("reduce_w1", SHEARED_REDUCE, (1, 2, 8, 4, 1, 1, 0, 16, 16, 0), INVALID, "snvc_sheared_reduce: bad sizes (q in {1,2}, D >= 2, W >= 2)"),
    ("warped_win_lds", WARPED_EXPAND, (1, 2, 6000, 4, 2048, 0, 0, 0, 0, 0), UNSUPPORTED, "snvc_warped_expand: rows do not fit the LDS"),
    ("warped_r3_lds", WARPED_EXPAND, (1, 2, 5000, 4, 2048, 0, 0, 0, 0, R3), UNSUPPORTED, "snvc_warped_expand: rows do not fit the LDS"),
    ("warped_w2052", WARPED_EXPAND, (1, 2, 6, 4, 2052, 0, 0, 0, 0, 0), UNSUPPORTED, "snvc_warped_expand: row too wide or too many channels"),
    ("warped_split_w516", WARPED_EXPAND_SPLIT, (1, 8, 6, 4, 516, 0, 0, 0, 0, 0), UNSUPPORTED,
     "snvc_warped_expand_split: row too wide (W <= 512) or too many channels"),
    ("warped_split_lds", WARPED_EXPAND_SPLIT, (1, 8, 9000, 4, 24, 0, 0, 0, 0, 0), UNSUPPORTED, "snvc_warped_expand_split: the row does not fit the LDS"),
    ("warped_bwd_lds", WARPED_EXPAND_BACKWARD, (1, 2, 6000, 1, 1024, 0, 0, 0, 0, 0), UNSUPPORTED,
     "snvc_warped_expand_backward: rows do not fit the LDS"),
    ("warped_bwd_w1028", WARPED_EXPAND_BACKWARD, (1, 2, 6, 4, 1028, 0, 0, 0, 0, 0), UNSUPPORTED,
     "snvc_warped_expand_backward: W <= 1024, C and N <= 65535"),
]


# ---------------------------------------------------------------------------------------------------------------------------- references
def depth_class(d, depth):
    return 0 if d == 0 else (2 if d == depth - 1 else 1)


def sheared_expand_ref(g, gcol, planes, shape, q, m0, off, off_col):
    """x[n,co,d,h,w] = float32(G[n,cls(d),co,h,q*w-d-m0+off] + planes[n,co,cls(d),h,w]) with 0 for G outside its row and G' (``gcol``
    at q*(W-1)-d-m0+off_col) at w = W-1: ``ops.sheared_expand`` without scale and bias.  One float32 add per element."""
    n, c, d, h, w = shape
    wg, wg2 = g.shape[3], gcol.shape[3]
    g5, gc5 = g.reshape(n, 3, c, h, wg), gcol.reshape(n, 3, c, h, wg2)
    raw = np.zeros(shape, np.float32)
    cols = np.arange(w - 1)
    for dd in range(d):
        cls = depth_class(dd, d)
        i = q * cols - dd - m0 + off
        ok = (i >= 0) & (i < wg)
        raw[:, :, dd, :, cols[ok]] = np.moveaxis(g5[:, cls][..., i[ok]], -1, 0)
        i2 = q * (w - 1) - dd - m0 + off_col
        if 0 <= i2 < wg2:
            raw[:, :, dd, :, w - 1] = gc5[:, cls, :, :, i2]
    if planes is None:
        return raw + np.float32(0)                   # the kernel adds a zero plane: a -0 of G is stored as +0
    cls_of = np.array([depth_class(dd, d) for dd in range(d)])
    return (raw + planes[:, :, cls_of]).astype(np.float32)


def sheared_expand_loops(g, gcol, planes, shape, q, m0, off, off_col):
    """The same definition one element at a time (tiny shapes only): what ``sheared_expand_ref`` is checked against on the CPU."""
    n, c, d, h, w = shape
    out = np.zeros(shape, np.float32)
    for idx in np.ndindex(*shape):
        ni, co, dd, hh, ww = idx
        cls = depth_class(dd, d)
        src, i = (gcol, q * (w - 1) - dd - m0 + off_col) if ww == w - 1 else (g, q * ww - dd - m0 + off)
        v = src[ni, cls * c + co, hh, i] if 0 <= i < src.shape[3] else np.float32(0)
        out[idx] = np.float32(v) + (planes[ni, co, cls, hh, ww] if planes is not None else np.float32(0))
    return out


def affine_ref(x, scale, bias, relu):
    """float32(float32(x * scale) + bias) per channel, then ReLU: the two roundings of the kernels' epilogue (contraction is off)."""
    sh = (1, -1, 1, 1, 1)
    v = ((x * scale.reshape(sh)).astype(np.float32) + bias.reshape(sh)).astype(np.float32)
    return np.where(v > 0, v, np.float32(0)).astype(np.float32) if relu else v


def stats_ref(x, gamma, beta, eps):
    """(scale, shift, mean, var) of train-mode BatchNorm over the float64 values of ``x`` [N,C,D,H,W]: biased variance."""
    x64 = x.astype(np.float64)
    mean, var = x64.mean((0, 2, 3, 4)), x64.var((0, 2, 3, 4))
    scale = gamma.astype(np.float64) / np.sqrt(var + eps)
    return scale, beta.astype(np.float64) - mean * scale, mean, var


def line_sums(src, q, m0, wg, off, wg2, off_col):
    """The adjoint of the expand's index rule on a float64 [N,C,D,H,W] array: (sums along every shear line [N,3,C,H,wg], the last
    column's slots [N,3,C,H,wg2] -- one term each --, the number of terms of every line slot [3, wg])."""
    n, c, d, h, w = src.shape
    line, last = np.zeros((n, 3, c, h, wg)), np.zeros((n, 3, c, h, wg2))
    terms = np.zeros((3, wg), np.int64)
    cols = np.arange(w - 1)
    for dd in range(d):
        cls = depth_class(dd, d)
        i = q * cols - dd - m0 + off
        ok = (i >= 0) & (i < wg)
        line[:, cls][..., i[ok]] += src[:, :, dd][..., cols[ok]]            # i is strictly increasing in w: no index twice
        terms[cls, i[ok]] += 1
        i2 = q * (w - 1) - dd - m0 + off_col
        assert 0 <= i2 < wg2, "sheared_geometry keeps every plane's last-column slot inside G'"
        last[:, cls, :, :, i2] += src[:, :, dd, :, w - 1]
    return line, last, terms


def class_sums(src):
    """[N,C,D,H,W] -> [N,C,3,H,W]: first plane, sum of the interior planes, last plane."""
    return np.stack([src[:, :, 0], src[:, :, 1:-1].sum(2), src[:, :, -1]], axis=2)


def wgrad_ref(x, gy):
    """dK[co,c,kh,t] = sum over n, h, i of gy[n,co,h,i] * x[n,c,h+kh-1,i+t-3] in float64 (zero outside the image)."""
    n, c, h, wu = x.shape
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (1, 1), (3, 3)))
    out = np.zeros((gy.shape[1], c, 3, 7))
    g64 = gy.astype(np.float64)
    for kh in range(3):
        for t in range(7):
            out[:, :, kh, t] = np.einsum("nohi,nchi->oc", g64, xp[:, :, kh:kh + h, t:t + wu])
    return out


def wgrad_loops(x, gy):
    """The same correlation one product at a time (tiny shapes only)."""
    n, c, h, wu = x.shape
    out = np.zeros((gy.shape[1], c, 3, 7))
    for ni, o, hh, i in np.ndindex(*gy.shape):
        for ci in range(c):
            for kh in range(3):
                for t in range(7):
                    y, j = hh + kh - 1, i + t - 3
                    if 0 <= y < h and 0 <= j < wu:
                        out[o, ci, kh, t] += float(gy[ni, o, hh, i]) * float(x[ni, ci, y, j])
    return out


def wgrad_kernel_order_f32(x, gy, chunks, cols):
    """The weight gradient accumulated in float32 in the kernel's order -- per sample, row and column chunk a running float32 sum over
    the chunk's columns, the partial sums then added in float32 over chunks, rows and samples --: the error a float32 accumulation of
    this length carries, from which the test's fall-back bound would be taken (4 x its distance to float64)."""
    n, c, h, wu = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (3, 3)))
    out = np.zeros((gy.shape[1], c, 3, 7), np.float32)
    for ni in range(n):
        for hh in range(h):
            for k in range(chunks):
                lo, hi = k * cols, min(wu, (k + 1) * cols)
                part = np.zeros_like(out)
                for i in range(lo, hi):
                    for kh in range(3):
                        part[:, :, kh, :] += gy[ni, :, hh, i][:, None, None] * xp[ni, :, hh + kh, i:i + 7][None]
                out += part
    return out


# ------------------------------------------------------------------------------------------------------------------------------- inputs
def expand_inputs(shape, seed, with_planes=True):
    """g, gcol, planes, scale, bias and the geometry of a sheared-expand case: standard normal data, scale in +-[0.5, 2)."""
    n, c, h, w, d, q, m0 = shape
    off, wu, off_col, wu_col = sheared_geometry(q, m0, d, w)
    r = np.random.default_rng(seed)
    f = lambda *s: r.standard_normal(s, dtype=np.float32)      # noqa: E731
    g, gcol = f(n, 3 * c, h, wu), f(n, 3 * c, h, wu_col)
    planes = f(n, c, 3, h, w) if with_planes else None
    scale = (r.uniform(0.5, 2.0, c) * r.choice([-1.0, 1.0], c)).astype(np.float32)
    bias = r.standard_normal(c).astype(np.float32)
    return g, gcol, planes, scale, bias, (off, wu, off_col, wu_col)


def warped_shifts(n, d, w, seed=0):
    """[n, d] float32 shift rows that mix fractional, whole, zero and beyond-the-image values, in no order."""
    r = np.random.default_rng(1000 + 10 * d + seed)
    s = r.uniform(0.0, w - 1.0, (n, d))
    s[:, 1::6] = np.floor(s[:, 1::6])
    s[:, 2::5] = 0.0
    s[:, 3::4] = r.uniform(w - 2.0, w + 3.0, s[:, 3::4].shape)
    s[0, 0], s[-1, 1] = float(w), float(w - 1)
    return s.astype(np.float32)
