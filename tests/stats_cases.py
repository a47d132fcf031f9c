"""The cases, the float64 reference and the bound of the batch statistics that the convolution kernels take in their own epilogues
(train-mode BatchNorm: ops.Conv3dLayer.forward_stats, ops.Conv3dLayerX3.forward_stats, ops.sheared_expand_stats).  numpy and CPU torch
only: tests/test_stats_cases_host.py pins this table on the CPU, tests/test_gpu_stats_epilogue.py runs it on the kernels.

Reference: the float64 moments (two passes) of the float32 raw tensor that the call itself returned -- not a float64 convolution: the
accumulation is judged apart from the convolution's own rounding.  Bound: epilogue_ref.norm_stats_bounds, the error of sums taken in
float64 from the first element on, plus u |ref| for the float32 each result is stored in; nothing in it is measured.

Data kinds (each on every case):
  ordinary       what the older tests use: zero-mean weights on zero-mean (fp32 route, sheared) or ReLU'd (split route) inputs.  The
                 propagated bound must itself stay below 1e-6 of the result (``cap``).
  offset         per-channel |mean| of the raw result 50 .. 400 times its standard deviation: E x^2 - mean^2 cancels six to eight
                 digits, which a float32 accumulator does not have.
  near-constant  as `offset`, and the last output channel's raw values are one value (3.7f, whose square is no float32): the
                 variance is 0 and a lossy accumulator's E x^2 - mean^2 goes negative.
A convolution has no bias and zero padding, so the offset rides on input channel 0, an exact constant c = 2^k (exact in a split pair
too), through weights that give EVERY output voxel the same sum: Conv3d (stride 1 or 2): the centre tap alone, 1; the transposed layer
(k3, s2, p1, op1): the separable product of the per-axis taps (0, 1, 1) -- even outputs see tap 1 only, odd outputs tap 2 only, the last
row included.  The other input channels are N(0, 1) through 0.05 N(0, 1) weights."""
import numpy as np

import epilogue_ref as ER

U = ER.U
EPS = 1e-5
N = 2
NEAR_CONSTANT = np.float32(3.7)
KINDS = ("ordinary", "offset", "near-constant")
RATIO = (50.0, 400.0)           # |mean| / std of every raw channel of the `offset` kind

# name: (Cin, Cout, input extents, stride, transposed, c of the offset kinds); forward_stats returns None on `unsupported_w78`
FP32_LAYERS = {"k3s1_32": (32, 32, (8, 8, 64), 1, False, 128.0), "k3s1_64_ragged": (6, 64, (5, 7, 72), 1, False, 64.0),
               "k3s2_32_64": (32, 64, (8, 16, 128), 2, False, 128.0), "k3s2_ragged": (4, 32, (10, 14, 72), 2, False, 64.0),
               "deconv_64_32": (64, 32, (4, 8, 64), 2, True, 128.0), "deconv_ragged": (6, 64, (3, 5, 36), 2, True, 32.0),
               "unsupported_w78": (8, 32, (4, 4, 78), 1, False, 64.0)}
FP32_UNSUPPORTED = ("unsupported_w78",)
X3_LAYERS = {"s1 64->64 (16x16x32 form)": (64, 64, (8, 8, 64), 1, False, 256.0), "s1 32->32": (32, 32, (6, 9, 40), 1, False, 128.0),
             "s1 64->32 small": (64, 32, (4, 4, 32), 1, False, 256.0), "s2 32->64": (32, 64, (8, 8, 64), 2, False, 128.0),
             "s2 64->64": (64, 64, (6, 12, 40), 2, False, 256.0), "deconv 64->32": (64, 32, (4, 6, 40), 2, True, 128.0),
             "deconv 64->64": (64, 64, (3, 5, 36), 2, True, 128.0),
             "s1 64->64 forced 16x16x32": (64, 64, (8, 8, 64), 1, False, 256.0)}
# The kernel form (SNVC_ALGO_X3_*, by name) that ops.x3_form gives each split case at N = 2 -- asked of the rule itself by the host test
# and of the layer after its launch by the GPU test.  At these sizes the rule never takes the 16x16x32 form (it wants 256 jobs; the
# stride-1 cases have 32, 24 and 2): one case forces it (``algo=``), which is how its statistics epilogue is reached at all here.
X3_FORCED = {"s1 64->64 forced 16x16x32": "Q16"}
X3_FORM = {"s1 64->64 (16x16x32 form)": "SMALL", "s1 32->32": "SMALL", "s1 64->32 small": "SMALL", "s2 32->64": "0", "s2 64->64": "0",
           "deconv 64->32": "0", "deconv 64->64": "SMALL", "s1 64->64 forced 16x16x32": "Q16", "fold two rounds (4160 slots)": "0",
           "fold one round (4096 slots)": "0"}
# The two-round fold of the per-wave slots (conv_stats_fold_rows_kernel, more than 4096 slots per sample).  The transposed split forms
# with 32 output channels tile the INPUT 4 x 4 x 32 and leave 32 slots per tile (4 z classes x 2 x classes x 4 waves): 130 tiles =
# 4160 slots take the first round, 128 tiles = 4096 slots do not.  Cin = 8: one channel group, the least a split layer takes; thin
# ragged tiles (H = 1, W = 4) keep the result at 4 MB -- and the count per channel at 33 k: the float64 bound grows with the count, a
# float32 accumulator's miss shrinks with its root, and the host test wants the two a factor 100 apart.
X3_FOLD_LAYERS = {"fold two rounds (4160 slots)": (8, 32, (517, 1, 4), 2, True, 32.0),
                  "fold one round (4096 slots)": (8, 32, (509, 1, 4), 2, True, 32.0)}
X3_FOLD_SLOTS = {"fold two rounds (4160 slots)": 4160, "fold one round (4096 slots)": 4096}
X3_TRANSPOSED_TILE = (4, 4, 32)
FOLD_SINGLE_ROUND_MAX = 4096
# (q, m0): the sheared first layer, (N, C, D, H, W) = (2, 3, 10, 6, 24); the offset goes into `planes`
SHEARED = {"q2 m0": (2, 0), "q2 m5": (2, 5), "q1 m1": (1, 1)}
SHEARED_SHAPE = (N, 3, 10, 6, 24)
SHEARED_C = 128.0


def layer_of(route, name):
    return {"fp32": FP32_LAYERS, "x3": {**X3_LAYERS, **X3_FOLD_LAYERS}}[route][name]


def out_extents(sp, stride, transposed):
    return tuple(2 * e for e in sp) if transposed else tuple((e + 2 - 3) // stride + 1 for e in sp)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def conv_inputs(route, name, kind):
    """(x [N, Cin, D, H, W], w [Cout, Cin, 3, 3, 3] or [Cin, Cout, 3, 3, 3] transposed), float32."""
    ci, co, sp, st, tr, c = layer_of(route, name)
    wshape = ((ci, co) if tr else (co, ci)) + (3, 3, 3)
    if kind == "ordinary":
        if route == "fp32":          # test_conv_statistics_epilogue_vs_separate_pass
            r = np.random.default_rng(231)
            w = _f32(0.1 * r.standard_normal(wshape))
            return _f32(r.standard_normal((N, ci) + sp)), w
        r = np.random.default_rng(9)                                  # test_split_layer_f32_output_residual_and_statistics
        x = _f32(np.maximum(_f32(r.standard_normal((N, ci) + sp)), 0.0))
        return x, _f32(r.standard_normal(wshape) * 0.05)
    r = np.random.default_rng(77)
    x = _f32(r.standard_normal((N, ci) + sp))
    w = _f32(0.05 * r.standard_normal(wshape))
    x[:, 0] = np.float32(c)
    carrier = np.zeros((3, 3, 3), np.float32)
    if tr:
        t = np.array([0.0, 1.0, 1.0], np.float32)
        carrier[:] = t[:, None, None] * t[None, :, None] * t[None, None, :]
        w[0, :] = carrier
    else:
        carrier[1, 1, 1] = 1.0
        w[:, 0] = carrier
    if kind == "near-constant":      # the last output channel: c * (3.7f / c) from channel 0 and nothing else
        v = carrier * (NEAR_CONSTANT / np.float32(c))
        if tr:
            w[:, co - 1] = 0.0
            w[0, co - 1] = v
        else:
            w[co - 1] = 0.0
            w[co - 1, 0] = v
    return x, w


def conv_ref(x, w, stride, transposed):
    """The float64 convolution (CPU torch) of float32 inputs."""
    import torch
    import torch.nn.functional as F
    xt, wt = torch.from_numpy(np.asarray(x, dtype=np.float64)), torch.from_numpy(np.asarray(w, dtype=np.float64))
    if transposed:
        return F.conv_transpose3d(xt, wt, stride=2, padding=1, output_padding=1).numpy()
    return F.conv3d(xt, wt, stride=stride, padding=1).numpy()


def sheared_inputs(name, kind):
    """(g, gcol, planes, (off, off_col)) of the sheared first layer, float32; test_sheared_fused_batchnorm_entry_points_vs_numpy's."""
    from snvc_amd.models.submodule import sheared_geometry
    q, m0 = SHEARED[name]
    n, c, d, h, w = SHEARED_SHAPE
    off, wu, off_col, wu_col = sheared_geometry(q, m0, d, w)
    r = np.random.default_rng(211 + q + m0)
    g, gcol = _f32(r.standard_normal((n, 3 * c, h, wu))), _f32(r.standard_normal((n, 3 * c, h, wu_col)))
    planes = _f32(r.standard_normal((n, c, 3, h, w)))
    if kind != "ordinary":
        planes += np.float32(SHEARED_C)
    if kind == "near-constant":      # the last channel: nothing from G, G', the planes hold the value
        g.reshape(n, 3, c, h, wu)[:, :, c - 1] = 0.0
        gcol.reshape(n, 3, c, h, wu_col)[:, :, c - 1] = 0.0
        planes[:, c - 1] = NEAR_CONSTANT
    return g, gcol, planes, (off, off_col)


def sheared_ref(name, g, gcol, planes, offs):
    """raw[n, c, d, h, w] = G[n, cls(d), c, h, q w - d - m0 + off] + planes[n, c, cls(d), h, w], G' at w = W - 1 (ops.sheared_expand's
    definition; a line index left of G's reach reads 0), in float64."""
    q, m0 = SHEARED[name]
    n, c, d, h, w = SHEARED_SHAPE
    off, off_col = offs
    G, Gc = ER.f64(g).reshape(n, 3, c, h, -1), ER.f64(gcol).reshape(n, 3, c, h, -1)
    raw = np.zeros(SHEARED_SHAPE)
    for dd in range(d):
        cls = 0 if dd == 0 else (2 if dd == d - 1 else 1)
        raw[:, :, dd] = ER.f64(planes)[:, :, cls]
        for ww in range(w - 1):
            i = q * ww - dd - m0 + off
            if 0 <= i < G.shape[4]:
                raw[:, :, dd, :, ww] += G[:, cls, :, :, i]
        raw[:, :, dd, :, w - 1] += Gc[:, cls, :, :, q * (w - 1) - dd - m0 + off_col]
    return raw


def stats_errors(raw, gamma, beta, got):
    """{name: (|got - ref|, bound)} of scale, shift, mean, var ([1, C] each) against the float64 moments of ``raw`` [N, C, ...], the
    bounds with their float32 storage terms, as tests/test_gpu_epilogue.py::_check_norm_stats applies them; also the reference and
    the propagated bounds alone (for the `cap`)."""
    c = raw.shape[1]
    r_scale, r_shift, r_mean, r_var = ER.norm_stats_ref(raw, gamma, beta, c, False, EPS)
    em, ev, b_scale, b_shift = ER.norm_stats_bounds(raw, gamma, c, False, EPS)
    ref = {"scale": r_scale, "shift": r_shift, "mean": r_mean, "var": r_var}
    bound = {"scale": b_scale + U * (np.abs(r_scale) + b_scale), "shift": b_shift + U * (np.abs(r_shift) + b_shift),
             "mean": em + U * np.abs(r_mean), "var": ev + U * r_var}
    err = {}
    for k, v in zip(("scale", "shift", "mean", "var"), got):
        v = np.asarray(v, dtype=np.float64).reshape(ref[k].shape)
        err[k] = (np.abs(v - ref[k]), bound[k] + 1e-45)
    return err, ref, (em, ev, b_scale, b_shift)


def cap_holds(ref, bounds):
    """On ordinary data the propagated bound stays below 1e-6 of the result: the formula may not grow into a tolerance."""
    _, _, b_scale, b_shift = bounds
    return bool((b_scale <= 1e-6 * np.abs(ref["scale"])).all() and
                (b_shift <= 1e-6 * (np.abs(ref["shift"]) + np.abs(ref["mean"] * ref["scale"]))).all())


def check_stats(raw, gamma, beta, got, cap, what):
    """Every statistic finite, var >= 0, and within its bound of the float64 moments of ``raw``.  Prints the largest error over its
    bound per statistic first (a run that keeps its output records by how much a kernel misses)."""
    got = [np.asarray(v, dtype=np.float64) for v in got]
    err, ref, bounds = stats_errors(raw, gamma, beta, got)
    worst = {k: float((e / b).max()) for k, (e, b) in err.items()}
    print(f"stats {what}: |got - ref| / bound  " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"  min var {got[3].min():.3e}")
    assert all(np.isfinite(v).all() for v in got), f"{what}: non-finite statistics"
    assert (got[3] >= 0.0).all(), f"{what}: negative variance {got[3].min():.3e}"
    if cap:
        assert cap_holds(ref, bounds), f"{what}: the propagated bound exceeds 1e-6 of the result"
    for k, (e, b) in err.items():
        i = np.unravel_index(np.argmax(e - b), e.shape)
        assert e[i] <= b[i], f"{what}: {k} off by {e[i]:.3e} > bound {b[i]:.3e} at channel {i[-1]} (ref {ref[k][i]:.6e})"


def lossy_stats(raw):
    """(mean, var) [1, C] of a float32 tensor by an accumulator that sums x and x^2 in float32 over runs of 8 consecutive values and in
    float64 from there: gentler than a kernel that keeps float32 over a lane's values and a 32-lane shuffle tree."""
    raw = np.asarray(raw, dtype=np.float32)
    c = raw.shape[1]
    rows = np.moveaxis(raw.reshape(raw.shape[0], c, -1), 0, 1).reshape(c, -1)
    count = rows.shape[1]
    rows = np.pad(rows, ((0, 0), (0, -count % 8))).reshape(c, -1, 8)
    s, q = np.zeros(rows.shape[:2], np.float32), np.zeros(rows.shape[:2], np.float32)
    for i in range(8):
        v = rows[:, :, i]
        s = (s + v).astype(np.float32)
        q = (q + (v * v).astype(np.float32)).astype(np.float32)
    mean = s.astype(np.float64).sum(1) / count
    var = q.astype(np.float64).sum(1) / count - mean * mean
    return mean[None], var[None]


def gamma_beta(c):
    r = np.random.default_rng(5)
    return _f32(r.uniform(0.5, 1.5, c)), _f32(r.standard_normal(c))


def x3_slots(name):
    """Statistics slots per sample of a transposed split layer with 32 output channels: 32 per 4 x 4 x 32 input tile."""
    sp = layer_of("x3", name)[2]
    return 32 * int(np.prod([-(-e // t) for e, t in zip(sp, X3_TRANSPOSED_TILE)]))


def x3_workspace_doubles(n, cout, slots):
    """What snvc_f16x3_conv3d_stats_workspace_bytes sizes, in doubles: the slots, the first round's scratch (one row of 64 per group
    for every 64 slots) when one round does not do, and the per-sample sums."""
    groups = cout // 32
    scratch = n * (-(-slots // 64)) * groups * 64 if slots > FOLD_SINGLE_ROUND_MAX else 0
    return n * slots * groups * 64 + scratch + n * cout * 2, scratch


def x3_algo(form):
    from snvc_amd import _lib
    return {"0": 0, "SERIAL": _lib.ALGO_X3_SERIAL, "NARROW": _lib.ALGO_X3_NARROW, "SMALL": _lib.ALGO_X3_SMALL, "Q16": _lib.ALGO_X3_Q16}[form]
