"""The normalisation / activation epilogue passes of csrc/elementwise.hip against the float64 restatement in tests/epilogue_ref.py
(itself pinned to float64 torch by tests/test_epilogue_ref_host.py): snvc_norm_stats, snvc_affine_act[_amax|_twin],
snvc_act_backward_reduce[_amax], snvc_act_backward_apply[_amax|_twin], snvc_bn_backward_coefs, snvc_bn_track, called through
snvc_amd.ops.  Reference semantics: train-mode nn.BatchNorm3d / nn.GroupNorm + ReLU / sigmoid + a residual before or after it, and
their backward.  Every bound is derived (u = 2^-24, float32's unit roundoff) and stated where it is applied; the one measured constant
is the sigmoid's (SIGMOID_MEASURED).

Shapes (N, C, spatial), from the launch code (kNormSplits = 32 splits per row, 256 threads, stream_blocks / twin_blocks):
  tiny         S = 1, 3, 20: rows shorter than a wave, chunk = ceil(S / 32) = 1 so splits >= S are empty; S % 4 != 0 and == 0
  vec_tail     S = 8*16*773 = 98944 = 4 * 32 * 773: VEC = 4, a split has 773 float4 = 3 * 256 + 5: threads 0..4 run the two-loads loop
               twice, the others once and then the single loop, and the last stride is partial (5 of 256)
  scalar_tail  S = 3*5*773 = 11595, odd: VEC = 1, chunk = 363 = 256 + 107: the two-loads loop for threads 0..106, the single loop for the rest
  slice4       x / out / residual = channels [1:7] of an (N, 9, 2, 3, 5) buffer: batch stride 270 != C*S = 180, base pointer 30 floats
               in (8 mod 16 bytes), so the scalar path runs although S*C % 4 == 0 would vectorise a copy; and channels [4:12] of 16 with
               S = 32: 16-byte aligned, vector path, batch stride 512 != 256
  sweep2       (2, 64, (8, 16, 773)): 12.7 M elements; stream_blocks = min(ceil((S/4 + 1) / 1024), ceil(2048 / 128)) = 16 workgroups =
               4096 threads for S/4 = 24736 float4 per row: seven grid-stride sweeps, the last partial.  The twin kernels start
               min(ceil(24736 / 256), ceil(2048 / 16)) = 97 workgroups (one sweep; a second needs N*C*S > 16.8 M) and 24736 = 386 * 64 + 32:
               the last wave of a row is half full and stores its twin directly
  groups       (3, 12, (2, 3, 6)): GroupNorm rows of 3, 12 and 1 channels (groups = 4, 1, 12)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import epilogue_ref as ER
from test_gpu_parity import dev

pytestmark = pytest.mark.gpu

U = ER.U
EPS = float(np.float32(1e-5))
RELU, PRE, POST, SIG = ER.EPI_RELU, ER.EPI_ADD_PRE, ER.EPI_ADD_POST, ER.EPI_SIGMOID
FLAG_SETS = [0, RELU, RELU | PRE, POST, RELU | POST, PRE]            # EPI_SIGMOID: test_sigmoid

TINY = [(2, 6, (1, 1, 1)), (1, 6, (1, 1, 3)), (3, 6, (1, 4, 5))]
GROUPS = (3, 12, (2, 3, 6))
VEC_TAIL = (2, 8, (8, 16, 773))
SCALAR_TAIL = (2, 6, (3, 5, 773))
SWEEP2 = (2, 64, (8, 16, 773))
SLICES = {"slice4_scalar": ((3, 9, (2, 3, 5)), 1, 7), "slice4_vector": ((3, 16, (2, 4, 4)), 4, 12)}      # buffer shape, channels lo:hi


def _id(v):
    names = {VEC_TAIL: "vec_tail", SCALAR_TAIL: "scalar_tail", GROUPS: "groups", TINY[0]: "tiny_s1", TINY[1]: "tiny_s3", TINY[2]: "tiny_s20"}
    return names.get(v, v) if isinstance(v, (tuple, str)) else None


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())


def _np(t):
    return t.detach().cpu().numpy()


def _sliced(a, spec):
    """``a`` [N, C, ...] as a channel slice of a larger device buffer (the other channels hold NaN: reading them shows)."""
    if spec is None:
        return _t(a)
    (n, ctot, sp), lo, hi = spec
    buf = torch.full((n, ctot) + sp, float("nan"), dtype=torch.float32, device=dev())
    view = buf[:, lo:hi]
    view.copy_(_t(a))
    assert view.stride(0) != view[0].numel() and view.data_ptr() % 16 == (0 if lo == 4 else 8)
    return view


def _shape_of(case):
    if case in SLICES:
        (n, _, sp), lo, hi = SLICES[case]
        return (n, hi - lo, sp), SLICES[case]
    return case, None


def _within(got, ref, bound, what):
    """|got - ref| <= bound element by element (+ 1e-45: a denormal's half spacing)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    over = np.abs(got - ref) - (bound + 1e-45)
    k = np.unravel_index(np.argmax(over), over.shape) if over.ndim else ()
    assert over[k] <= 0.0, f"{what}: |got - ref| = {abs(got[k] - ref[k]):.3e} > bound {np.broadcast_to(bound, ref.shape)[k]:.3e} at {k} (ref {ref[k]:.6e})"


def _amax_value(words):
    return words.max().view(torch.float32).item()


class Case:
    """Inputs of the elementwise passes for one shape: ordinary data (standard normal * 3, scale magnitudes in [0.5, 2], every
    per-channel vector different per (n, c) when per_sample), one exact-zero block at (n, c) = (0, 0) -- raw = 0, shift = 0, res = 0, so
    the pre-activation is exactly 0 on both sides -- and no ReLU edge (ER.clear_relu_edges, asserted in `edges_clear`)."""

    def __init__(self, shape, per_sample, seed, edge_flags=(RELU, RELU | PRE),
                 variants=lambda s: ((s.scale, s.shift), (None, s.shift), (s.scale, None))):
        n, c, sp = shape
        r = np.random.default_rng(seed)
        f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        outer = n if per_sample else 1
        self.shape, self.per_sample = shape, per_sample
        self.raw, self.res, self.gy = f(r.standard_normal((n, c) + sp) * 3), f(r.standard_normal((n, c) + sp)), f(r.standard_normal((n, c) + sp))
        self.scale = f(r.uniform(0.5, 2, (outer, c)) * r.choice([-1.0, 1.0], (outer, c)))
        self.shift = f(r.standard_normal((outer, c)))
        self.A, self.B, self.Cc = f(r.standard_normal(outer * c)), f(r.standard_normal(outer * c) * 0.1), f(r.standard_normal(outer * c) * 0.1)
        self.raw[0, 0], self.res[0, 0], self.shift[0, 0] = 0.0, 0.0, 0.0
        # one raw serves every flag set and every scale / shift = None variant: clear the edges of each in turn until none finds any
        for _ in range(6):
            moved = 0
            for fl in edge_flags:
                for sc, sh in variants(self):
                    moved += ER.clear_relu_edges(self.raw, sc, sh, self.res, fl, per_sample)
            if not moved:
                break

    def edges_clear(self, scale, shift, res, flags):
        """The condition on the INPUTS that makes the reference unambiguous, checked on the reference alone: no element with
        0 < |v| < 8 u M, and the exact-zero block still there."""
        v = ER.preact_ref(self.raw, scale, shift, res, flags, self.per_sample)[0]
        m = ER.affine_act_ref(self.raw, scale, shift, res, flags, self.per_sample)[1]
        assert not ((np.abs(v) > 0) & (np.abs(v) < 8 * U * m)).any()
        assert not self.raw[0, 0].any() and not self.res[0, 0].any() and not self.shift[0, 0].any() and (v[0, 0] == 0.0).all()


# =============================================================================== norm_stats
def _check_norm_stats(x_np, x_dev, gamma, beta, groups, per_sample, cap, what):
    """mean, var:  the kernel sums x and x^2 of a row of `count` elements in float64, in some order: each of the two sums is off by at
    most count * 2^-53 * sum|terms| (every partial sum is bounded by the sum of the magnitudes, one rounding per addition), so
        |mean - ref| <= count * 2^-53 * mean|x|                            (+ u |ref| for the float32 it is stored in)
        |var - ref|  <= count * 2^-53 * (mean x^2 + 2 |mean| mean|x|) + 2^-53 * ... <= 4 * count * 2^-53 * mean x^2   (+ u ref)
    as var = E x^2 - mean^2 and mean|x|^2 <= mean x^2.  scale = gamma * rstd, shift = beta - mean * rstd * gamma are formed in float64 from
    the unrounded mean / var: with ev, em the two bounds without their float32 term and rstd' = d rstd / d var = rstd^3 / 2 taken at the
    lowest admissible variance (where it is largest),
        |scale - ref| <= |gamma| ev rstd' + u |scale|,   |shift - ref| <= |gamma| (em rstd + |mean| ev rstd' + em ev rstd') + u |shift|.
    ``cap``: on ordinary data the propagated part must itself stay below 1e-6 of the result -- the formula may not grow into a tolerance.
    A float32 accumulator misses this on the offset data (x = 100 + N(0, 1)): squares near 1e4 carry up to u * 1e4 = 6e-4 of rounding
    each, about 3.5e-4 / sqrt(count) in their mean -- 3e-5 at count = 108, five hundred times the bound of 6e-8 + 5e-11."""
    from snvc_amd import ops
    scale, shift, mean, var = (_np(t).astype(np.float64) for t in ops.norm_stats(x_dev, _t(gamma), _t(beta), groups, per_sample, EPS))
    r_scale, r_shift, r_mean, r_var = ER.norm_stats_ref(x_np, gamma, beta, groups, per_sample, EPS)
    em, ev, b_scale, b_shift = ER.norm_stats_bounds(x_np, gamma, groups, per_sample, EPS)       # the arithmetic of the lines above
    assert (var >= 0.0).all(), f"{what}: negative variance"
    _within(mean, r_mean, em + U * np.abs(r_mean), what + " mean")
    _within(var, r_var, ev + U * r_var, what + " var")
    rep = lambda a: np.repeat(a, x_np.shape[1] // groups, axis=1)
    if cap:
        assert (b_scale <= 1e-6 * np.abs(r_scale)).all() and (b_shift <= 1e-6 * (np.abs(r_shift) + np.abs(rep(r_mean) * r_scale))).all(), what
    _within(scale, r_scale, b_scale + U * (np.abs(r_scale) + b_scale), what + " scale")
    _within(shift, r_shift, b_shift + U * (np.abs(r_shift) + b_shift), what + " shift")


def _norm_modes(c, small):
    modes = [(c, False), (c // 3 if c % 3 == 0 else c // 4, True)]
    return modes + ([(1, True), (c, True)] if small else [])


_NORM_CASES = TINY + [GROUPS, VEC_TAIL, SCALAR_TAIL, "slice4_scalar", "slice4_vector"]
_SMALL = TINY + [GROUPS, "slice4_scalar", "slice4_vector"]      # the constant row is a property of the finalisation: small shapes cover it


@pytest.mark.parametrize("case,data", [(k, d) for k in _NORM_CASES for d in ("ordinary", "offset")] + [(k, "constant") for k in _SMALL], ids=_id)
def test_norm_stats(case, data):
    """Batch statistics (rows (n, c) folded over n) and GroupNorm rows of cpg channels ((n, group) indexing of mean / var; groups = 1
    and groups = C on the small shapes), on ordinary, offset (mean 100 x the spread) and constant-row data (variance exactly 0: must come
    back >= 0, finite).  gamma / beta = None once each.  Bounds: _check_norm_stats."""
    shape, spec = _shape_of(case)
    n, c, sp = shape
    small = case in _SMALL
    r = np.random.default_rng(17)
    x = r.standard_normal((n, c) + sp)
    x = x * 3 if data == "ordinary" else x + 100.0
    x = np.ascontiguousarray(x, dtype=np.float32)
    gamma, beta = r.uniform(0.5, 2, c).astype(np.float32), r.standard_normal(c).astype(np.float32)
    x_dev = None
    for groups, per_sample in _norm_modes(c, small):
        if data == "constant":           # one statistics row constant, at a value whose square is not a float32
            if per_sample:
                x.reshape(n, groups, -1)[n - 1, groups - 1] = np.float32(3.7)
            else:
                x[:, c - 1] = np.float32(3.7)
            x_dev = None
        if x_dev is None:
            x_dev = _sliced(x, spec)
        what = f"{case} groups={groups} per_sample={per_sample} {data}"
        _check_norm_stats(x, x_dev, gamma, beta, groups, per_sample, data == "ordinary" and int(np.prod(sp)) > 1, what)
    _check_norm_stats(x, x_dev, None, beta, c, False, False, f"{case} gamma=None")
    _check_norm_stats(x, x_dev, gamma, None, _norm_modes(c, small)[1][0], True, False, f"{case} beta=None")


# =============================================================================== affine_act
def _check_affine(cs, flags, scale, shift, spec, twin=False):
    """y = act(x*sc + sh [+ res]) [+ res] in float32 (no contraction) rounds x*sc, the sum with sh, and the sum with res: at most three
    roundings, each of an intermediate that M = |x sc| + |sh| + |res| + |y| bounds, so |got - ref| <= 3 u M; ReLU is 1-Lipschitz and
    carries the bound through (no edge: see Case).  The amax words hold max|y| exactly."""
    from snvc_amd import ops
    res = cs.res if flags & (PRE | POST) else None
    cs.edges_clear(scale, shift, res, flags)
    ref, m = ER.affine_act_ref(cs.raw, scale, shift, res, flags, cs.per_sample)
    x_dev, res_dev = _sliced(cs.raw, spec), (_sliced(res, spec) if res is not None else None)
    out = _sliced(np.zeros_like(cs.raw), spec) if spec is not None else None
    am = ops.amax_word(dev())
    mul = ops.split_scale_of(ops.affine_act(x_dev, _t(scale), _t(shift), res_dev, flags, cs.per_sample)) if twin else None
    got = ops.affine_act(x_dev, _t(scale), _t(shift), res_dev, flags, cs.per_sample, out=out, amax=am, twin_mul=mul)
    assert out is None or got is out
    what = f"affine_act {cs.shape} flags={flags} per_sample={cs.per_sample} scale={scale is not None} shift={shift is not None} twin={twin}"
    _within(_np(got), ref, 3 * U * m, what)
    assert _amax_value(am) == got.abs().max().item(), what + " amax"
    if flags & RELU and not flags & POST:
        assert (_np(got)[0, 0] == 0.0).all(), what + " exact-zero block"
    if twin:
        pair, _ = ops.twin_of(got)
        assert torch.equal(pair, ops.to_split(got, mul_dev=mul)), what + " pair"


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("case", TINY + [GROUPS, SCALAR_TAIL, "slice4_scalar", "slice4_vector"], ids=_id)
def test_affine_act(case, per_sample):
    """Every flag set; scale, shift, residual different per (n, c); scale = None and shift = None once each.  Bound: _check_affine."""
    shape, spec = _shape_of(case)
    cs = Case(shape, per_sample, 21)
    for flags in FLAG_SETS:
        _check_affine(cs, flags, cs.scale, cs.shift, spec)
    _check_affine(cs, RELU | PRE, None, cs.shift, spec)
    _check_affine(cs, RELU, cs.scale, None, spec)


@pytest.fixture(scope="module")
def sweep2_case():
    return Case(SWEEP2, True, 23, edge_flags=(RELU | PRE,), variants=lambda s: ((s.scale, s.shift),))


@pytest.mark.parametrize("twin", [False, True])
def test_affine_act_sweep2(sweep2_case, twin):
    """The capped grid's later sweeps (plain kernel) and the half-full tail wave of the twin kernel, per-sample coefficients"""
    _check_affine(sweep2_case, RELU | PRE, sweep2_case.scale, sweep2_case.shift, None, twin=twin)


# =============================================================================== act_backward_reduce / _apply
def _check_backward(cs, flags, spec, want_g, scale="given", shift="given", B="given", Cc="given", twin=False):
    """g = gy * act'(v) is gy or 0 exactly (no sigmoid here), so
      * g_out is bit-equal to the reference;
      * the sums [sum g, sum g raw] per (n, c) are float64 sums of exact products (24 x 24 bits) of S terms in some order: off by at
        most S * 2^-53 * sum|terms|;
      * draw = A g + B raw + Cc rounds the two products, their sum and the final sum: u (|A g| + |B raw|) + u |A g + B raw| + u |draw|
        <= 3 u M with M = |A g| + |B raw| + |Cc| + |draw|.
    The amax words hold max|draw| and max|gy| exactly."""
    from snvc_amd import ops
    scale = cs.scale if scale == "given" else None
    shift = cs.shift if shift == "given" else None
    B = cs.B if B == "given" else None
    Cc = cs.Cc if Cc == "given" else None
    res = cs.res if flags & PRE else None
    cs.edges_clear(scale, shift, res, flags & ~POST)
    g = ER.act_grad_ref(cs.raw, cs.gy, res, scale, shift, flags, cs.per_sample)
    r_sums, r_abs = ER.act_backward_sums_ref(cs.raw, g)
    r_draw, m = ER.act_backward_apply_ref(cs.raw, g, cs.A, B, Cc, cs.per_sample)
    raw_dev, gy_dev, res_dev = _sliced(cs.raw, spec), _sliced(cs.gy, spec), (_sliced(res, spec) if res is not None else None)
    what = f"backward {cs.shape} flags={flags} per_sample={cs.per_sample} want_g={want_g} twin={twin}"
    s = int(np.prod(cs.shape[2]))
    amg = ops.amax_word(dev())
    sums = ops.act_backward_reduce(raw_dev, gy_dev, res_dev, _t(scale), _t(shift), flags, cs.per_sample, amax_gy=amg)
    _within(_np(sums), r_sums, s * 2.0 ** -53 * r_abs, what + " sums")
    assert _amax_value(amg) == float(np.abs(cs.gy).max()), what + " amax_gy"
    am = ops.amax_word(dev())
    mul = None
    if twin:
        mul = ops.split_scale_bound(cs.A.size, cs.shape[1], dev(), a=_t(cs.A), amax_p=amg, b=_t(B), l1=_t(np.ones(cs.shape[1])),
                                    amax_x=ops.amax_from_bound(raw_dev.abs().max()), cc=_t(Cc))
    draw, g_out = ops.act_backward_apply(raw_dev, gy_dev, res_dev, _t(scale), _t(shift), _t(cs.A), _t(B), _t(Cc), flags, cs.per_sample,
                                         want_g, amax=am, twin_mul=mul)
    _within(_np(draw), r_draw, 3 * U * m, what + " draw")
    assert _amax_value(am) == draw.abs().max().item(), what + " amax"
    assert (g_out is not None) == want_g
    if want_g:
        assert np.array_equal(_np(g_out), g.astype(np.float32)), what + " g_out"
    if twin:
        pair, _ = ops.twin_of(draw)
        assert torch.equal(pair, ops.to_split(draw, mul_dev=mul)), what + " pair"
    if flags == PRE:        # no activation: the kernel documents that it does not read the residual -- none must give the same bits
        sums0 = ops.act_backward_reduce(raw_dev, gy_dev, None, _t(scale), _t(shift), 0, cs.per_sample)
        draw0, _ = ops.act_backward_apply(raw_dev, gy_dev, None, _t(scale), _t(shift), _t(cs.A), _t(B), _t(Cc), 0, cs.per_sample, False)
        assert torch.equal(sums0, sums) and torch.equal(draw0, draw), what + " residual read without an activation"


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("case", TINY + [GROUPS, VEC_TAIL, SCALAR_TAIL, "slice4_scalar", "slice4_vector"], ids=_id)
def test_act_backward(case, per_sample):
    """Every flag set (ADD_POST does not enter the backward pass: with and without it), want_g both ways, coef_raw / coef_const / scale
    / shift = None once each, A / B / Cc different per (n, c).  Bounds: _check_backward."""
    shape, spec = _shape_of(case)
    cs = Case(shape, per_sample, 29)
    small = cs.raw.size < 10000
    for i, flags in enumerate(FLAG_SETS if small else [RELU | PRE, PRE]):
        _check_backward(cs, flags, spec, want_g=bool(i % 2))
    _check_backward(cs, RELU | PRE, spec, want_g=False)
    _check_backward(cs, RELU, spec, True, B=None)
    _check_backward(cs, RELU, spec, False, Cc=None)
    _check_backward(cs, RELU | PRE, spec, True, scale=None)
    _check_backward(cs, RELU, spec, False, shift=None)


@pytest.mark.parametrize("twin", [False, True])
def test_act_backward_apply_sweep2(sweep2_case, twin):
    """As test_affine_act_sweep2 for the apply pass (and the reduction at 64 x 2 rows of 24736 float4)"""
    _check_backward(sweep2_case, RELU | PRE, None, want_g=True, twin=twin)


# =============================================================================== sigmoid
# Largest absolute error of the device's sigmoid and of its derivative s (1 - s) against float64, measured on an MI355X over the ten
# cases of test_sigmoid on 2026-10-17 (the largest at vec_tail, per-sample); the outputs lie in [0, 1] and [0, 1/4].
SIGMOID_MEASURED = {"forward": 1.034e-07, "derivative": 9.034e-08}


def _sigmoid_errors(case, per_sample):
    from snvc_amd import ops
    shape, spec = _shape_of(case)
    cs = Case(shape, per_sample, 31, edge_flags=())
    ref, _ = ER.affine_act_ref(cs.raw, cs.scale, cs.shift, None, SIG, per_sample)
    raw_dev = _sliced(cs.raw, spec)
    got = ops.affine_act(raw_dev, _t(cs.scale), _t(cs.shift), None, SIG, per_sample)
    ones = np.ones_like(cs.raw)
    one = np.ones(cs.A.size, dtype=np.float32)
    # gy = 1, A = 1, no B / Cc: draw = g = s (1 - s) exactly as the kernel forms it
    draw, g_out = ops.act_backward_apply(raw_dev, _sliced(ones, spec), None, _t(cs.scale), _t(cs.shift), _t(one), None, None, SIG, per_sample, True)
    assert torch.equal(draw, g_out)
    g = ER.act_grad_ref(cs.raw, ones, None, cs.scale, cs.shift, SIG, per_sample)
    sums = ops.act_backward_reduce(raw_dev, _sliced(ones, spec), None, _t(cs.scale), _t(cs.shift), SIG, per_sample)
    return np.abs(_np(got) - ref).max(), np.abs(_np(g_out) - g).max(), _np(sums), g, cs


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("case", [TINY[2], GROUPS, VEC_TAIL, SCALAR_TAIL, "slice4_scalar"], ids=_id)
def test_sigmoid(case, per_sample):
    """EPI_SIGMOID forward, y = 1 / (1 + expf(-v)), and derivative, g = gy * s (1 - s).  The error of the device's expf is not derivable
    from the source, so this bound is MEASURED: the largest absolute error against float64 over these shapes on an MI355X on 2026-10-17
    was 1.034e-07 forward and 9.034e-08 for the derivative (SIGMOID_MEASURED); the test allows four times that, and that allowance must itself stay below 1e-6 (absolute; outputs in [0, 1]).
    The sums of the reduction pass then follow: S terms, each within the derivative's bound (times |raw| for the second sum), plus the
    float64 summation error."""
    e_fwd, e_der, sums, g, cs = _sigmoid_errors(case, per_sample)
    print(f"sigmoid {case} per_sample={per_sample}: forward {e_fwd:.3e} derivative {e_der:.3e}")
    b_fwd, b_der = 4 * SIGMOID_MEASURED["forward"], 4 * SIGMOID_MEASURED["derivative"]
    assert 0.0 < b_fwd < 1e-6 and 0.0 < b_der < 1e-6
    assert e_fwd <= b_fwd and e_der <= b_der
    r_sums, r_abs = ER.act_backward_sums_ref(cs.raw, g)
    n, c = cs.shape[:2]
    s = int(np.prod(cs.shape[2]))
    raw_abs = np.abs(ER.f64(cs.raw)).reshape(n, c, -1).sum(2)
    _within(sums, r_sums, np.stack([np.full((n, c), s * b_der), b_der * raw_abs], axis=2) + s * 2.0 ** -52 * r_abs, f"sigmoid sums {case}")


# =============================================================================== bn_backward_coefs / bn_track
@pytest.mark.parametrize("with_gamma", [True, False])
@pytest.mark.parametrize("n,c", [(3, 12), (1, 70), (2, 64)])
def test_bn_backward_coefs(n, c, with_gamma):
    """Each output is float64 algebra on the given sums, mean and var, rounded once to float32: u of the value, and 2^-53-sized errors
    of the float64 steps relative to the terms of the expression (which cancel: sum g raw - mean sum g) -- together within 2^-23 of
    the sum of the magnitudes of the terms.  C = 70: a second, partial block of the 64-thread launch."""
    from snvc_amd import ops
    r = np.random.default_rng(37)
    count = 360.0
    sums = r.standard_normal((n, c, 2)) * 50
    sums[..., 1] += 100 * sums[..., 0]                                       # sum g raw ~ mean * sum g: the cancelling case
    mean, var = (100 + r.standard_normal(c)).astype(np.float32), r.uniform(0.5, 2, c).astype(np.float32)
    var[0] = 0.0
    gamma = r.uniform(0.5, 2, c).astype(np.float32) if with_gamma else None
    got = ops.bn_backward_coefs(torch.from_numpy(sums).to(dev()), _t(mean), _t(var), _t(gamma), count, EPS)
    ref, mag = ER.bn_backward_coefs_ref(sums, mean, var, gamma, count, EPS)
    for t, key in zip(got, ("coef_g", "coef_raw", "coef_const", "dgamma", "dbeta")):
        _within(_np(t), ref[key], 2.0 ** -23 * mag[key], f"bn_backward_coefs {key} N={n} C={c}")


@pytest.mark.parametrize("count", [1, 50])
@pytest.mark.parametrize("momentum", [0.1, 0.25])
def test_bn_track(momentum, count):
    """running <- running + momentum * (batch - running) over two updates, the variance unbiased by count / max(count - 1, 1) (count = 1:
    unchanged), num_batches_tracked exact.  In float32 with momentum <= 1/4: the difference (u (|a| + |b|)), the float32 momentum and
    the fused multiply-add's single rounding (u |result|), for the variance also the float32 unbias factor and its product (2 u |b|):
    u ((1 + 2 m) |a| + (1 + 4 m) |b|) <= 2^-23 (|running| + |batch|) per update.  Each update is compared from the kernel's own state."""
    from snvc_amd import ops
    r = np.random.default_rng(41)
    c = 70
    norm = torch.nn.BatchNorm3d(c, momentum=momentum).to(dev())
    norm.running_mean.copy_(_t(r.standard_normal(c)))
    norm.running_var.copy_(_t(r.uniform(0.5, 2, c)))
    for step in range(2):
        mean, var = r.standard_normal(c).astype(np.float32), r.uniform(0.5, 2, c).astype(np.float32)
        rm0, rv0 = _np(norm.running_mean).copy(), _np(norm.running_var).copy()
        assert ops.bn_track(norm, _t(mean), _t(var), float(count))
        rm, rv, nbt, (m_mean, m_var) = ER.bn_track_ref(rm0, rv0, step, mean, var, count, momentum)
        _within(_np(norm.running_mean), rm, 2.0 ** -23 * m_mean, f"running_mean step {step}")
        _within(_np(norm.running_var), rv, 2.0 ** -23 * m_var, f"running_var step {step}")
        assert int(norm.num_batches_tracked) == nbt


# =============================================================================== the passes chained as the product runs them
def _chain_data(shape, groups, per_sample, flags, seed):
    """Ordinary data without ReLU edges for the chained statistics: the statistics move with raw, so clear and recompute until stable."""
    n, c, sp = shape
    r = np.random.default_rng(seed)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    x, res, gy = f(r.standard_normal((n, c) + sp) * 3), f(r.standard_normal((n, c) + sp)), f(r.standard_normal((n, c) + sp))
    gamma, beta = f(r.uniform(0.5, 2, c)), f(r.standard_normal(c))
    for _ in range(8):
        scale, shift, _, _ = ER.norm_stats_ref(x, gamma, beta, groups, per_sample, EPS)
        if not ER.clear_relu_edges(x, scale, shift, res if flags & (PRE | POST) else None, flags, per_sample):
            break
    return x, res, gy, gamma, beta


def _torch_autograd(x, res, gy, gamma, beta, groups, per_sample, flags):
    t = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    x_, res_, gamma_, beta_ = t(x), t(res), t(gamma), t(beta)
    v = F.group_norm(x_, groups, gamma_, beta_, EPS) if per_sample else F.batch_norm(x_, None, None, gamma_, beta_, True, 0.1, EPS)
    if flags & PRE:
        v = v + res_
    if flags & RELU:
        v = F.relu(v)
    if flags & POST:
        v = v + res_
    (v * torch.tensor(gy, dtype=torch.float64)).sum().backward()
    dres = res_.grad.numpy() if res_.grad is not None else np.zeros(x.shape)
    return v.detach().numpy(), x_.grad.numpy(), gamma_.grad.numpy(), beta_.grad.numpy(), dres


@pytest.mark.parametrize("flags", [RELU | PRE, RELU, POST], ids=["relu_pre", "relu", "post"])
@pytest.mark.parametrize("norm", ["batchnorm", "groupnorm"])
@pytest.mark.parametrize("case", [GROUPS, "slice4_scalar", "slice4_vector"], ids=_id)
def test_chain_vs_float64_autograd(case, norm, flags):
    """norm_stats -> affine_act, then act_backward_reduce -> coefficients -> act_backward_apply (BatchNorm: snvc_bn_backward_coefs by
    hand, and the same data through submodule._epilogue_backward, bit-equal to the hand chain; GroupNorm: submodule._epilogue_backward,
    cpg = 3 / 3 / 2), against float64 torch autograd of norm -> [+res] -> relu -> [+res].
      y:     3 u M as _check_affine, plus |x| |scale - scale64| + |shift - shift64| for the float32 scale / shift the pass was handed
             (exact: the epilogue is 1-Lipschitz in v); the statistics themselves are held to _check_norm_stats;
      draw:  3 u M as _check_backward, plus the coefficients' own error: each of A, B, Cc is float64 algebra on float32 mean and var
             (u each; rstd enters up to three times at u / 2) rounded to float32 (u): at most 4.5 u, taken as 2^-21, of the magnitudes
             of its terms: 2^-21 (mag A |g| + mag B |raw| + mag Cc);
      dgamma, dbeta: the same 2^-21 of the magnitudes of their terms;  the residual's gradient: gy or 0, bit for bit.
    The ReLU mask of the float32 pass equals the reference's: no |v| below 8 u M, of which the float32 scale / shift move v by at most
    4 u M (asserted) and the pass's own roundings by 3 u M."""
    from snvc_amd import ops
    from snvc_amd.models import submodule as S
    shape, spec = _shape_of(case)
    n, c, sp = shape
    per_sample = norm == "groupnorm"
    groups = (c // 3 if c % 3 == 0 else c // 2) if per_sample else c
    x, res, gy, gamma, beta = _chain_data(shape, groups, per_sample, flags, 43)
    ref = ER.chain_ref(x, res, gy, gamma, beta, groups, per_sample, flags, EPS)
    y64, dx64, dgamma64, dbeta64, dres64 = _torch_autograd(x, res, gy, gamma, beta, groups, per_sample, flags)
    assert not ER.relu_edge(ER.preact_ref(x, ref["scale"], ref["shift"], res if flags & PRE else None, flags, per_sample)[0], ref["m_y"]).any()
    what = f"chain {case} {norm} flags={flags}"
    x_dev, gy_dev = _sliced(x, spec), _t(gy)
    res_dev = _sliced(res, spec) if flags & (PRE | POST) else None
    # forward
    _check_norm_stats(x, x_dev, gamma, beta, groups, per_sample, True, what)
    scale, shift, mean, var = ops.norm_stats(x_dev, _t(gamma), _t(beta), groups, per_sample, EPS)
    y = ops.affine_act(x_dev, scale, shift, res_dev, flags, per_sample)
    moved = np.abs(ER.f64(x)) * np.abs(_np(scale).astype(np.float64) - ref["scale"])[:, :, None, None, None] + \
        np.abs(_np(shift).astype(np.float64) - ref["shift"])[:, :, None, None, None]
    assert (moved <= 4 * U * ref["m_y"]).all(), what
    _within(_np(y), y64, 3 * U * ref["m_y"] + moved, what + " y")
    # backward
    mags = ref["coef_mags"]
    if per_sample:
        gn = torch.nn.GroupNorm(groups, c, eps=EPS).to(dev())
        with torch.no_grad():
            gn.weight.copy_(_t(gamma)); gn.bias.copy_(_t(beta))
        rec = S._Epilogue(y, x_dev, scale, shift, mean, var, True)
        draw, gres, dgamma, dbeta = S._epilogue_backward(rec, gy_dev, res_dev, gn, flags, want_res=res_dev is not None, want_gamma=True,
                                                          want_beta=True)
    else:
        act_flags = flags & (RELU | PRE)
        sums = ops.act_backward_reduce(x_dev, gy_dev, res_dev, scale, shift, act_flags, False)
        cg, cr, cc, dgamma, dbeta = ops.bn_backward_coefs(sums, mean[0].contiguous(), var[0].contiguous(), _t(gamma), float(n * int(np.prod(sp))), EPS)
        draw, g_out = ops.act_backward_apply(x_dev, gy_dev, res_dev, scale, shift, cg, cr, cc, act_flags, False, bool(flags & PRE))
        gres = g_out if flags & PRE else (gy_dev if flags & POST else None)
        # the same three launches through the product's own entry, train-mode BatchNorm3d: the same bits
        bn = torch.nn.BatchNorm3d(c, eps=EPS).to(dev()).train()
        with torch.no_grad():
            bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta))
        rec = S._Epilogue(y, x_dev, scale, shift, mean, var, False)
        got = S._epilogue_backward(rec, gy_dev, res_dev, bn, flags, want_res=res_dev is not None, want_gamma=True, want_beta=True)
        for name, a, b in zip(("draw", "residual gradient", "dgamma", "dbeta"), got, (draw, gres, dgamma, dbeta)):
            assert (a is None) == (b is None), what + " " + name
            assert a is None or (a.dtype == b.dtype and np.array_equal(_np(a), _np(b))), what + " _epilogue_backward " + name
    bc = (lambda a: a[:, :, None, None, None]) if per_sample else (lambda a: a[None, :, None, None, None])
    coef_err = 2.0 ** -21 * (bc(mags["coef_g"]) * np.abs(ref["g"]) + bc(mags["coef_raw"]) * np.abs(ER.f64(x)) + bc(mags["coef_const"]))
    _within(_np(draw), dx64, 3 * U * ref["m_draw"] + coef_err, what + " draw")
    _within(_np(dgamma), dgamma64, 2.0 ** -21 * mags["dgamma"], what + " dgamma")
    _within(_np(dbeta), dbeta64, 2.0 ** -21 * mags["dbeta"], what + " dbeta")
    if gres is not None:
        assert np.array_equal(_np(gres), dres64.astype(np.float32)), what + " residual gradient"


def test_flag_bits_are_the_abi():
    from snvc_amd import ops
    assert (ops.EPI_RELU, ops.EPI_ADD_PRE, ops.EPI_ADD_POST, ops.EPI_SIGMOID) == (RELU, PRE, POST, SIG)
