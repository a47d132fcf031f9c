"""Every kernel that writes (or reads) a split pair, held to the host definition of the format in tests/split_format.py -- bit for
bit wherever the arithmetic in front of the split is exact or a single float32 rounding of an exact float64 value, and to a bound
derived in the case's docstring where it is not (``warped_expand_split`` alone).  NaN positions are compared as NaN, not by payload.

Layout passes (layout_f16.hip): to_split, from_split, to_c8, from_c8, mul_broadcast_split, mul_broadcast_c8.
Norm pass (snvc_f16x3_affine_from_ncdhw): affine_act_split, every residual mode, the clamp and its flag at the boundary.
Split conv forms (conv3d_f16.hip): every split form of f16_plan_cases.FORMS with Cout > 1 as a channel-copy layer, whose
accumulator is exact, so that the epilogue's stored bits and flag follow from split_format.clamp_pair.
First-layer producers (sheared_conv.hip): sheared_expand_split against a restatement of its index rule, warped_expand_split
against ops.warped_expand; flag rows for both.

The ``*_case`` functions are also rows of tests/test_gpu_guard_split.py (run between guard bands): every device operand is made by
a torch call, every pair by ``torch.empty`` + ``copy_`` (a pair must be 16-byte aligned), and nothing depends on state outside.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import f16_plan_cases as PC
import split_format as SF

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 2
U = 2.0 ** -24                                   # float32's unit roundoff
SENTINEL = 1234.0
LAYOUT_C = (5, 8, 20)
LAYOUT_SP = ((1, 1, 1), (2, 3, 67))              # S = 402 = 256 + 146: a second, partial block
LAYOUT = [(c, sp) for c in LAYOUT_C for sp in LAYOUT_SP]
LAYOUT_IDS = [f"c{c}-s{int(np.prod(sp))}" for c, sp in LAYOUT]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16_plan_gpu.json")


# ------------------------------------------------------------------------------------------------------------------ helpers
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_pair(a):
    """A half array as a device tensor from ``torch.empty`` (256-byte aligned under every placement of the guard-band suite)."""
    t = torch.empty(a.shape, dtype=torch.float16, device=DEV)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    return t


def host(t):
    return t.detach().cpu().numpy()


def assert_bits(got, exp, what):
    """Equal bits of two arrays of one float type; where the expected value is a NaN, any NaN."""
    g = host(got) if isinstance(got, torch.Tensor) else got
    assert g.shape == exp.shape and g.dtype == exp.dtype, (what, g.shape, exp.shape, g.dtype, exp.dtype)
    u = {2: np.uint16, 4: np.uint32}[g.dtype.itemsize]
    gn, en = np.isnan(g), np.isnan(exp)
    bad = (gn != en) | (~en & (np.ascontiguousarray(g).view(u) != np.ascontiguousarray(exp).view(u)))
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, the first at {i}: got {g[i]!r} "
                             f"(bits {int(np.ascontiguousarray(g).view(u)[i]):#x}), expected {exp[i]!r} "
                             f"(bits {int(np.ascontiguousarray(exp).view(u)[i]):#x})")


def assert_ragged_zero(pair, c, what):
    """The lanes of a ragged channel group hold +0 in both planes."""
    if c % 8:
        pad = host(pair)[:, :, -1, ..., c % 8:]
        assert not pad.view(np.uint16).any(), f"{what}: the lanes behind channel {c} of the last group are not +0"


def layout_data(c, sp, seed=0, scale=1.0):
    return (SF.edge_data((N, c) + tuple(sp), 100 * c + int(np.prod(sp)) + seed) * np.float32(scale)).astype(np.float32)


def expected_pair(x, mul):
    return SF.pair_tensor(*SF.split_pair(x, mul))


# ----------------------------------------------------------------------------------------------------------- layout passes
@pytest.mark.parametrize("exp", [-2, 0, 3])
@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_to_split_is_the_definition(c, sp, exp):
    """ops.to_split on the edge set (ties of both parities, subnormal and vanishing lo, the bottom and the top of half's range, both
    signs) and log-uniform magnitudes: equal bits in both planes; |x * 2^exp| >= 65520 gives (+-inf, -+inf), as the definition says;
    the lanes of a ragged group are +0."""
    from snvc_amd import ops
    x = layout_data(c, sp)
    pair = ops.to_split(dev(x), exp)
    want = expected_pair(x, 2.0 ** exp)
    assert pair.shape == (N, 2, (c + 7) // 8) + tuple(sp) + (8,)
    assert_bits(pair, want, f"to_split(exp={exp})")
    assert_ragged_zero(pair, c, "to_split")
    hi, lo = SF.split_pair(x, 2.0 ** exp)
    over = np.abs(x.astype(np.float64) * 2.0 ** exp) >= 65520
    assert over.any() or exp < 0 or x.size < 100
    assert np.array_equal(hi[over], np.sign(x[over]) * np.float16(np.inf)) and np.array_equal(lo[over], -hi[over])
    SF.lo_within_half_ulp(hi, lo)


@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_to_split_with_a_device_scale(c, sp):
    """``mul_dev`` from split_scale_of: the data is the edge set * 2^-5, whose maximum the scale rule puts into [2^13, 2^14) (* 8 for
    the larger shapes): a multiplier other than the host exponents', read on the device."""
    from snvc_amd import ops
    x = layout_data(c, sp, 1, 2.0 ** -5)
    xd = dev(x)
    mul = ops.split_scale_of(xd)
    pair = ops.to_split(xd, mul_dev=mul)
    m = float(mul.item())
    assert m == 2.0 ** round(np.log2(m)) and 2.0 ** 13 <= float(np.abs(x).max()) * m < 2.0 ** 14 and (m == 8.0 or x.size < 100), m
    assert_bits(pair, expected_pair(x, m), "to_split(mul_dev)")
    assert torch.isfinite(pair.float()).all()


@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_to_split_into_a_slice_and_from_a_slice(c, sp):
    """``out=`` a channel-group slice of a larger pair filled with a sentinel: the surroundings keep it.  ``x`` a channel slice of a
    wider tensor (a padded batch stride): the same bits."""
    from snvc_amd import ops
    g = (c + 7) // 8
    wide = layout_data(c + 3, sp, 2)
    xs = dev(wide)[:, 2:2 + c]
    assert not xs.is_contiguous()
    big = torch.full((N, 2, g + 2) + tuple(sp) + (8,), SENTINEL, dtype=torch.float16, device=DEV)
    out = big[:, :, 1:1 + g]
    back = ops.to_split(xs, 3, out=out)
    assert back.data_ptr() == out.data_ptr()
    want = expected_pair(wide[:, 2:2 + c], 8.0)
    assert_bits(big[:, :, 1:1 + g].contiguous(), want, "to_split(out=slice)")
    assert (big[:, :, 0] == SENTINEL).all() and (big[:, :, g + 1] == SENTINEL).all()


def test_to_split_of_non_finite_input():
    from snvc_amd import ops
    x = layout_data(5, (2, 3, 67), 3)
    x.reshape(-1)[[0, 7, 401, 402, 1300, 2009]] = [np.inf, -np.inf, np.nan, np.inf, np.nan, -np.inf]
    want = expected_pair(x, 1.0)
    assert np.isnan(want).sum() >= 6                    # lo of an infinite hi is inf - inf
    assert_bits(ops.to_split(dev(x), 0), want, "to_split(non-finite)")


def random_half_patterns(shape, seed):
    """Arbitrary half bit patterns (NaN, inf, subnormals included), with every subnormal magnitude class and the extremes in front."""
    r = np.random.default_rng(seed)
    b = r.integers(0, 1 << 16, size=shape, dtype=np.uint16)
    front = np.array([0x0001, 0x8001, 0x03FF, 0x83FF, 0x0400, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x7E00, 0x0000, 0x8000, 0x0200], np.uint16)
    k = min(front.size, b.size)
    b.reshape(-1)[:k] = front[:k]
    return b.view(np.float16)


@pytest.mark.parametrize("exp", [0, 3])
@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_from_split_is_pair_value(c, sp, exp):
    """ops.from_split on arbitrary bit patterns in both planes (non-canonical pairs, subnormals, inf, NaN): float32((hi + lo) * 2^-exp)."""
    from snvc_amd import ops
    g = (c + 7) // 8
    p = random_half_patterns((N, 2, g) + tuple(sp) + (8,), 7 * c + exp)
    want = SF.from_c8(SF.pair_value(p[:, 0], p[:, 1], 2.0 ** -exp), c)
    got = ops.from_split(dev_pair(p), exp, c)
    assert_bits(got, want, f"from_split(exp={exp})")


@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_c8_layout_passes(c, sp):
    """to_c8 = one rounding to half (ties, subnormals, overflow to inf), zero lanes in a ragged group; from_c8 widens any pattern."""
    from snvc_amd import ops
    x = layout_data(c, sp, 4)
    with np.errstate(over="ignore"):
        want = SF.to_c8(x.astype(np.float16))
    assert np.isinf(want).any() or x.size < 100
    got = ops.to_c8(dev(x))
    assert_bits(got, want, "to_c8")
    if c % 8:
        assert not host(got)[:, -1, ..., c % 8:].view(np.uint16).any()
    h = random_half_patterns((N, (c + 7) // 8) + tuple(sp) + (8,), c)
    assert_bits(ops.from_c8(dev_pair(h), c), SF.from_c8(h.astype(np.float32), c), "from_c8")


OCC = np.array([0.0, -0.0, 1.0, 2.0 ** -3, 0.3, -1.7], np.float32)


def mul_broadcast_split_case(c, sp):
    """ops.mul_broadcast_split on host-built pairs of the edge set * 2^-3: split_pair(float32(pair_value(hi, lo, 1) * occ), 1), the
    occupancy holding 0, -0, 1, 2^-3, 0.3 and -1.7; once into a fresh pair and once with ``out=``."""
    from snvc_amd import ops
    x = layout_data(c, sp, 5, 2.0 ** -3)
    p = expected_pair(x, 1.0)
    s = int(np.prod(sp))
    occ = np.resize(OCC, N * s).reshape((N, 1) + tuple(sp)).astype(np.float32)
    v = (SF.pair_value(p[:, 0], p[:, 1], 1.0) * occ.reshape((N, 1) + tuple(sp) + (1,))).astype(np.float32)
    want = np.ascontiguousarray(np.stack(SF.split_pair(v, 1.0), axis=1))
    feat, od = dev_pair(p), dev(occ)
    assert_bits(ops.mul_broadcast_split(feat, od), want, "mul_broadcast_split")
    out = torch.empty(p.shape, dtype=torch.float16, device=DEV)
    assert ops.mul_broadcast_split(feat, od, out=out) is out
    assert_bits(out, want, "mul_broadcast_split(out=)")
    SF.lo_within_half_ulp(want[:, 0], want[:, 1])


@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_mul_broadcast_split(c, sp):
    mul_broadcast_split_case(c, sp)


@pytest.mark.parametrize("c,sp", LAYOUT, ids=LAYOUT_IDS)
def test_mul_broadcast_c8(c, sp):
    """The C8 form of the same product: one rounding of float32(h) * occ."""
    from snvc_amd import ops
    x = layout_data(c, sp, 6, 2.0 ** -3)
    h = SF.to_c8(x.astype(np.float16))
    s = int(np.prod(sp))
    occ = np.resize(OCC, N * s).reshape((N, 1) + tuple(sp)).astype(np.float32)
    with np.errstate(over="ignore"):
        want = (h.astype(np.float32) * occ.reshape((N, 1) + tuple(sp) + (1,))).astype(np.float32).astype(np.float16)
    feat, od = dev_pair(h), dev(occ)
    assert_bits(ops.mul_broadcast_c8(feat, od), want, "mul_broadcast_c8")
    out = torch.empty(h.shape, dtype=torch.float16, device=DEV)
    ops.mul_broadcast_c8(feat, od, out=out)
    assert_bits(out, want, "mul_broadcast_c8(out=)")


# --------------------------------------------------------------------------------------------------------------- norm pass
def f32(a64):
    """One float32 rounding of float64 values that are exact: what a float32 operation (an FMA included) stores."""
    return np.asarray(a64, np.float64).astype(np.float32)


def epilogue_ref(v, res, res_mul, mode, relu, out_mul=1.0):
    """The clamping epilogues after their affine, step by step in float32: v (float32) [+ r] -> ReLU -> [+ r] -> * out_mul; r =
    float32(hi + lo) * res_mul (exact).  Returns the float32 value the clamp sees.  Every step is one rounding of an exact float64."""
    if res is not None:
        rr = f32((res[0].astype(np.float64) + res[1].astype(np.float64)) * res_mul)
    if mode == "pre":
        v = f32(v.astype(np.float64) + rr)
    if relu:
        v = np.where(v > 0, v, np.float32(0.0)).astype(np.float32)
    if mode == "post":
        v = f32(v.astype(np.float64) + rr)
    return f32(v.astype(np.float64) * out_mul)


AFFINE_C, AFFINE_SP, AFFINE_OUT_EXP, AFFINE_RES_EXP = 12, (2, 3, 67), 2, 1
# the value stored at the boundary voxel (sample 1, channel 11, the last voxel), with ReLU or without -> (stored, flag)
BOUNDARY = {"none": None, "65472": 65472.0, "65504": 65504.0, "70000": 70000.0, "-70000": -70000.0}


def boundary_expectation(row, relu):
    t = BOUNDARY[row]
    if t is None:
        return None, False
    if t < 0:
        return (0.0, False) if relu else (-65504.0, True)
    return min(t, 65504.0), t >= 65504.0


@functools.lru_cache(maxsize=None)
def affine_inputs(per_sample):
    r = np.random.default_rng(31 + per_sample)
    shape = (N, AFFINE_C) + AFFINE_SP
    raw = (r.integers(-512 * 64, 512 * 64, shape) / 64.0).astype(np.float32)                 # a 2^-6 grid
    rows = N if per_sample else 1
    scale = (r.choice([-1.0, 1.0], (rows, AFFINE_C)) * np.exp2(r.integers(-2, 3, (rows, AFFINE_C)))).astype(np.float32)
    shift = (r.integers(-8 * 64, 8 * 64, (rows, AFFINE_C)) / 64.0).astype(np.float32)
    res = SF.split_pair((r.standard_normal(shape) * 4).astype(np.float32), 2.0 ** AFFINE_RES_EXP)      # a host pair: any canonical one
    return raw, scale, shift, res


@pytest.mark.parametrize("row", list(BOUNDARY))
@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("mode", ["none", "pre", "post"])
@pytest.mark.parametrize("per_sample", [True, False], ids=["per_sample", "shared"])
def test_affine_act_split_stored_bits_and_flag(per_sample, mode, relu, row):
    """snvc_f16x3_affine_from_ncdhw.  Scale +-2^k per channel, raw and shift on a 2^-6 grid, the residual a host pair: fma(raw, scale,
    shift), + r and * 2^out_exp are each one float32 rounding of an exact float64 value, so the stored pair is clamp_pair of the
    restatement, bit for bit, and the flag is that of the stored values.  Boundary rows: the last voxel of channel 11 (the ragged
    group) of sample 1 lands on 65472 (no flag), on 65504 (flag), above (clamped, flag) and below -65504 (ReLU: stored 0, no flag)."""
    from snvc_amd import ops
    raw, scale, shift, res = affine_inputs(per_sample)
    raw = raw.copy()
    res = (res[0].copy(), res[1].copy())
    out_mul, res_mul = 2.0 ** AFFINE_OUT_EXP, 2.0 ** -AFFINE_RES_EXP
    at = (1, 11, 1, 2, 66)
    if BOUNDARY[row] is not None:
        sc, sh = float(scale[-1, 11]), float(shift[-1, 11])
        x = (BOUNDARY[row] / out_mul - sh) / sc
        assert float(np.float32(x)) == x
        raw[at] = x
        res[0][at] = res[1][at] = 0
    sc_full = np.broadcast_to(scale, (N, AFFINE_C)).reshape(N, AFFINE_C, 1, 1, 1).astype(np.float64)
    sh_full = np.broadcast_to(shift, (N, AFFINE_C)).reshape(N, AFFINE_C, 1, 1, 1).astype(np.float64)
    v = f32(raw.astype(np.float64) * sc_full + sh_full)
    v = epilogue_ref(v, res if mode != "none" else None, res_mul, mode, relu, out_mul)
    hi, lo, flag = SF.clamp_pair(v, False)
    stored, eflag = boundary_expectation(row, relu)
    if stored is not None:
        assert float(hi[at]) + float(lo[at]) == stored and flag == eflag, (float(v[at]), flag)
    else:
        assert not flag
    flags = (ops.EPI_RELU if relu else 0) | {"none": 0, "pre": ops.EPI_ADD_PRE, "post": ops.EPI_ADD_POST}[mode]
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    pair = ops.affine_act_split(dev(raw), dev(scale), dev(shift), AFFINE_OUT_EXP, dev_pair(SF.pair_tensor(*res)) if mode != "none" else None,
                                AFFINE_RES_EXP, flags, per_sample, overflow=word)
    assert_bits(pair, SF.pair_tensor(hi, lo), f"affine_act_split({mode}, relu={relu}, {row})")
    assert_ragged_zero(pair, AFFINE_C, "affine_act_split")
    assert int(word.item()) == int(flag), f"flag {int(word.item())}, the stored values say {int(flag)}"


# --------------------------------------------------------------------------------------------------------- split conv forms
CONV_CIN, CONV_EXT, W_EXP = 16, (9, 10, 33), 13
SPECIAL = (1, 3, 8, 8, 32)          # sample, input channel, (d, h, w): the last input column; stride 2 and the transposed layer read it
SPECIAL_STORED = 2046.0             # the stored input there (hi = 2046, lo = 0): * 32 = 65472
CB = 19                             # the output channel that carries the boundary rows (copies input channel 3)
CONV_ROWS = {"65472": (32.0, 0.0), "65504": (32.0, 32.0), "70000": (32.0, 4528.0), "-70000": (-32.0, -4528.0)}      # (S, bias) of channel CB
CONV_KINDS = [("split", True), ("split", False), ("res pre", True), ("res post", True), ("head", True)]               # (kind, ReLU)
with open(GOLDEN) as _f:
    _REJECTS = {(name, kind) for name, kinds in json.load(_f).items() if name in PC.FORMS
                for kind, rec in kinds.items() if kind != "packed" and rec[0] != 0}
CONV_FORMS = [name for name, (split, _, cout, _) in PC.FORMS.items() if split and cout > 1]
CONV_CASES = [(name, kind, relu) for name in CONV_FORMS for kind, relu in CONV_KINDS if (name, kind) not in _REJECTS]


@functools.lru_cache(maxsize=None)
def conv_reference(key, cout):
    """Input pair (host), channel-copy weights and the exact accumulator of a layer of ``key``: F.conv3d / F.conv_transpose3d in
    float64 on the CPU of the stored input hi + lo with the weights * 2^13, the packed (8192, 0).  One nonzero weight per output
    channel: every output is one stored input times 8192 (or 0) -- exact in float32, in any order of accumulation."""
    import torch.nn.functional as F
    k, stride, dil = key[:3]
    transposed = len(key) == 4
    x_exp = 2 if (k + cout // 32) % 2 else 0
    r = np.random.default_rng(500 + 10 * k + stride + dil + cout)
    xv = (r.standard_normal((N, CONV_CIN) + CONV_EXT) * 3).astype(np.float32)
    e = np.concatenate([SF.EDGES, -SF.EDGES])
    e = e[np.abs(e) < 8]                                     # the small edges: ties, subnormal and vanishing lo
    xv.reshape(-1)[:e.size] = e * np.float32(2.0 ** -x_exp)
    xv[SPECIAL] = SPECIAL_STORED * 2.0 ** -x_exp
    xhi, xlo = SF.split_pair(xv, 2.0 ** x_exp)
    assert float(xhi[SPECIAL]) == SPECIAL_STORED and float(xlo[SPECIAL]) == 0.0
    c = k // 2
    if transposed:
        w = np.zeros((CONV_CIN, cout, 3, 3, 3), np.float32)
        for co in range(cout):
            w[co % CONV_CIN, co, 1, 1, 1] = 1.0
    else:
        w = np.zeros((cout, CONV_CIN, k, k, k), np.float32)
        for co in range(cout):
            w[co, co % CONV_CIN, c, c, c] = 1.0
    xs = torch.from_numpy(xhi.astype(np.float64) + xlo.astype(np.float64))
    w64 = torch.from_numpy(w.astype(np.float64) * 2.0 ** W_EXP)
    if transposed:
        acc = F.conv_transpose3d(xs, w64, stride=2, padding=1, output_padding=1)
    else:
        acc = F.conv3d(xs, w64, stride=stride, padding=dil * (k - 1) // 2, dilation=dil)
    acc = acc.numpy()
    assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
    sp = np.argwhere(acc[1, CB] == SPECIAL_STORED * 2.0 ** W_EXP)
    assert len(sp) == 1, "the boundary voxel is read by exactly one output of channel CB"
    return x_exp, xhi, xlo, w, acc, tuple(int(v) for v in sp[0])


def conv_epilogue(acc, scale, bias, res, res_mul, kind, relu):
    """fma(acc, scale, bias) [+ r] -> ReLU -> [+ r] -> clamp_pair, on [N, C', ...] arrays with per-channel scale / bias [C']."""
    shape = (1, -1, 1, 1, 1)
    v = f32(acc * scale.astype(np.float64).reshape(shape) + bias.astype(np.float64).reshape(shape))
    mode = {"res pre": "pre", "res post": "post"}.get(kind, "none")
    v = epilogue_ref(v, res if mode != "none" else None, res_mul, mode, relu)
    return SF.clamp_pair(v, False)


@pytest.mark.parametrize("name,kind,relu", CONV_CASES, ids=[f"{n}-{k.replace(' ', '_')}-{'relu' if r else 'plain'}" for n, k, r in CONV_CASES])
def test_split_conv_form_stores_the_definition(name, kind, relu):
    """One split form of conv3d_f16.hip (selected as f16_plan_cases.run_form selects it: Cin 16, N = 2, input extents 9 x 10 x 33) run as
    a channel-copy layer.  The accumulator is x_hi * 8192 + x_lo * 8192 = (hi + lo) * 8192, exact; the folded scale is +-2^k, the bias on
    a grid, so v = fma(acc, scale, bias) is one rounding of an exact float64 value, as is each residual add (res_exp != out_exp: the
    residual's units are folded by res_mul = 1/2, exact).  Expected: clamp_pair of that value -- equal bits of both planes and the flag.
    Four launches: the stored value of channel 19 at the output that reads the input's last column (the last valid column of a ragged
    tile for the stride-1 and stride-2 layers) is 65472 (no flag), 65504 (flag), 70000 (clamped, lo = 0, flag), -70000 (ReLU without a
    residual behind it: 0, no flag; otherwise -65504, flag).  A (form, kind) that the form rejects (tests/golden/f16_plan_gpu.json) is
    not in the list."""
    from snvc_amd import _lib
    L = _lib.lib()
    split, key, cout, algo = PC.FORMS[name]
    x_exp, xhi, xlo, w, acc, at = conv_reference(key, cout)
    out_exp = 2 - x_exp
    res_exp = out_exp + 1
    base = PC.desc(key, CONV_CIN, cout, algo, ext=CONV_EXT, n=N)
    out_ext = (base["Dout"], base["Hout"], base["Wout"])
    out_sp = int(np.prod(out_ext))
    r = np.random.default_rng(900 + sorted(PC.FORMS).index(name))
    fold = 2.0 ** (out_exp - x_exp - W_EXP)
    s_user = r.choice([-1.0, 1.0], cout) * np.exp2(r.integers(-2, 3, cout))
    b_user = r.integers(-32, 33, cout) / 8.0
    rv = (r.standard_normal((N, cout) + out_ext) * 4).astype(np.float32)
    rv[(1, CB) + at] = 0.0
    res = SF.split_pair(rv, 2.0 ** res_exp)
    res_mul = 2.0 ** (out_exp - res_exp)

    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    lo_of = lambda t: ctypes.c_void_p(t.data_ptr() + t.stride(1) * 2)             # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    d0 = _lib.Conv3dDesc(**base)
    nbytes = int(L.snvc_f16x3_conv3d_packed_weight_bytes(ctypes.byref(d0)))
    assert nbytes > 0, L.snvc_last_error_string().decode()
    packed = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    wt = dev(w)
    assert L.snvc_f16x3_conv3d_pack_weights(ctypes.byref(d0), ptr(wt), ptr(packed), float(2.0 ** W_EXP), stream) == 0
    x = dev_pair(SF.pair_tensor(xhi, xlo))
    withres, withhead = kind.startswith("res"), kind == "head"
    resd = dev_pair(SF.pair_tensor(*res)) if withres else None
    head = dev(r.standard_normal(32).astype(np.float32)) if withhead else None
    flags = (PC.RELU if relu else 0) | {"res pre": PC.ADD_PRE, "res post": PC.ADD_POST}.get(kind, 0)
    d = _lib.Conv3dDesc(**dict(base, flags=flags))
    full = None
    for row, (S, b) in CONV_ROWS.items():
        scale = (s_user * fold).astype(np.float32)
        bias = (b_user * 2.0 ** out_exp).astype(np.float32)
        scale[CB], bias[CB] = S / 2.0 ** W_EXP, b
        if full is None:
            full = conv_epilogue(acc, scale, bias, res, res_mul, kind, relu)
            assert not full[2], "the base data stays below 65504"
            hi, lo, flag = full
        else:           # only channel CB differs from the first row
            one = conv_epilogue(acc[:, CB:CB + 1], scale[CB:CB + 1], bias[CB:CB + 1], (res[0][:, CB:CB + 1], res[1][:, CB:CB + 1]), res_mul, kind, relu)
            hi, lo = full[0].copy(), full[1].copy()
            hi[:, CB:CB + 1], lo[:, CB:CB + 1] = one[0], one[1]
            flag = one[2]
        stored = float(hi[(1, CB) + at]) + float(lo[(1, CB) + at])
        assert (stored, flag) == boundary_expectation(row, relu), (row, stored, flag)      # the residual is 0 at that voxel
        y = torch.zeros((N, 2, cout // 8) + out_ext + (8,), dtype=torch.float16, device=DEV)
        y_head = torch.zeros((N, out_sp), dtype=torch.float32, device=DEV) if withhead else None
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        sd, bd = dev(scale), dev(bias)
        rc = L.snvc_f16x3_conv3d_forward(ctypes.byref(d), ptr(x), lo_of(x), ptr(packed), ptr(sd), ptr(bd),
                                         ptr(resd), lo_of(resd) if withres else None, ptr(y), lo_of(y), None, ptr(head), ptr(y_head),
                                         0.5, float(res_mul), ptr(word), stream)
        assert rc == 0, (name, kind, L.snvc_last_error_string().decode())
        torch.cuda.synchronize()
        assert_bits(y, SF.pair_tensor(hi, lo), f"{name} {kind} relu={relu} row {row}")
        assert int(word.item()) == int(flag), f"{name} {kind} row {row}: flag {int(word.item())}, the stored values say {int(flag)}"


def test_every_split_form_with_more_than_one_channel_is_in_the_list():
    assert len(CONV_FORMS) == 19 and {n for n, _, _ in CONV_CASES} == set(CONV_FORMS)
    assert all((n, "split") not in _REJECTS for n in CONV_FORMS)


# ---------------------------------------------------------------------------------------------------- first-layer producers
FL_C, FL_D, FL_H, FL_W = 12, 17, 2, 68       # D = 17: two depth chunks of 9 and 8 planes in both launchers (H * G * N = 8 workgroups);
FL_AT = (1, 11, 1, 5)                         # W = 68: two waves, the second partial.  Flag voxel: sample, channel, row, column
FL = (N, FL_C, FL_H, FL_W, FL_D)              # the shape of the tests of this file; tests/test_gpu_first_layer_forms.py passes the shapes of
FL_ROWS = list(BOUNDARY)                      # tests/first_layer_cases.SPLIT (more depth chunks, a short one, one without planes)
FL_WG = {1: 60, 2: 100}                       # G's row length at the shape FL


def flag_at(shape):
    """The flag voxel (sample, channel, row, column) and the exact channel's sample: the last sample, channel 11, the last row."""
    return (shape[0] - 1, 11, shape[2] - 1, 5)


def first_layer_affine(r, c=FL_C):
    scale = (r.choice([-1.0, 1.0], c) * np.exp2(r.integers(-2, 3, c))).astype(np.float32)
    bias = (r.integers(-64, 65, c) / 8.0).astype(np.float32)
    scale[11], bias[11] = 1.0, 0.0
    return scale, bias


def sheared_inputs(q, with_planes, row, shape=FL):
    """g / gcol / planes on a 2^-6 grid, scale +-2^k: raw + pe and fma(raw + pe, sc, bi) are exact.  WG and the offsets are such that
    i = q w - d - m0 + off leaves [0, WG) on both sides and the last column's i2 leaves [0, WG2) on both sides.  Channel 11 of the last
    sample has g = gcol = 0, scale 1, bias 0: what is stored there is its depth-class plane.  At D = 17 (the shape FL): off = 5, WG = 60
    or 100, WG2 = 12, i2 = 13 - d; deeper shapes move off, WG and WG2 along with D, so that every plane still has columns inside G."""
    n, c, h, w, d = shape
    r = np.random.default_rng(70 + q + (0 if shape == FL else sum(shape)))
    m0, off = 3, d - 12
    wg = FL_WG[q] if shape == FL else q * (w - 2) + d - 23           # the largest i is q (W - 2) + D - 15: 8 columns past the row
    wg2 = d - 5
    off_col = -q * (w - 1) + m0 + d - 4                    # i2 = D - 4 - d: D - 4, D - 5 (out), D - 6 .. 0, -1 .. -3 (out)
    grid = lambda shape: (r.integers(-512, 513, shape) / 64.0).astype(np.float32)      # noqa: E731
    g, gcol = grid((n, 3 * c, h, wg)), grid((n, 3 * c, h, wg2))
    planes = grid((n, c, 3, h, w))
    at = flag_at(shape)
    for cls in range(3):
        g[at[0], cls * c + 11] = 0
        gcol[at[0], cls * c + 11] = 0
    if BOUNDARY[row] is not None:
        planes[at[0], at[1], 1, at[2], at[3]] = BOUNDARY[row]
    elif not with_planes:
        planes = None
    scale, bias = first_layer_affine(r, c)
    return g, gcol, planes, scale, bias, m0, off, off_col


def sheared_reference(g, gcol, planes, scale, bias, q, m0, off, off_col, relu, shape=FL):
    """A restatement of the kernel's ``emit``: class 0 / 1 / 2 by plane, raw = G[cls][i] with i = q w - d - m0 + off (0 outside
    [0, WG)), the last column from G' at i2 = q (W - 1) - d - m0 + off_col; t = fma(raw + planes, scale, bias); clamp_pair."""
    n, c, h, w, depth = shape
    wg, wg2 = g.shape[3], gcol.shape[3]
    raw = np.zeros((n, c, depth, h, w), np.float32)
    pe = np.zeros_like(raw)
    for d in range(depth):
        cls = 0 if d == 0 else (2 if d == depth - 1 else 1)
        for col in range(w - 1):
            i = q * col - d - m0 + off
            if 0 <= i < wg:
                raw[:, :, d, :, col] = g[:, cls * c:(cls + 1) * c, :, i]
        i2 = q * (w - 1) - d - m0 + off_col
        if 0 <= i2 < wg2:
            raw[:, :, d, :, w - 1] = gcol[:, cls * c:(cls + 1) * c, :, i2]
        if planes is not None:
            pe[:, :, d] = planes[:, :, cls]
    s = (raw + pe).astype(np.float32)
    t64 = s.astype(np.float64) * scale.astype(np.float64).reshape(1, -1, 1, 1, 1) + bias.astype(np.float64).reshape(1, -1, 1, 1, 1)
    return SF.clamp_pair(f32(t64), relu), raw


def flag_voxels(hi, lo, shape=FL):
    """hi + lo at the flag voxel of the interior planes."""
    at = flag_at(shape)
    return (hi.astype(np.float64) + lo.astype(np.float64))[at[0], at[1], 1:shape[4] - 1, at[2], at[3]]


def sheared_expand_split_case(q, with_planes, row="none", relu=True, shape=FL):
    """The output starts as NaN in every half: a voxel that no depth chunk writes stays one and fails the comparison."""
    from snvc_amd import ops
    n, c, h, w, d = shape
    g, gcol, planes, scale, bias, m0, off, off_col = sheared_inputs(q, with_planes, row, shape)
    (hi, lo, flag), raw = sheared_reference(g, gcol, planes, scale, bias, q, m0, off, off_col, relu, shape)
    outside = (raw[0, 0, :, 0, :w - 1] == 0)
    assert outside[:, 0].any() and outside[:, w - 2].any() and not outside.all()           # i leaves [0, WG) on both sides
    assert not outside.all(axis=1).any(), "every plane has columns inside G"
    stored, eflag = boundary_expectation(row, relu)
    assert flag == eflag and (stored is None or (flag_voxels(hi, lo, shape) == stored).all())
    want = SF.pair_tensor(hi, lo)
    gd, gcd, pd, sd, bd = dev(g), dev(gcol), dev(planes) if planes is not None else None, dev(scale), dev(bias)
    for stream_out in (0, ops.EPI_STREAM_OUT):
        out = torch.full(want.shape, float("nan"), dtype=torch.float16, device=DEV)
        word = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.sheared_expand_split(gd, gcd, pd, sd, bd, out, q, m0, off, off_col, (ops.EPI_RELU if relu else 0) | stream_out, word)
        assert_bits(out, want, f"sheared_expand_split(q={q}, planes={with_planes}, row={row}, stream_out={bool(stream_out)}, shape={shape})")
        assert_ragged_zero(out, c, "sheared_expand_split")
        assert int(word.item()) == int(flag), f"flag {int(word.item())}, the stored values say {int(flag)}"


@pytest.mark.parametrize("with_planes", [True, False], ids=["planes", "no_planes"])
@pytest.mark.parametrize("q", [1, 2])
def test_sheared_expand_split_is_the_definition(q, with_planes):
    """ops.sheared_expand_split called directly: C = 12 (a ragged group), N = 2, D = 17 (two depth chunks: DCH doubles while
    H * G * N * DCH < 512 and D / (2 DCH) >= 8, so DCH = 2 and DC = 9), W = 68; EPI_STREAM_OUT on and off with equal bits."""
    sheared_expand_split_case(q, with_planes)


@pytest.mark.parametrize("row,relu", [(r, True) for r in FL_ROWS if r != "none"] + [("-70000", False)])
def test_sheared_expand_split_flag_rows(row, relu):
    """65472 -> no flag, 65504 -> flag, above -> clamped and flag; with ReLU a value below -65504 -> stored 0 and no flag."""
    sheared_expand_split_case(2, True, row, relu)


WARPED_SHIFTS = np.array([
    [0.0, 1.0, 2.0, 3.0, 0.5, 1.5, 2.5, 2.0 ** 0.5, np.pi, 7.3, 12.25, 30.0, 66.5, 67.0, 68.0, 68.5, 70.0],     # whole, half, irrational, s <= W, s > W
    [5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0, 8.5, 9.0, np.e, 3 ** 0.5, 0.25, 0.0, 0.0, 40.75, 41.0, 1e-3]], np.float32)


def warped_shifts(shape):
    """WARPED_SHIFTS at the shape FL; for a deeper shape the same kinds of rows (whole, half, irrational, zero, at and beyond W) from
    tests/first_layer_cases.warped_shifts, with runs of equal and of half-pixel steps so that the register windows stand and move."""
    if shape == FL:
        return WARPED_SHIFTS
    import first_layer_cases as FC
    n, c, h, w, d = shape
    s = FC.warped_shifts(n, d, w)
    s[0, 4:12] = np.float32(3.0) + np.float32(0.5) * np.arange(8, dtype=np.float32)
    s[-1, d // 2:d // 2 + 4] = np.float32(2.0 ** 0.5)
    return s


def warped_inputs(with_planes, row, shape=FL):
    n, c, h, w, d = shape
    r = np.random.default_rng(90 if shape == FL else 90 + sum(shape))
    p = r.standard_normal((n, 3 * c, h, w)).astype(np.float32)
    q = r.standard_normal((n, 3 * c, h, w)).astype(np.float32)
    e = r.standard_normal((n, 9 * c, h, 4)).astype(np.float32)
    planes = r.standard_normal((n, c, 3, h, w)).astype(np.float32)
    at = flag_at(shape)
    for kd in range(3):                                    # channel 11 of the last sample: nothing but its planes
        p[at[0], kd * c + 11] = 0
        q[at[0], kd * c + 11] = 0
        for kw in range(3):
            e[at[0], (kd * 3 + kw) * c + 11] = 0
    planes[at[0], 11] = (r.integers(-512, 513, (3, h, w)) / 64.0).astype(np.float32)
    if BOUNDARY[row] is not None:
        planes[at[0], at[1], 1, at[2], at[3]] = BOUNDARY[row]
    elif not with_planes:
        planes = None
    scale = r.uniform(0.5, 2.0, c).astype(np.float32) * r.choice([-1.0, 1.0], c).astype(np.float32)
    bias = r.standard_normal(c).astype(np.float32)
    scale[11], bias[11] = 1.0, 0.0
    return p, q, e, planes, scale, bias


def warped_expand_split_case(with_planes, row="none", relu=True, shape=FL):
    """ops.warped_expand_split against ops.warped_expand (float32, held to the C oracle by test_gpu_parity) on the same operands.

    Bound.  Both kernels evaluate, per voxel, t = fma(o, sc, bi) with o = pe + sum over kd of (f F_kd + g G_kd) [- tas at the last column],
    f + g = 1, G = F - E at three columns; they differ in the order of the sum.  Roundings per kernel: the subtraction that forms G, six
    FMAs (or multiply-adds), the add of the two partial sums, the subtraction of tas, the affine: 10, each at most u = 2^-24 times the
    magnitude of a partial result, which M = |sc| (|pe| + 3 (Pmax + Emax) + 3 Qmax) + |bi| bounds (Pmax, Emax, Qmax: the maxima of |p|,
    |e|, |q| over the channel's rows of the sample; |f F + g G| <= Pmax + Emax, |tas| <= 3 Qmax).  tas itself carries 11 more roundings
    (six products, five adds) of terms bounded by 3 |sc| Qmax <= M.  So each kernel is within 21 u M (1 + 21 u) of the exact value, the
    two within 42 u M (1 + 2^-19) of each other: k = 43.  The pair holds its value to 2^-22 |t| + 2^-25 (22 bits; a subnormal lo
    steps by 2^-24).  The clamp is monotone and ReLU is 1-Lipschitz: neither widens the distance.  In all:

        |pair_value - clamp(y32)| <= 2^-22 |y| + 2^-25 + 43 u M.

    Channel 11 of the last sample has p = q = e = 0, scale 1, bias 0 and planes on a grid: its stored pair is clamp_pair(planes), bit for
    bit, which is where the flag rows sit.  The output starts as NaN in every half, and EPI_STREAM_OUT on and off give equal bits."""
    from snvc_amd import ops
    n, c, h, w, d = shape
    p, q, e, planes, scale, bias = warped_inputs(with_planes, row, shape)
    flags = ops.EPI_RELU if relu else 0
    pd_, qd, ed, pld, shd, sd, bd = dev(p), dev(q), dev(e), dev(planes) if planes is not None else None, dev(warped_shifts(shape)), dev(scale), dev(bias)
    y32 = torch.empty((n, c, d, h, w), dtype=torch.float32, device=DEV)
    ops.warped_expand(pd_, qd, ed, pld, shd, sd, bd, y32, flags)
    out = torch.full((n, 2, (c + 7) // 8, d, h, w, 8), float("nan"), dtype=torch.float16, device=DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.warped_expand_split(pd_, qd, ed, pld, shd, sd, bd, out, flags, word)
    streamed = torch.full(out.shape, float("nan"), dtype=torch.float16, device=DEV)
    ops.warped_expand_split(pd_, qd, ed, pld, shd, sd, bd, streamed, flags | ops.EPI_STREAM_OUT, None)
    pair = host(out)
    assert_bits(streamed, pair, "warped_expand_split, EPI_STREAM_OUT")
    assert_ragged_zero(out, c, "warped_expand_split")
    hi, lo = SF.from_c8(pair[:, 0], c), SF.from_c8(pair[:, 1], c)
    assert np.isfinite(hi).all() and np.isfinite(lo).all()
    SF.lo_within_half_ulp(hi, lo)
    y = np.clip(host(y32).astype(np.float64), -65504.0, 65504.0)
    amax = lambda t, k: np.abs(t).reshape(n, k, c, -1).max(axis=(1, 3))                   # noqa: E731  [N, C]
    pl = amax(planes.transpose(0, 2, 1, 3, 4).reshape(n, 3 * c, h, w), 3) if planes is not None else 0.0
    M = np.abs(scale)[None] * (pl + 3 * (amax(p, 3) + amax(e, 9)) + 3 * amax(q, 3)) + np.abs(bias)[None]
    bound = 2.0 ** -22 * np.abs(y) + 2.0 ** -25 + 43 * U * M.reshape(n, c, 1, 1, 1)
    err = np.abs(SF.pair_value(hi, lo, 1.0).astype(np.float64) - y)
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    print(f"warped_expand_split(planes={with_planes}, row={row}, shape={shape}): max |pair - y32| / bound = {float((err / bound).max()):.3f} at {worst}")
    assert (err <= bound).all(), (worst, float(err[worst]), float(bound[worst]))
    # channel 11 of the last sample: exact
    at = flag_at(shape)
    cls = np.array([0] + [1] * (d - 2) + [2])
    src = planes[at[0], 11][cls] if planes is not None else np.zeros((d, h, w), np.float32)
    ehi, elo, _ = SF.clamp_pair(src, relu)
    assert_bits(hi[at[0], 11], ehi, "warped_expand_split, the exact channel (hi)")
    assert_bits(lo[at[0], 11], elo, "warped_expand_split, the exact channel (lo)")
    stored, eflag = boundary_expectation(row, relu)
    if stored is not None:
        assert (flag_voxels(hi, lo, shape) == stored).all()
    assert int(word.item()) == int(eflag), f"flag {int(word.item())}, the stored values say {int(eflag)}"


@pytest.mark.parametrize("with_planes", [True, False], ids=["planes", "no_planes"])
def test_warped_expand_split_vs_the_float32_pass(with_planes):
    """The shapes of the sheared test (D = 17: DCH doubles while H * G * N * DCH < 768 and D / (2 DCH) >= 8: two chunks), shifts
    whole-pixel, half-pixel, irrational, at and beyond W."""
    warped_expand_split_case(with_planes)


@pytest.mark.parametrize("row,relu", [(r, True) for r in FL_ROWS if r != "none"] + [("-70000", False)])
def test_warped_expand_split_flag_rows(row, relu):
    """65472 -> no flag, 65504 -> flag, above -> clamped and flag; with ReLU a value below -65504 -> stored 0 and NO flag: the flag looks
    at what is stored."""
    warped_expand_split_case(True, row, relu)
