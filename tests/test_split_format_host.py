"""tests/split_format.py held to an independent restatement (no GPU): float32 -> half by round-to-nearest-even on integer bit
patterns, no ``astype(float16)`` anywhere in the restatement; the clamp-and-flag rule at its boundary; |lo| <= ulp_half(hi) / 2 and
the exactness of float32(hi) + float32(lo) over every finite half, its float32 neighbours and the ties between halves."""
import numpy as np
import pytest

import split_format as SF

MULS = [1.0, 8.0, 0.25]


def half_bits_rne(bits32: np.ndarray) -> np.ndarray:
    """The half bit pattern nearest to each float32 bit pattern, ties to even, in integer arithmetic.  A float32 normal is
    M * 2^(E - 23) with M in [2^23, 2^24); a half keeps M >> 13 of it in its normal range (E >= -14) and M >> (13 + (-14 - E)) below;
    what is shifted out decides the rounding, and a carry out of the mantissa runs into the exponent field, up to 0x7c00 = inf."""
    b = bits32.astype(np.int64)
    sign = (b >> 16) & 0x8000
    e = (b >> 23) & 0xFF
    m = b & 0x7FFFFF
    E = e - 127
    M = m | 0x800000
    shift = np.where(E >= -14, 13, np.minimum(13 + (-14 - E), 31))
    q = M >> shift
    rem = M & ((np.int64(1) << shift) - 1)
    half = np.int64(1) << (shift - 1)
    up = ((rem > half) | ((rem == half) & ((q & 1) == 1))).astype(np.int64)
    normal = ((E + 14) << 10) + q + up               # q carries the implicit one: (E + 15) << 10 with the fraction q - 0x400
    sub = q + up                                     # a carry to 0x400 is the smallest normal
    out = np.where(E >= -14, normal, sub)
    out = np.where(E > 15, 0x7C00, np.minimum(out, 0x7C00))
    out = np.where(e == 0, 0, out)                   # float32 zero and subnormals: far below 2^-25
    out = np.where(e == 255, np.where(m == 0, 0x7C00, 0x7E00), out)
    return (sign | out).astype(np.uint16)


def half_value64(bits16: np.ndarray) -> np.ndarray:
    """The value of a half bit pattern as float64, from its fields."""
    b = bits16.astype(np.int64)
    s = np.where(b & 0x8000, -1.0, 1.0)
    e = (b >> 10) & 0x1F
    m = (b & 0x3FF).astype(np.float64)
    with np.errstate(invalid="ignore"):
        v = np.where(e == 0, m * 2.0 ** -24, (1024.0 + m) * np.exp2((e - 25).astype(np.float64)))
        v = np.where(e == 31, np.where(m == 0, np.inf, np.nan), v)
    return s * v


def restated_pair(v32: np.ndarray, mul: float):
    """split_pair by the restatement: v * mul is the float32 nearest the exact (float64) product -- the product itself except for
    the float32 subnormals next to 0 under mul < 1 -- and v * mul - hi is exact in float64 and fits a float32 (asserted); both halves
    rounded on bit patterns."""
    vm = (v32.astype(np.float64) * mul).astype(np.float32)
    vm64 = vm.astype(np.float64)
    hi_bits = half_bits_rne(vm.view(np.uint32))
    with np.errstate(invalid="ignore"):
        d64 = vm64 - half_value64(hi_bits)
    d = d64.astype(np.float32)
    assert np.array_equal(d.astype(np.float64), d64)                     # what hi's rounding left fits a float32
    return hi_bits, half_bits_rne(d.view(np.uint32))


@pytest.fixture(scope="module")
def every_half():
    """Every finite half h >= 0 as float32, its two float32 neighbours, and the midpoint to the next half (65520 behind 65504)
    -- and the negatives of all of them."""
    h = np.arange(0x7C00, dtype=np.uint16).view(np.float16).astype(np.float32)
    nxt = np.append(h[1:], np.float32(65536.0))
    mid = ((h.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (h.astype(np.float64) + nxt) / 2)
    pos = np.concatenate([h, np.nextafter(h, np.float32(np.inf)), np.nextafter(h, np.float32(-np.inf)), mid, SF.EDGES])
    return np.concatenate([pos, -pos]).astype(np.float32)


def test_the_restatement_knows_the_ties():
    f = lambda *v: half_bits_rne(np.array(v, np.float32).view(np.uint32)).view(np.float16).astype(np.float64).tolist()      # noqa: E731
    assert f(2049.0, 2051.0, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11) == [2048.0, 2052.0, 1.0, 1 + 2.0 ** -9]
    assert f(2.0 ** -25, 1.5 * 2.0 ** -24, np.nextafter(np.float32(2.0 ** -25), np.float32(1))) == [0.0, 2.0 ** -23, 2.0 ** -24]
    assert f(65519.996, 65520.0, -65520.0, 1e-40, np.inf) == [65504.0, np.inf, -np.inf, 0.0, np.inf]
    assert half_bits_rne(np.array([-0.0, np.nan], np.float32).view(np.uint32)).tolist() == [0x8000, 0x7E00]
    allh = np.arange(0x10000, dtype=np.uint16)
    fin = ~np.isnan(allh.view(np.float16))
    assert np.array_equal(half_value64(allh)[fin], allh.view(np.float16).astype(np.float64)[fin])
    assert np.array_equal(half_bits_rne(allh.view(np.float16).astype(np.float32).view(np.uint32))[fin], allh[fin])


@pytest.mark.parametrize("mul", MULS)
def test_split_pair_equals_the_integer_restatement_bit_for_bit(every_half, mul):
    hi, lo = SF.split_pair(every_half, mul)
    rhi, rlo = restated_pair(every_half, mul)
    assert not np.isnan(hi).any() and not np.isnan(lo).any()
    assert np.array_equal(hi.view(np.uint16), rhi)
    assert np.array_equal(lo.view(np.uint16), rlo)


@pytest.mark.parametrize("mul", MULS)
def test_lo_is_within_half_a_step_and_the_float32_sum_is_exact(every_half, mul):
    hi, lo = SF.split_pair(every_half, mul)
    SF.lo_within_half_ulp(hi, lo)
    fin = np.isfinite(hi)
    s64 = hi.astype(np.float64)[fin] + lo.astype(np.float64)[fin]
    s32 = SF.pair_value(hi, lo, 1.0)[fin]
    assert np.array_equal(s32.astype(np.float64), s64)
    # and the pair holds v * mul to 2^-22 relative, or to half a subnormal step
    vm = every_half.astype(np.float64)[fin] * mul
    assert (np.abs(s64 - vm) <= np.maximum(2.0 ** -22 * np.abs(vm), 2.0 ** -25)).all()
    r = np.random.default_rng(3)
    v = (np.exp2(r.uniform(-27, 16, 1 << 18)) * r.choice([-1.0, 1.0], 1 << 18)).astype(np.float32)
    hi, lo = SF.split_pair(v, 1.0)
    SF.lo_within_half_ulp(hi, lo)
    with pytest.raises(AssertionError):
        SF.lo_within_half_ulp(np.array([1.0], np.float16), np.array([2.0 ** -10], np.float16))


def test_overflow_gives_opposite_infinities_and_the_value_read_back():
    hi, lo = SF.split_pair(np.array([65520.0, -1e6, np.inf], np.float32), 1.0)
    assert hi.tolist() == [np.inf, -np.inf, np.inf] and lo.tolist()[:2] == [-np.inf, np.inf] and np.isnan(lo[2])
    hi, lo = SF.split_pair(np.array([3.0, 1 + 2.0 ** -12], np.float32), 8.0)
    assert SF.pair_value(hi, lo, 0.125).tolist() == [3.0, 1 + 2.0 ** -12]


@pytest.mark.parametrize("relu", [False, True])
def test_clamp_pair_at_the_boundary(relu):
    f = np.float32
    above = np.nextafter(f(65504.0), f(np.inf))
    rows = [  # value, stored hi, stored lo, flag
        (65472.0, 65472.0, 0.0, False), (65504.0, 65504.0, 0.0, True), (above, 65504.0, 0.0, True), (np.inf, 65504.0, 0.0, True),
        (65503.0, 65504.0, -1.0, False),                                   # hi rounds up to 65504, the stored VALUE is below: no flag
        (-70000.0, 0.0 if relu else -65504.0, 0.0, not relu), (-np.inf, 0.0 if relu else -65504.0, 0.0, not relu),
        (-3.0, 0.0 if relu else -3.0, 0.0, False),
    ]
    for v, ehi, elo, eflag in rows:
        hi, lo, flag = SF.clamp_pair(np.array([1.0, v, -0.5], f), relu)
        assert (float(hi[1]), float(lo[1]), flag) == (ehi, elo, eflag), (v, hi, lo, flag)
        assert not np.signbit(hi[1]) or not relu
    hi, lo, flag = SF.clamp_pair(np.array([70000.0], f), relu)
    assert lo[0] == 0 and hi[0] == 65504                                  # lo of the CLAMPED value, not 70000 - 65504 = 4496


@pytest.mark.parametrize("c", [5, 8, 20])
def test_c8_layout_round_trip_and_zero_lanes(c):
    x = np.arange(2 * c * 6, dtype=np.float32).reshape(2, c, 1, 2, 3) + 1
    x8 = SF.to_c8(x)
    g = (c + 7) // 8
    assert x8.shape == (2, g, 1, 2, 3, 8)
    assert x8[1, c // 8 if c % 8 else 0, 0, 1, 2, 0] == x[1, 8 * (c // 8) if c % 8 else 0, 0, 1, 2]
    assert np.array_equal(SF.from_c8(x8, c), x)
    if c % 8:
        pad = x8[:, -1, ..., c % 8:]
        assert not pad.any() and not np.signbit(pad).any()
    hi, lo = SF.split_pair(x, 1.0)
    p = SF.pair_tensor(hi, lo)
    assert p.shape == (2, 2, g, 1, 2, 3, 8) and np.array_equal(SF.from_c8(p[:, 0], c), hi)


def test_edges_hold_what_they_are_named_for():
    hi, lo = SF.split_pair(SF.EDGES, 1.0)
    lo64 = np.abs(lo.astype(np.float64))
    assert ((lo64 > 0) & (lo64 < 2.0 ** -14)).sum() >= 4                   # subnormal lo
    assert np.isinf(hi).sum() == 1 and SF.EDGES[np.isinf(hi)][0] == 65520.0
    assert np.signbit(SF.EDGES).sum() == 1
    d = SF.edge_data((2, 5, 2, 3, 67), 1)
    assert d.dtype == np.float32 and np.isfinite(d).all() and (np.abs(d[np.abs(d) > 0]) >= 2.0 ** -26).all()
    assert d.reshape(-1)[-1] == 0.0 and d.reshape(-1)[-SF.EDGES.size] == 65520.0
