"""The split format ("f16x3") on the host, numpy only: the one definition that tests/test_split_format_host.py holds to an integer
restatement of round-to-nearest-even and that tests/test_gpu_split_format.py holds every kernel that writes a split pair to.

A value v travels as two half planes in the C8 layout [N, 2 (hi | lo), ceil(C/8), spatial..., 8]:

    hi = half(v * mul),   lo = half(v * mul - float32(hi)),   every operation in float32, mul a power of two;

the value read back is float32((float32(hi) + float32(lo)) * inv_mul).  float32(hi) + float32(lo) is exact for every pair the
definition produces, and |lo| <= ulp_half(hi) / 2 (``lo_within_half_ulp``).  |v * mul| >= 65520 rounds to hi = +-inf and gives
lo = -+inf: the layout pass does not clamp.  The epilogues that do (``clamp_pair``) store the pair of median(v, lower, 65504)
and raise their flag when a STORED magnitude reaches 65504.

Re-splitting hi + lo does not give the pair back in general (lo is rounded to half, so hi + lo is not v): nothing here asserts it.
"""
import numpy as np

HALF_MAX = np.float32(65504.0)


def split_pair(v: np.ndarray, mul: float):
    """The split format's definition: hi = float16(v * mul), lo = float16(v * mul - float32(hi)), every operation in float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        vm = (v.astype(np.float32) * np.float32(mul)).astype(np.float32)
        hi = vm.astype(np.float16)
        lo = (vm - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi, lo


def pair_value(hi: np.ndarray, lo: np.ndarray, inv_mul: float):
    """float32((float32(hi) + float32(lo)) * inv_mul): what the kernels that read a pair compute."""
    with np.errstate(invalid="ignore", over="ignore"):
        s = (hi.astype(np.float32) + lo.astype(np.float32)).astype(np.float32)
        return (s * np.float32(inv_mul)).astype(np.float32)


def to_c8(x: np.ndarray):
    """[N, C, spatial...] -> the C8 layout [N, ceil(C/8), spatial..., 8] in x's dtype; the missing channels of the last group are +0."""
    n, c = x.shape[:2]
    sp = x.shape[2:]
    g = (c + 7) // 8
    full = np.zeros((n, g * 8) + sp, x.dtype)
    full[:, :c] = x
    return np.ascontiguousarray(np.moveaxis(full.reshape((n, g, 8) + sp), 2, -1))


def from_c8(x8: np.ndarray, channels=None):
    """The C8 layout [N, G, spatial..., 8] -> [N, channels, spatial...] (all 8 G channels by default)."""
    n, g = x8.shape[:2]
    sp = x8.shape[2:-1]
    full = np.moveaxis(x8, -1, 2).reshape((n, g * 8) + sp)
    return np.ascontiguousarray(full[:, :g * 8 if channels is None else channels])


def pair_tensor(hi: np.ndarray, lo: np.ndarray):
    """Two [N, C, spatial...] half arrays -> the pair tensor [N, 2, ceil(C/8), spatial..., 8]."""
    return np.ascontiguousarray(np.stack([to_c8(hi), to_c8(lo)], axis=1))


def clamp_pair(v: np.ndarray, relu: bool):
    """(hi, lo, flag) of a clamping split epilogue on float32 values: c = median(v, 0 if relu else -65504, 65504), the pair is
    split_pair(c, 1), and the flag looks at what is stored: any |c| >= 65504.  Finite or infinite v; NaN is out of scope."""
    v = v.astype(np.float32)
    assert not np.isnan(v).any()
    c = np.minimum(np.maximum(v, np.float32(0.0) if relu else -HALF_MAX), HALF_MAX).astype(np.float32)
    if relu:
        c = np.where(c > 0, c, np.float32(0.0)).astype(np.float32)     # -0 leaves a median with bound +0 as +0
    hi, lo = split_pair(c, 1.0)
    return hi, lo, bool((np.abs(c) >= HALF_MAX).any())


def ulp_half(hi: np.ndarray):
    """The spacing of halves at |hi| as float64: 2^(e - 10) in the binade [2^e, 2^(e+1)), 2^-24 below the smallest normal."""
    a = np.abs(hi.astype(np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return np.exp2(e - 10)


def lo_within_half_ulp(hi: np.ndarray, lo: np.ndarray):
    """Asserts |lo| <= ulp_half(hi) / 2 wherever hi is finite: lo holds what hi's rounding left, never more than half a step."""
    fin = np.isfinite(hi)
    bad = fin & ~(np.abs(lo.astype(np.float64)) <= ulp_half(np.where(fin, hi, np.float16(0))) / 2)
    assert not bad.any(), (f"{int(bad.sum())} pairs with |lo| above half a step of hi, the first (hi, lo) = "
                           f"({hi[bad].ravel()[0]!r}, {lo[bad].ravel()[0]!r})")


def _edges():
    f = np.float32
    below_65520 = np.nextafter(f(65520.0), f(0.0))
    vals = [
        0.0, -0.0,
        # ties between neighbouring halves, of both parities: 2049 -> 2048, 2051 -> 2052; 1 + 2^-11 -> 1, 1 + 3 * 2^-11 -> 1 + 2^-9
        2049.0, 2051.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11,
        # lo is a half subnormal: 3 * 2^-24 behind 2^-10; 2^-24 behind 2^-12; rounded ones (2^-25 + 2^-30 -> 2^-24, 5 * 2^-25 -> 2^-23)
        2.0 ** -10 + 3 * 2.0 ** -24, 2.0 ** -12 + 2.0 ** -24, 2.0 ** -12 + 2.0 ** -25 + 2.0 ** -30, 2.0 ** -11 + 5 * 2.0 ** -25, 0.001,
        # lo underflows to 0: what is left is below (or a tie at) half the smallest subnormal
        2.0 ** -10 + 2.0 ** -26, 1.0 + 2.0 ** -26, 2.0 ** -12 + 2.0 ** -25, 2.0 ** -14 + 2.0 ** -25 + 2.0 ** -30,
        # the bottom of the range: 2^-25 is a tie between 0 and 2^-24 (-> 0), 1.5 * 2^-24 one between 2^-24 and 2^-23 (-> 2^-23, and
        # lo = -2^-25 is a tie again -> -0); the smallest normal, the smallest and the largest subnormal
        2.0 ** -25, 1.5 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24,
        # the top: the last two halves, the largest float32 that still rounds to 65504, and the tie that rounds to inf
        65472.0, 65504.0, float(below_65520), 65520.0,
    ]
    return np.array(vals, dtype=np.float32)


EDGES = _edges()


def edge_data(shape, seed: int, lo_exp: float = -26.0, hi_exp: float = 15.99):
    """float32 data of ``shape``: EDGES with both signs tiled from the front of the flattened array and at its very end (the last
    element of the last partial block), the rest log-uniform magnitudes over [2^lo_exp, 2^hi_exp] with random signs."""
    r = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = (np.exp2(r.uniform(lo_exp, hi_exp, n)) * r.choice([-1.0, 1.0], n)).astype(np.float32)
    e = np.concatenate([EDGES, -EDGES])
    k = min(n, 3 * e.size)
    x[:k] = np.resize(e, k)
    if n > e.size:
        x[n - e.size:] = e[::-1]
    return x.reshape(shape)
