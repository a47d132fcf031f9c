"""Case tables and float64 references for snvc_conv3d_wgrad (csrc/conv3d_bwd.hip).  No GPU import: tests/test_wgrad_ref_host.py pins
the references to the kernel's own definition on the CPU, tests/test_gpu_wgrad_forms.py runs the cases on the device.

A case is (N, Cin, Cout, (D, H, W) of x, ksize, stride, dilation); pad = dilation * (ksize - 1) / 2 throughout (the only padding the
entry point accepts).  A role-swapped case is (N, Cin_d, Cout_d, (D, H, W) of the transposed layer's INPUT): the layer is
ConvTranspose3d(Cin_d, Cout_d, 3, stride 2, padding 1, output_padding 1), its output gradient lives on the doubled grid.

What each shape is for, from the dispatcher (snvc_conv3d_wgrad_amax) and the kernels' tile sizes:
  generic tap-chunk kernel (keys 511 / 512 / 711): tiles of TH = 2 rows x 32 columns, channel blocks of 32, tap chunks of KHG kernel
      rows -- k7 has KHG = 4: its second chunk holds 3 rows (21 live taps in 28 slots)
  split-operand forms (311 / 321 default): columns of 4 (stride 2: 2) rows x 32 columns walked along d, cut into depth parts when
      there are fewer jobs than 3/4 of the CUs and the parts stay >= 8 planes (`dparts`, restated in `expected_dparts`)
  12-wave forms (311 Winograd-domain under WGRAD_FP32, 321 when the big grid is not exactly twice the small one): 8 * (CUs / 8 / 3)
      units for the channel pairs (`wgrad_unit_count`)
  k1 streaming form: Cout <= 2, D*H*W % 4 == 0, chunks of 65536 voxels, four input channels per workgroup
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------------------------ case tables
K57_CASES = {
    "k5 16-byte rows": (2, 32, 32, (5, 6, 36), 5, 1, 1),                 # two tiles along W, the second 4 columns wide
    "k5 8-byte rows, partial blocks": (1, 40, 24, (3, 5, 38), 5, 1, 1),  # W % 4 == 2, odd H against TH = 2, channel blocks of 8 and 24
    "k5 odd width": (1, 8, 32, (4, 3, 33), 5, 1, 1),                     # the second W tile holds one column
    # dilation 2: D = 5, 3, 4 is below the effective extent 9, most taps see only padding along D
    "k5d2 16-byte rows": (2, 32, 32, (5, 6, 36), 5, 1, 2),
    "k5d2 8-byte rows, partial blocks": (1, 40, 24, (3, 5, 38), 5, 1, 2),
    "k5d2 odd width": (1, 8, 32, (4, 3, 33), 5, 1, 2),
    "k7 16-byte rows": (1, 64, 32, (4, 6, 36), 7, 1, 1),
    "k7 8-byte rows, partial blocks": (2, 24, 40, (2, 7, 38), 7, 1, 1),
    "k7 odd width": (1, 32, 32, (3, 5, 35), 7, 1, 1),
}
# the same 16-byte-row shapes once more with SNVC_ALGO_SCALAR_STAGING
SCALAR_STAGING_CASES = ["k5 16-byte rows", "k5d2 16-byte rows", "k7 16-byte rows"]

ROLE_SWAP_CASES = {
    "64->32 rows of 40": (2, 64, 32, (3, 4, 20)),      # output rows 40 wide: the split-operand stride-2 form
    "64->64 rows of 38": (1, 64, 64, (2, 3, 19)),      # 8-byte pieces
    "40->24 rows of 18": (2, 40, 24, (2, 5, 9)),       # partial channel blocks
    "8->5 one voxel": (2, 8, 5, (1, 1, 1)),
}

DEPTH1_CASES = {
    "k3 d1": (2, 32, 64, (1, 12, 40), 3, 1, 1),
    "k3 d1 small": (1, 9, 32, (1, 6, 4), 3, 1, 1),
    "k3s2 d1": (1, 32, 32, (1, 12, 40), 3, 2, 1),      # Din = 1 != 2 * Dout = 2: leaves the split-operand stride-2 form
    "k3s2 d1 odd channels": (2, 64, 27, (1, 14, 34), 3, 2, 1),
    "k1 d1": (1, 256, 64, (1, 16, 24), 1, 1, 1),
}

DPART_CASES = {
    # name: (case, parts expected on a 256-CU device, planes of the last part)
    "k3 D17": ((1, 32, 32, (17, 4, 32), 3, 1, 1), 2, 8),
    "k3 D35": ((1, 32, 32, (35, 4, 32), 3, 1, 1), 4, 8),
    "k3 D33": ((1, 32, 32, (33, 4, 32), 3, 1, 1), 4, 6),
    "k3s2 Dout17": ((1, 32, 64, (34, 4, 64), 3, 2, 1), 2, 8),
    "k3s2 Dout33": ((1, 32, 64, (66, 4, 64), 3, 2, 1), 4, 6),
}

PAIRS_CASES = {
    "k3 99 pairs": (1, 352, 288, (2, 4, 32), 3, 1, 1),
    "k3s2 99 pairs": (1, 352, 288, (4, 8, 64), 3, 2, 1),
}

# Batch-strided operands: x and g are channels [lo, lo + C) of buffers 3 channels wider, N = 2.  "aligned": D*H*W % 4 == 0 on both
# grids, so the slices start on 16 bytes and the batch strides are multiples of 4 -- the vector forms run with x_bs != Cin * D*H*W.
# "unaligned": an odd D*H*W on at least one grid and lo = 1: that slice starts 4 bytes off and every alignment predicate must
# send the call to scalar staging.  name: (kind, case, lo)
STRIDED_CASES = {
    "k3 aligned": ("conv", (2, 32, 64, (1, 12, 40), 3, 1, 1), 1),
    "k3 unaligned": ("conv", (2, 9, 32, (1, 7, 5), 3, 1, 1), 1),
    "k3s2 aligned": ("conv", (2, 32, 32, (1, 12, 40), 3, 2, 1), 2),
    "k3s2 unaligned": ("conv", (2, 32, 32, (1, 5, 7), 3, 2, 1), 1),
    "k5 aligned": ("conv", (2, 32, 32, (5, 6, 36), 5, 1, 1), 1),
    "k5 unaligned": ("conv", (2, 8, 32, (3, 3, 33), 5, 1, 1), 1),
    "role swap aligned": ("swap", (2, 64, 32, (3, 4, 20)), 1),
    "role swap unaligned": ("swap", (2, 40, 24, (1, 5, 9)), 1),
}
STRIDED_EXTRA_CHANNELS = 3
STRIDED_FILL = 1.0e3          # what the channels outside the slice hold: a wrong stride or offset shows

K1_STREAM_CASES = {
    # name: (case, takes the streaming form, chunks of 16384 float4)
    "k1 to two channels": ((3, 32, 2, (4, 6, 40), 1, 1, 1), True, 1),
    "k1 two chunks": ((1, 8, 2, (8, 96, 96), 1, 1, 1), True, 2),
    "k1 idle channels": ((1, 6, 1, (4, 6, 40), 1, 1, 1), True, 1),          # Cin % 4 != 0: the last workgroup's spare channels
    "k1 voxels not in fours": ((1, 32, 1, (3, 5, 7), 1, 1, 1), False, 1),    # falls through to key 111
}

UNSUPPORTED_CASES = {
    "k5 stride 2": (1, 8, 8, (4, 6, 8), 5, 2, 1),
    "k3 dilation 2": (1, 8, 8, (4, 6, 8), 3, 1, 2),
}

SEED_BASE = {"k57": 1100, "swap": 1200, "depth1": 1300, "dparts": 1400, "pairs": 1500, "strided": 1600, "k1": 1700, "host": 1800}


def seed_of(group, table, name):
    """The seed of a case: the group's base plus the case's index in the sorted table."""
    return SEED_BASE[group] + sorted(table).index(name)


# ------------------------------------------------------------------------------------------------------------------ geometry
def out_extent(n, k, stride, dil):
    pad = dil * (k - 1) // 2
    return (n + 2 * pad - (dil * (k - 1) + 1)) // stride + 1


def out_shape(shp, k, stride, dil):
    return tuple(out_extent(n, k, stride, dil) for n in shp)


def ceil_div(a, b):
    return -(-a // b)


def channel_pairs(cin, cout):
    return ceil_div(cout, 32) * ceil_div(cin, 32)


def wgrad_unit_count(cus):
    """wgrad_units: 8 XCDs x (CUs / 8 / 3) units of three workgroups; more channel pairs than this and the units take several rounds."""
    return 8 * max(1, cus // 8 // 3)


def expected_dparts(case, cus):
    """(parts, planes per part, planes of the last part) of the split-operand forms: the dispatcher's own loop."""
    n, cin, cout, shp, k, stride, dil = case
    assert k == 3 and dil == 1 and stride in (1, 2)
    do, ho, wo = out_shape(shp, k, stride, dil)
    th, limit = (4, 256) if stride == 1 else (2, 512)
    cols = n * ceil_div(ho, th) * ceil_div(wo, 32)
    pairs = channel_pairs(cin, cout) if stride == 1 else ceil_div(cout, 64) * ceil_div(cin, 32)
    dparts = 1
    while cols * dparts * pairs < cus * 3 // 4 and do // (dparts * 2) >= 8 and cols * dparts * 2 <= limit:
        dparts *= 2
    dchunk = ceil_div(do, dparts)
    dparts = ceil_div(do, dchunk)
    return dparts, dchunk, do - (dparts - 1) * dchunk


# ------------------------------------------------------------------------------------------------------------------ inputs
def _f32(r, shape):
    return torch.from_numpy(r.standard_normal(shape).astype(np.float32))


def conv_inputs(case, seed):
    """(x on the big grid, g on the small grid), standard normal float32."""
    n, cin, cout, shp, k, stride, dil = case
    r = np.random.default_rng(seed)
    x = _f32(r, (n, cin) + tuple(shp))
    g = _f32(r, (n, cout) + out_shape(shp, k, stride, dil))
    return x, g


def swap_inputs(case, seed):
    """(gy_big = gradient of the transposed layer's output, x_small = its input)."""
    n, cin_d, cout_d, shp = case
    r = np.random.default_rng(seed)
    x_small = _f32(r, (n, cin_d) + tuple(shp))
    gy_big = _f32(r, (n, cout_d) + tuple(2 * e for e in shp))
    return gy_big, x_small


# ------------------------------------------------------------------------------------------------------------------ references
def wgrad_ref64(x, g, k, stride, dil):
    """float64 weight gradient of F.conv3d(x, w, stride, pad = dil * (k - 1) / 2, dil) for the output gradient g: [Cout, Cin, k, k, k]."""
    w = torch.zeros(g.shape[1], x.shape[1], k, k, k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, stride=stride, padding=dil * (k - 1) // 2, dilation=dil)
    assert y.shape == g.shape, (tuple(y.shape), tuple(g.shape))
    (y * g.double()).sum().backward()
    return w.grad.numpy()


def wgrad_ref64_transposed(gy_big, x_small):
    """float64 weight gradient of F.conv_transpose3d(x_small, w, None, 2, 1, 1) for the output gradient gy_big:
    nn.ConvTranspose3d's layout [Cin_d, Cout_d, 3, 3, 3]."""
    w = torch.zeros(x_small.shape[1], gy_big.shape[1], 3, 3, 3, dtype=torch.float64, requires_grad=True)
    y = F.conv_transpose3d(x_small.double(), w, None, 2, 1, 1)
    assert y.shape == gy_big.shape, (tuple(y.shape), tuple(gy_big.shape))
    (y * gy_big.double()).sum().backward()
    return w.grad.numpy()


_TABLES = {"k57": K57_CASES, "depth1": DEPTH1_CASES, "pairs": PAIRS_CASES,
           "dparts": {k: v[0] for k, v in DPART_CASES.items()}, "k1": {k: v[0] for k, v in K1_STREAM_CASES.items()}}


@functools.lru_cache(maxsize=None)
def conv_case(group, name):
    """(x, g, float64 reference) of a plain case, computed once per process and shared by its variants; treat as read-only."""
    case = _TABLES[group][name]
    x, g = conv_inputs(case, seed_of(group, _TABLES[group], name))
    return x, g, wgrad_ref64(x, g, case[4], case[5], case[6])


@functools.lru_cache(maxsize=None)
def swap_case(name):
    gy_big, x_small = swap_inputs(ROLE_SWAP_CASES[name], seed_of("swap", ROLE_SWAP_CASES, name))
    return gy_big, x_small, wgrad_ref64_transposed(gy_big, x_small)


@functools.lru_cache(maxsize=None)
def strided_case(name):
    """(x_big, g_small, float64 reference, call arguments (k, stride, pad, dil), lo) of a batch-strided case, dense on the CPU."""
    kind, case, lo = STRIDED_CASES[name]
    seed = seed_of("strided", STRIDED_CASES, name)
    if kind == "swap":
        gy_big, x_small = swap_inputs(case, seed)
        return gy_big, x_small, wgrad_ref64_transposed(gy_big, x_small), (3, 2, 1, 1), lo
    x, g = conv_inputs(case, seed)
    k, stride, dil = case[4:]
    return x, g, wgrad_ref64(x, g, k, stride, dil), (k, stride, dil * (k - 1) // 2, dil), lo
