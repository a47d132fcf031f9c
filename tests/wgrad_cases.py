"""Case tables and float64 references for snvc_conv3d_wgrad (csrc/conv3d_bwd.hip).  No GPU import: tests/test_wgrad_ref_host.py pins
the references to the kernel's own definition on the CPU, tests/test_gpu_wgrad_forms.py runs the cases on the device.

A case is (N, Cin, Cout, (D, H, W) of x, ksize, stride, dilation); pad = dilation * (ksize - 1) / 2 throughout (the only padding the
entry point accepts).  A role-swapped case is (N, Cin_d, Cout_d, (D, H, W) of the transposed layer's INPUT): the layer is
ConvTranspose3d(Cin_d, Cout_d, 3, stride 2, padding 1, output_padding 1), its output gradient lives on the doubled grid.

What each shape is for: the form column below (`FORMS`) says which kernel form a case takes under each variant and alignment, and
tests/test_wgrad_plan_host.py holds that column to the library's own plan (snvc_conv3d_wgrad_form, include/snvc_forms.h, which
lists the forms and their conditions).  The tile sizes behind the shapes:
  generic forms (TAPS; KSPLIT for 311 / 321 on vector rows): tiles of TH = 2 (stride 2: 1) rows x 32 columns, channel blocks of 32,
      tap chunks of KHG kernel rows -- k7 has KHG = 4: its second chunk holds 3 rows (21 live taps in 28 slots)
  split-operand forms (X3 / X3S2): columns of 4 (stride 2: 2) rows x 32 columns walked along d, cut into depth parts when there are
      fewer jobs than 3/4 of the CUs and the parts stay >= 8 planes (`dparts`, restated in `expected_dparts`)
  12-wave forms (WINO / S2): 8 * (CUs / 8 / 3) units for the channel pairs (`wgrad_unit_count`)
  k1 streaming form (K1_STREAM): chunks of 65536 voxels, four input channels per workgroup
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

# The two places where a 3x3x3 layer leaves its split-operand form for the 12-wave one because its columns (N * ceil(H / 4) *
# ceil(W / 32), stride 2: N * ceil(Ho / 2) * ceil(Wo / 32)) would need more partial slabs than the workspace holds: 256 / 512 columns
COLUMN_LIMIT_CASES = {
    "k3 257 columns": (1, 32, 32, (1, 1028, 32), 3, 1, 1),
    "k3s2 513 columns": (1, 32, 32, (2, 2052, 64), 3, 2, 1),
}

# Rows of 8 bytes: W % 4 == 2 on both grids (X3's float2 pieces), and a gradient grid with Wo % 4 == 2 under 16-byte input rows
# (vec == 2: X3S2 / S2 / KSPLIT with float2 pieces of g)
ROWS8_CASES = {
    "k3 8-byte rows": (1, 32, 32, (2, 4, 38), 3, 1, 1),
    "k3s2 8-byte gradient rows": (1, 32, 32, (4, 4, 36), 3, 2, 1),
}

UNSUPPORTED_CASES = {
    "k5 stride 2": (1, 8, 8, (4, 6, 8), 5, 2, 1),
    "k3 dilation 2": (1, 8, 8, (4, 6, 8), 3, 1, 2),
}

SEED_BASE = {"k57": 1100, "swap": 1200, "depth1": 1300, "dparts": 1400, "pairs": 1500, "strided": 1600, "k1": 1700, "host": 1800,
             "columns": 2000, "rows8": 2100}


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
           "dparts": {k: v[0] for k, v in DPART_CASES.items()}, "k1": {k: v[0] for k, v in K1_STREAM_CASES.items()},
           "columns": COLUMN_LIMIT_CASES, "rows8": ROWS8_CASES}


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


# ------------------------------------------------------------------------------------------------------------------ form column
# Which form of include/snvc_forms.h (enum snvc_conv3d_wgrad_form_id) every case takes, written down from the dispatcher's
# conditions case by case -- not generated from the library.  Three alignment classes decide: "full" = x and g both on 16 bytes;
# "g8" = x on 16 bytes, g on 8 only; everything else ("rest": x off 16 bytes, or g on 4 only) stages scalars.
VARIANTS = ("auto", "fp32", "direct")
ALIGNMENTS = (16, 8, 4)


def _forms(auto, fp32, direct, g8="KSPLIT", rest="TAPS"):
    """{variant: (full, g8, rest)}; off full alignment no variant matters: vector rows of g in pieces of 2 (KSPLIT) or scalars."""
    return {"auto": (auto, g8, rest), "fp32": (fp32, g8, rest), "direct": (direct, g8, rest)}


_TAPS = _forms("TAPS", "TAPS", "TAPS", g8="TAPS")                 # the key has no other form, or a row is not in whole pieces
_K3 = _forms("X3", "WINO", "KSPLIT")                              # 3x3x3 stride 1 on 16-byte rows
_K3S2 = _forms("X3S2", "S2", "KSPLIT")                            # 3x3x3 stride 2, the big grid exactly twice the small one
_K3S2_ODD = _forms("S2", "S2", "KSPLIT")                          # ... and not exactly twice
_K1 = _forms("K1_STREAM", "K1_STREAM", "K1_STREAM", g8="TAPS")    # the streaming form does not look at the variant

FORMS = {
    **{("k57", n): _TAPS for n in K57_CASES},
    ("swap", "64->32 rows of 40"): _K3S2,
    ("swap", "64->64 rows of 38"): _TAPS,              # the big grid's rows are 38 wide: no vector staging of x
    ("swap", "40->24 rows of 18"): _TAPS,
    ("swap", "8->5 one voxel"): _TAPS,
    ("depth1", "k3 d1"): _K3,
    ("depth1", "k3 d1 small"): _K3,
    ("depth1", "k3s2 d1"): _K3S2_ODD,
    ("depth1", "k3s2 d1 odd channels"): _TAPS,         # rows of 34
    ("depth1", "k1 d1"): _TAPS,                        # 64 output channels
    **{("dparts", n): (_K3 if c[0][5] == 1 else _K3S2) for n, c in DPART_CASES.items()},
    ("pairs", "k3 99 pairs"): _K3,
    ("pairs", "k3s2 99 pairs"): _K3S2,
    ("strided", "k3 aligned"): _K3,
    ("strided", "k3 unaligned"): _TAPS,                # rows of 5
    ("strided", "k3s2 aligned"): _K3S2_ODD,
    ("strided", "k3s2 unaligned"): _TAPS,
    ("strided", "k5 aligned"): _TAPS,
    ("strided", "k5 unaligned"): _TAPS,
    ("strided", "role swap aligned"): _K3S2,
    ("strided", "role swap unaligned"): _TAPS,         # rows of 18
    ("k1", "k1 to two channels"): _K1,
    ("k1", "k1 two chunks"): _K1,
    ("k1", "k1 idle channels"): _K1,
    ("k1", "k1 voxels not in fours"): _TAPS,
    ("columns", "k3 257 columns"): _forms("WINO", "WINO", "KSPLIT"),           # 257 columns: one too many for X3's slabs
    ("columns", "k3s2 513 columns"): _forms("S2", "S2", "KSPLIT"),             # 513: one too many for X3S2's
    ("rows8", "k3 8-byte rows"): _forms("X3", "TAPS", "TAPS", g8="TAPS"),       # X3 alone reads rows in float2 pieces of x
    ("rows8", "k3s2 8-byte gradient rows"): _K3S2,
}

# (slot 2, slot 3) of the query's info at 256 CUs and full alignment, for the forms that have such numbers: (dparts, dchunk) of the
# split-operand forms, (P, upx) of the 12-wave forms, (chunks, 0) of the k1 streaming form.  {(group, name): {variant: numbers}}
_P80, _P40, _P1 = (80, 10), (40, 10), (1, 13)          # 1, 2 and 99 channel pairs over the 80 units of 256 CUs
PLAN_256 = {
    ("swap", "64->32 rows of 40"): {"auto": (1, 3), "fp32": _P40},
    ("depth1", "k3 d1"): {"auto": (1, 1), "fp32": _P40},
    ("depth1", "k3 d1 small"): {"auto": (1, 1), "fp32": _P80},
    ("depth1", "k3s2 d1"): {"auto": _P80, "fp32": _P80},
    ("dparts", "k3 D17"): {"auto": (2, 9), "fp32": _P80},
    ("dparts", "k3 D35"): {"auto": (4, 9), "fp32": _P80},
    ("dparts", "k3 D33"): {"auto": (4, 9), "fp32": _P80},
    ("dparts", "k3s2 Dout17"): {"auto": (2, 9), "fp32": _P40},
    ("dparts", "k3s2 Dout33"): {"auto": (4, 9), "fp32": _P40},
    ("pairs", "k3 99 pairs"): {"auto": (1, 2), "fp32": _P1},
    ("pairs", "k3s2 99 pairs"): {"auto": (1, 2), "fp32": _P1},
    ("strided", "k3 aligned"): {"auto": (1, 1), "fp32": _P40},
    ("strided", "k3s2 aligned"): {"auto": _P80, "fp32": _P80},
    ("strided", "role swap aligned"): {"auto": (1, 3), "fp32": _P40},
    ("k1", "k1 to two channels"): {v: (1, 0) for v in VARIANTS},
    ("k1", "k1 two chunks"): {v: (2, 0) for v in VARIANTS},
    ("k1", "k1 idle channels"): {v: (1, 0) for v in VARIANTS},
    ("columns", "k3 257 columns"): {"auto": _P80, "fp32": _P80},
    ("columns", "k3s2 513 columns"): {"auto": _P80, "fp32": _P80},
    ("rows8", "k3 8-byte rows"): {"auto": (1, 2)},
    ("rows8", "k3s2 8-byte gradient rows"): {"auto": (1, 2), "fp32": _P80},
}
# bytes of a staging piece where it is not 16 at full alignment: {(group, name): {variant: bytes}}
PIECE_BYTES = {
    ("rows8", "k3 8-byte rows"): {"auto": 8},
    ("rows8", "k3s2 8-byte gradient rows"): {"auto": 8, "fp32": 8, "direct": 8},
}
SPLIT_FORMS, UNIT_FORMS = ("X3", "X3S2"), ("WINO", "S2")


def alignment_class(x_align, g_align):
    """Index into a FORMS entry: 0 full, 1 g8, 2 rest."""
    return 0 if (x_align, g_align) == (16, 16) else (1 if (x_align, g_align) == (16, 8) else 2)


def expected_form(group, name, variant, x_align=16, g_align=16):
    return FORMS[(group, name)][variant][alignment_class(x_align, g_align)]


def expected_numbers(group, name, variant, form, cus):
    """Slots 2 and 3 of the query's info from the restatements above (`expected_dparts`, `wgrad_unit_count`), for the split-operand
    and 12-wave forms on a device of ``cus`` compute units; None for the other forms."""
    case = case_of(group, name)
    if form in SPLIT_FORMS:
        return expected_dparts(case, cus)[:2]
    if form in UNIT_FORMS:
        pairs, units = channel_pairs(case[1], case[2]), wgrad_unit_count(cus)
        parts = min(max(1, units // pairs), 512 // (2 if form == "WINO" else 4))
        return parts, max(units, ceil_div(parts * pairs, 8) * 8) // 8
    return None


# ------------------------------------------------------------------------------------------------------------------ descriptors
_GROUP_TABLES = {"k57": K57_CASES, "swap": ROLE_SWAP_CASES, "depth1": DEPTH1_CASES, "dparts": {k: v[0] for k, v in DPART_CASES.items()},
                 "pairs": PAIRS_CASES, "strided": {k: v[1] for k, v in STRIDED_CASES.items()},
                 "k1": {k: v[0] for k, v in K1_STREAM_CASES.items()}, "columns": COLUMN_LIMIT_CASES, "rows8": ROWS8_CASES}
DESC_FIELDS = ("N", "Cin", "Din", "Hin", "Win", "Cout", "Dout", "Hout", "Wout", "ksize", "stride", "dilation", "pad", "transposed",
               "algo", "x_batch_stride", "y_batch_stride")
ALGO_BITS = {"auto": 0, "fp32": 0x10000, "direct": 1}      # SNVC_ALGO_WGRAD_FP32, SNVC_ALGO_DIRECT


def case_of(group, name):
    """The case as (N, Cin, Cout, (D, H, W) of x, ksize, stride, dilation) of the convolution the descriptor states: a role-swapped
    case becomes the stride-2 convolution from the doubled grid."""
    c = _GROUP_TABLES[group][name]
    if len(c) == 4:
        n, cin_d, cout_d, shp = c
        return (n, cout_d, cin_d, tuple(2 * e for e in shp), 3, 2, 1)
    return c


def desc_fields(case, algo=0, extra_channels=0):
    """The snvc_conv3d_desc of a case as a dict over DESC_FIELDS; ``extra_channels``: x and g are channel slices of buffers that much
    wider (the batch strides say so)."""
    n, cin, cout, shp, k, stride, dil = case
    osh = out_shape(shp, k, stride, dil)
    f = dict(N=n, Cin=cin, Din=shp[0], Hin=shp[1], Win=shp[2], Cout=cout, Dout=osh[0], Hout=osh[1], Wout=osh[2], ksize=k, stride=stride,
             dilation=dil, pad=dil * (k - 1) // 2, transposed=0, algo=algo, x_batch_stride=0, y_batch_stride=0)
    if extra_channels:
        f["x_batch_stride"] = (cin + extra_channels) * int(np.prod(shp))
        f["y_batch_stride"] = (cout + extra_channels) * int(np.prod(osh))
    return f


def all_cases():
    """[(group, name)] of every case that has a form column, in a fixed order."""
    return [(g, n) for g in _GROUP_TABLES for n in sorted(_GROUP_TABLES[g])]


def case_desc_fields(group, name, variant="auto"):
    return desc_fields(case_of(group, name), ALGO_BITS[variant], STRIDED_EXTRA_CHANNELS if group == "strided" else 0)


def sweep_desc_fields():
    """200 descriptors for the workspace query: every key the dispatcher knows and two it refuses, x the channel counts around the
    32-channel blocks, over three extents."""
    keys = [(1, 1, 1), (3, 1, 1), (3, 2, 1), (5, 1, 1), (5, 1, 2), (7, 1, 1), (5, 2, 1), (3, 1, 2)]
    extents = [(4, 6, 40), (1, 12, 38), (9, 5, 33)]
    chans = (1, 5, 32, 40, 352)
    rows = []
    for k, stride, dil in keys:
        for cin in chans:
            for cout in chans:
                rows.append(desc_fields((1 + len(rows) % 2, cin, cout, extents[len(rows) % 3], k, stride, dil)))
    return rows


def refusal_desc_fields():
    """{what: descriptor (None: a null one)} that snvc_conv3d_wgrad refuses before it looks at a pointer."""
    ok = desc_fields((1, 8, 8, (4, 6, 8), 3, 1, 1))
    return {"null desc": None, "transposed": dict(ok, transposed=1), "zero batch": dict(ok, N=0), "zero input channels": dict(ok, Cin=0),
            "negative output channels": dict(ok, Cout=-1), "wrong pad": dict(ok, pad=0), "wrong output depth": dict(ok, Dout=5),
            "wrong output width": dict(ok, Wout=7), "accepted, null pointers": ok}


def make_desc(fields):
    """``snvc_amd._lib.Conv3dDesc`` of a field dict."""
    from snvc_amd import _lib
    d = _lib.Conv3dDesc()
    for k, v in fields.items():
        setattr(d, k, v)
    return d
