"""Cases of the fp32 forward convolution (csrc/conv3d.hip, csrc/conv3d_small.hip): one row per kernel form and epilogue variant that
a descriptor can reach -- the smallest shape that takes the form and still has the places where these kernels go wrong -- with the
form it must take and the launch numbers it must get, as snvc_conv3d_forward_form of include/snvc_forms.h reports them (the
header lists the forms and their conditions).  tests/test_conv_forward_forms_host.py holds the table to the query without a
device; tests/test_gpu_conv_forward_forms.py asks the query for the real addresses, runs the layer and compares with the float64
reference below.  No GPU import here.

A row: the layer (a key of `KEYS`), Cin, Cout, N, the INPUT extents (D, H, W), the epilogue flags, the SNVC_ALGO_* bits, the entry
point, where each operand lies (`off`: bytes off a 256-byte boundary; `pad`: floats added to the batch stride of x / y / the
residual, which makes the operand a channel slice of a wider buffer), then the form, the bytes of a staging piece and the epilogue
variant the query must report.  tiles / jobs, channel groups, the grid and the LDS bytes follow from the form's tile
(`expected_numbers`).

Shapes.  The Winograd tiles are 4 x 4 x 32 (2 x 4 x 64 and 4 x 4 x 64 under the tile bits) output voxels: (5, 6, 40) leaves D and
H ragged and gives two W tiles, the second 8 wide; (5, 6, 72) does the same for the 64-wide tiles.  Cin 6 is three chunks of two,
Cin 5 leaves the last chunk half empty; the direct forms get a Cin that is no multiple of their KC.  Cout 64 is two channel groups
(one MI = 2 workgroup on the direct forms).  N = 2, so that a batch stride is used, except in the CU-sized depth-1 pair (N = 1).
"""
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

INVALID, UNSUPPORTED = 1, 2               # SNVC_ERR_INVALID_ARGUMENT, SNVC_ERR_UNSUPPORTED
RELU, PRE, POST, SIGMOID, POOL = 1, 2, 4, 8, 16                      # SNVC_EPI_*
DIRECT, BIG, STD, NREG, GENERIC = 1, 0x100, 0x200, 0x300, 0x400      # SNVC_ALGO_*
ENTRIES = {"forward": 0, "head": 1, "side_head": 2, "stats": 3}      # snvc_conv3d_forward_entry
FILL = 7.0                                # what the buffers hold around a placed operand

# key: (ksize, stride, dilation, pad, transposed, planar, ksize_h)
KEYS = {
    "k1": (1, 1, 1, 0, False, False, 0), "k3": (3, 1, 1, 1, False, False, 0), "k3s2": (3, 2, 1, 1, False, False, 0),
    "k5": (5, 1, 1, 2, False, False, 0), "k5d2": (5, 1, 2, 4, False, False, 0), "k7": (7, 1, 1, 3, False, False, 0),
    "dc": (3, 2, 1, 1, True, False, 0),
    "p1": (1, 1, 1, 0, False, True, 0), "p1s2": (1, 2, 1, 0, False, True, 0), "p3": (3, 1, 1, 1, False, True, 0),
    "p3s2": (3, 2, 1, 1, False, True, 0), "p37": (7, 1, 1, 3, False, True, 3), "p3d2": (3, 1, 2, 2, False, True, 0),
    "dcp": (3, 2, 1, 1, True, True, 0),
    # what make_plan refuses
    "k5s2": (5, 2, 1, 2, False, False, 0), "k3 pad 0": (3, 1, 1, 0, False, False, 0), "p5": (5, 1, 1, 2, False, True, 0),
    "dc pad 0": (3, 2, 1, 0, True, False, 0),
}

# form: (family, MI, TD, TH, TW).  Families: "stream" (16-byte pieces of a channel), "k3c1", "dc1", "wino" (jobs
# of TD x TH x TW output voxels per 32-channel group and sample), "direct" (tiles of TD x TH x 32 output voxels, 32 * MI channels
# per workgroup), "deconv" (four -- depth-1: two -- parity classes of TD x TH x 32 INPUT tiles).
FORMS = {
    "POINTWISE_SMALL_1": ("stream", 1, 0, 0, 0), "POINTWISE_SMALL_2": ("stream", 1, 0, 0, 0),
    "POINTWISE_EXPAND_1": ("stream", 1, 0, 0, 0), "POINTWISE_EXPAND_2": ("stream", 1, 0, 0, 0),
    "K3_COUT1": ("k3c1", 1, 4, 8, 32), "DECONV_COUT1": ("dc1", 1, 0, 0, 0),
    "WINO_S2_PIPE4": ("wino", 1, 4, 4, 32), "WINO_S2_PIPE2": ("wino", 1, 4, 4, 32),
    "WINO_S2": ("wino", 1, 4, 4, 32), "WINO_S2_V8": ("wino", 1, 4, 4, 32),
    "WINO_K5": ("wino", 1, 4, 4, 32), "WINO_K5D2": ("wino", 1, 4, 4, 32), "WINO_K7": ("wino", 1, 4, 4, 32),
    "WINO_P": ("wino", 1, 1, 16, 32),
    "WINO_BIG": ("wino", 1, 4, 4, 64), "WINO_N3": ("wino", 1, 4, 4, 32), "WINO_N": ("wino", 1, 4, 4, 32),
    "WINO_N8": ("wino", 1, 4, 4, 32), "WINO": ("wino", 1, 2, 4, 64), "WINO8": ("wino", 1, 2, 4, 64),
    "K1M1": ("direct", 1, 4, 4, 32), "K1M2": ("direct", 2, 4, 4, 32),
    "K3M1": ("direct", 1, 4, 4, 32), "K3M2": ("direct", 2, 4, 4, 32),
    "K3S2M1": ("direct", 1, 2, 4, 32), "K3S2M2": ("direct", 2, 2, 4, 32),
    "K5M1": ("direct", 1, 4, 4, 32), "K5M2": ("direct", 2, 4, 4, 32),
    "K5D2M1": ("direct", 1, 4, 4, 32), "K5D2M2": ("direct", 2, 4, 4, 32),
    "K7M1": ("direct", 1, 4, 4, 32), "K7M2": ("direct", 2, 4, 4, 32),
    "P1M1S": ("direct", 1, 1, 4, 32), "P1S2M1S": ("direct", 1, 1, 4, 32), "P3M1S": ("direct", 1, 1, 4, 32),
    "P3S2M1S": ("direct", 1, 1, 4, 32), "P7M1S": ("direct", 1, 1, 4, 32), "P3D2M1S": ("direct", 1, 1, 4, 32),
    "DCM1": ("deconv", 1, 2, 4, 32), "DCM2": ("deconv", 2, 2, 4, 32), "DCM1_V8": ("deconv", 1, 2, 4, 32),
    "DCM2_V8": ("deconv", 2, 2, 4, 32), "DCP": ("deconv", 1, 1, 8, 32), "DCP_V8": ("deconv", 1, 1, 8, 32),
}
# dynamic LDS bytes of each configuration (Cfg::LDS_BYTES, recorded from the library); a Winograd launch adds 256 bytes of
# scale | bias, 384 with the side head's weights.  The streaming and VALU forms use none.
LDS = {
    "WINO_S2_PIPE4": 73728, "WINO_S2_PIPE2": 73728, "WINO_S2": 71712, "WINO_S2_V8": 71712,
    "WINO_K5": 40960, "WINO_K5D2": 66560, "WINO_K7": 67840, "WINO_P": 20736,
    "WINO_BIG": 69120, "WINO_N3": 50688, "WINO_N": 50688, "WINO_N8": 50688, "WINO": 55296, "WINO8": 55296,
    "K1M1": 34816, "K1M2": 36864, "K3M1": 73728, "K3M2": 101376, "K3S2M1": 38304, "K3S2M2": 52128,
    "K5M1": 53760, "K5M2": 66560, "K5D2M1": 58880, "K5D2M2": 71680, "K7M1": 57088, "K7M2": 82176,
    "P1M1S": 40960, "P1S2M1S": 61440, "P3M1S": 67584, "P3S2M1S": 57600, "P7M1S": 58368, "P3D2M1S": 77824,
    "DCM1": 29568, "DCM2": 41856, "DCM1_V8": 29568, "DCM2_V8": 41856, "DCP": 33024, "DCP_V8": 33024,
}


@dataclass(frozen=True, repr=False)
class Case:
    name: str
    key: str
    cin: int
    cout: int
    sp: Tuple[int, int, int]              # input extents (D, H, W)
    form: Optional[str]                   # SNVC_CF_* without the prefix; None: a refusal or an empty batch
    piece: int = 0                        # bytes of an input staging piece
    epi: int = 0                          # the epilogue variant (snvc_forms.h)
    n: int = 2
    flags: int = 0
    bits: int = 0
    entry: str = "forward"
    planes: bool = False
    off: dict = field(default_factory=dict, hash=False, compare=False)      # x, y, res, planes: bytes off a 256-byte boundary
    pad: dict = field(default_factory=dict, hash=False, compare=False)      # x, y, res: floats added to the batch stride
    refusal: Optional[Tuple[int, str]] = None                               # (status, text the message starts with)
    bound: str = "TIGHT"                  # test_gpu_parity.TIGHT (2e-5), or WINO7 (3e-4) for the k7 Winograd form
    gpu: bool = True                      # False: only the query can pose the row (no wrapper passes such a call on)
    align: dict = field(default_factory=dict, hash=False, compare=False)    # host test: alignments that no placement gives (0: NULL)
    jobs_per_cu: int = 0                  # depth-1 Winograd pair: extents (1, 256, 4 * CUs + jobs_per_cu's W offset), see shape()

    def __str__(self):
        return self.name

    __repr__ = __str__

    @property
    def residual(self):
        return bool(self.flags & (PRE | POST))

    def shape(self, cus):
        """The input extents; the unforced depth-1 Winograd pair scales with the CU count (16 x CUs / 8 jobs, or one column of
        jobs fewer)."""
        if not self.jobs_per_cu:
            return self.sp
        return (1, 256, 4 * cus + (0 if self.jobs_per_cu > 0 else -32))


def ceil_div(a, b):
    return -(-a // b)


def out_spatial(key, sp):
    k, s, dil, pad, transposed, planar, kh = KEYS[key]
    if transposed:
        return (sp[0] if planar else 2 * sp[0], 2 * sp[1], 2 * sp[2])
    eff = dil * (k - 1) + 1
    ext = lambda v, kk, p: (v + 2 * p - (dil * (kk - 1) + 1)) // s + 1
    if planar:
        khh = kh or k
        return (sp[0], ext(sp[1], khh, dil * (khh - 1) // 2), ext(sp[2], k, pad))
    return tuple((v + 2 * pad - eff) // s + 1 for v in sp)


def batch_strides(case, cus=256):
    """(x, y, residual) batch strides in floats as the wrappers of snvc_amd.ops pass them: the operand's own stride; 0 for an
    output the wrapper allocates for a pooled or fused-head call, and for an absent residual."""
    sp = case.shape(cus)
    osp = out_spatial(case.key, sp)
    x_bs = case.cin * int(np.prod(sp)) + case.pad.get("x", 0)
    y_bs = case.cout * int(np.prod(osp)) + case.pad.get("y", 0)
    r_bs = case.cout * int(np.prod(osp)) + case.pad.get("res", 0) if case.residual else 0
    if case.entry == "head" or case.flags & POOL:
        y_bs = 0
    if case.entry == "stats":
        r_bs = 0
    return x_bs, y_bs, r_bs


def geometry(case):
    """The layer's snvc_amd.ops._ConvGeometry without a device (what Conv3dLayer derives its descriptor from)."""
    from snvc_amd import ops
    k, s, dil, pad, transposed, planar, kh = KEYS[case.key]
    shape = (case.cin, case.cout) if transposed else (case.cout, case.cin)
    g = ops._ConvGeometry(torch.empty(shape + (1, 1, 1), device="meta"), k, s, pad, dil, transposed)
    g.planar, g.ksize_h = planar, kh
    return g


def desc_args(case, cus=256):
    """The arguments of _ConvGeometry._desc for the row's call."""
    return (case.n, case.shape(cus), case.flags, case.bits) + batch_strides(case, cus)


def address_align(off):
    return 16 if off % 16 == 0 else 8 if off % 8 == 0 else 4


def alignments(case):
    """(x, y, residual, planes, y_head) alignments of the row's placement: the largest of 16 / 8 / 4 dividing 256 + off, 0 for an
    operand the call does not have."""
    a = {
        "x": address_align(case.off.get("x", 0)),
        "y": 0 if case.entry == "head" else address_align(case.off.get("y", 0)),
        "res": address_align(case.off.get("res", 0)) if case.residual else 0,
        "planes": address_align(case.off.get("planes", 0)) if case.planes else 0,
        "y_head": 16 if case.entry in ("head", "side_head") else 0,
    }
    a.update(case.align)
    return tuple(a[k] for k in ("x", "y", "res", "planes", "y_head"))


def expected_numbers(case, cus=256):
    """{info name: value} the query must report for the row's form."""
    family, mi, td, th, tw = FORMS[case.form]
    sp = case.shape(cus)
    osp = out_spatial(case.key, sp)
    n, s_out = case.n, int(np.prod(osp))
    if family == "stream":
        tiles, groups, gx, gyz = s_out // 4, 1, min(ceil_div(s_out // 4, 256), 4096), n
    elif family == "k3c1":
        tiles = ceil_div(osp[0], td) * ceil_div(osp[1], th) * ceil_div(osp[2], tw)
        groups, gx, gyz = 1, tiles, n
    elif family == "dc1":
        tiles = sp[0] * sp[1] * (sp[2] // 4)
        groups, gx, gyz = 1, ceil_div(tiles, 256), n
    elif family == "wino":
        groups = ceil_div(case.cout, 32)
        tiles = ceil_div(osp[0], td) * ceil_div(osp[1], th) * ceil_div(osp[2], tw) * groups * n
        gx, gyz = tiles, 1
    else:
        ext = sp if family == "deconv" else osp
        tiles = ceil_div(ext[0], td) * ceil_div(ext[1], th) * ceil_div(ext[2], tw)
        if family == "deconv":
            tiles *= 2 if KEYS[case.key][5] else 4
        groups = ceil_div(case.cout, 32 * mi)
        gx, gyz = tiles, groups * n
    lds = LDS.get(case.form, 0)
    if family == "wino":
        lds += 384 if case.epi // 4 == 1 else 256
    return dict(piece_bytes=case.piece, epi=case.epi, tiles=tiles, groups=groups, grid_x=gx, grid_yz=gyz, threads=256, lds=lds)


# ------------------------------------------------------------------------------------------------------------------ the table
_SIDE = "snvc_conv3d_forward_side_head: needs the default Winograd form"
_POOL = "snvc_conv3d_forward: SNVC_EPI_AVGPOOL_D4 needs the default Winograd form"
_STATS = "snvc_conv3d_forward_stats: this layer does not take the default Winograd form"
_STATS_ROWS = "snvc_conv3d_forward_stats: the layer's rows do not allow"
_STATS_S2 = "snvc_conv3d_forward_stats: this stride-2 layer does not take the default kernel form"
A, B, C = (5, 6, 40), (5, 6, 72), (5, 6, 38)          # 3x3x3 stride 1: 32-wide tiles, 64-wide tiles, 8-byte rows


def _k3():
    return [
        # the default form: 4 x 4 x 32 tiles, LDS-DMA staged
        Case("k3 n3", "k3", 6, 32, A, "WINO_N3", 16, 0, flags=RELU),
        Case("k3 n3 residual, odd Cin, two groups", "k3", 5, 64, A, "WINO_N3", 16, 1, flags=RELU | PRE),
        Case("k3 n3 planes", "k3", 6, 32, A, "WINO_N3", 16, 2, planes=True),
        Case("k3 n3 residual after, planes", "k3", 5, 64, A, "WINO_N3", 16, 3, flags=RELU | POST, planes=True),
        Case("k3 n3 sliced x and y", "k3", 6, 32, A, "WINO_N3", 16, 0, pad=dict(x=3 * 1200, y=1200)),
        # its 8-byte-row twin, reached through the width, the address and the batch stride of x, and through y / residual
        Case("k3 n8 W 38", "k3", 6, 32, C, "WINO_N8", 8, 0, flags=RELU),
        Case("k3 n8 W 38 residual, planes", "k3", 5, 64, C, "WINO_N8", 8, 3, flags=PRE, planes=True),
        Case("k3 n8 x 8 bytes off", "k3", 6, 32, A, "WINO_N8", 8, 0, off=dict(x=8)),
        Case("k3 n8 x batch stride 2 off", "k3", 6, 32, A, "WINO_N8", 8, 0, pad=dict(x=2)),
        Case("k3 n8 y 8 bytes off", "k3", 6, 32, A, "WINO_N8", 8, 0, off=dict(y=8)),
        Case("k3 n8 y batch stride 2 off", "k3", 6, 32, A, "WINO_N8", 8, 0, pad=dict(y=2)),
        Case("k3 n8 residual 8 bytes off", "k3", 6, 32, A, "WINO_N8", 8, 1, flags=RELU | PRE, off=dict(res=8)),
        Case("k3 n8 planes 8 bytes off", "k3", 6, 32, A, "WINO_N8", 8, 2, planes=True, off=dict(planes=8)),
        Case("k3 n8 under the big-tile bit", "k3", 6, 32, C, "WINO_N8", 8, 0, bits=BIG),
        Case("k3 n8 under the register-staged bit", "k3", 6, 32, C, "WINO_N8", 8, 0, bits=NREG),
        # the tile bits
        Case("k3 nreg", "k3", 6, 32, A, "WINO_N", 16, 0, bits=NREG),
        Case("k3 nreg residual, planes", "k3", 5, 64, A, "WINO_N", 16, 3, flags=RELU | PRE, planes=True, bits=NREG),
        Case("k3 big", "k3", 6, 32, B, "WINO_BIG", 16, 0, bits=BIG),
        Case("k3 big residual", "k3", 5, 64, B, "WINO_BIG", 16, 1, flags=RELU | POST, bits=BIG),
        Case("k3 big planes", "k3", 6, 32, B, "WINO_BIG", 16, 2, planes=True, bits=BIG),
        Case("k3 std", "k3", 6, 32, B, "WINO", 16, 0, bits=STD),
        Case("k3 std residual, planes", "k3", 5, 64, B, "WINO", 16, 3, flags=RELU | PRE, planes=True, bits=STD),
        Case("k3 std8 W 70", "k3", 6, 32, (5, 6, 70), "WINO8", 8, 0, bits=STD),
        Case("k3 std8 x 8 bytes off, residual", "k3", 5, 64, B, "WINO8", 8, 1, flags=PRE, bits=STD, off=dict(x=8)),
        Case("k3 std8 x batch stride 2 off", "k3", 6, 32, B, "WINO8", 8, 0, bits=STD, pad=dict(x=2)),
        # what leaves the Winograd family
        Case("k3 odd width", "k3", 6, 32, (5, 6, 37), "K3M1", 4, 0, flags=RELU),
        Case("k3 x 4 bytes off", "k3", 6, 32, A, "K3M1", 4, 0, off=dict(x=4)),
        Case("k3 y 4 bytes off", "k3", 6, 32, A, "K3M1", 16, 0, off=dict(y=4)),
        Case("k3 Cout 27", "k3", 6, 27, A, "K3M1", 16, 0, flags=RELU | PRE),
        Case("k3 Sigmoid, Cout 64", "k3", 6, 64, A, "K3M2", 16, 0, flags=SIGMOID),
        Case("k3 direct bit", "k3", 5, 64, A, "K3M2", 16, 0, flags=RELU | POST, bits=DIRECT),
        Case("k3 generic-epilogue bit", "k3", 6, 32, A, "K3M1", 16, 0, bits=GENERIC),
        # side head, depth-4 average, statistics: the default form alone
        Case("k3 side head", "k3", 6, 32, A, "WINO_N3", 16, 4, flags=RELU, entry="side_head"),
        Case("k3 side head W 38", "k3", 6, 32, C, None, entry="side_head", refusal=(UNSUPPORTED, _SIDE)),
        Case("k3 side head nreg", "k3", 6, 32, A, None, entry="side_head", bits=NREG, refusal=(UNSUPPORTED, _SIDE)),
        Case("k3 side head Cout 64", "k3", 6, 64, A, None, entry="side_head", refusal=(UNSUPPORTED, _SIDE)),
        Case("k3 side head residual", "k3", 6, 32, A, None, entry="side_head", flags=PRE, refusal=(UNSUPPORTED, _SIDE)),
        Case("k3 side head y_head 8 bytes off", "k3", 6, 32, A, None, entry="side_head", refusal=(UNSUPPORTED, _SIDE), gpu=False,
             align=dict(y_head=8)),
        Case("k3 side head direct bit", "k3", 6, 32, A, None, entry="side_head", bits=DIRECT,
             refusal=(UNSUPPORTED, "snvc_conv3d_forward_side_head: built for 3x3x3 / stride-1 layers on the Winograd path")),
        Case("k5 side head", "k5", 6, 32, (6, 7, 36), None, entry="side_head",
             refusal=(UNSUPPORTED, "snvc_conv3d_forward_side_head: built for 3x3x3 / stride-1 Conv3d layers")),
        Case("k3 pooled", "k3", 6, 32, (8, 6, 40), "WINO_N3", 16, 8, flags=RELU | POOL),
        Case("k3 pooled two groups", "k3", 5, 64, (8, 6, 40), "WINO_N3", 16, 8, flags=POOL),
        Case("k3 pooled W 38", "k3", 6, 32, (8, 6, 38), None, flags=POOL, refusal=(UNSUPPORTED, _POOL)),
        Case("k3 pooled nreg", "k3", 6, 32, (8, 6, 40), None, flags=POOL, bits=NREG, refusal=(UNSUPPORTED, _POOL)),
        Case("k3 pooled x 4 bytes off", "k3", 6, 32, (8, 6, 40), None, flags=POOL, off=dict(x=4),
             refusal=(UNSUPPORTED, "snvc_conv3d_forward: SNVC_EPI_AVGPOOL_D4 needs 16-byte aligned rows")),
        Case("k3 pooled D 6", "k3", 6, 32, (6, 6, 40), None, flags=POOL,
             refusal=(UNSUPPORTED, "snvc_conv3d_forward: SNVC_EPI_AVGPOOL_D4 is built for")),
        Case("k3 pooled direct bit", "k3", 6, 32, (8, 6, 40), None, flags=POOL, bits=DIRECT,
             refusal=(UNSUPPORTED, "snvc_conv3d_forward: SNVC_EPI_AVGPOOL_D4 is built for")),
        Case("k3 stats", "k3", 6, 32, A, "WINO_N3", 16, 12, entry="stats"),
        Case("k3 stats two groups", "k3", 5, 64, A, "WINO_N3", 16, 12, entry="stats"),
        Case("k3 stats W 38", "k3", 6, 32, C, None, entry="stats", refusal=(UNSUPPORTED, _STATS)),
        Case("k3 stats nreg", "k3", 6, 32, A, None, entry="stats", bits=NREG, refusal=(UNSUPPORTED, _STATS)),
        Case("k3 stats x 4 bytes off", "k3", 6, 32, A, None, entry="stats", off=dict(x=4), refusal=(UNSUPPORTED, _STATS_ROWS)),
        Case("k3 stats Cout 40", "k3", 6, 40, A, None, entry="stats", refusal=(UNSUPPORTED, "snvc_conv3d_forward_stats: built for")),
    ]


S2A, S2B = (7, 9, 72), (7, 9, 44)         # odd D and H; output rows of 36 (16-byte) and 22 (8-byte)


def _s2():
    return [
        Case("s2 pipe4", "k3s2", 6, 32, S2A, "WINO_S2_PIPE4", 16, 0, flags=RELU),
        Case("s2 pipe4 residual", "k3s2", 5, 64, S2A, "WINO_S2_PIPE4", 16, 1, flags=RELU | PRE),
        Case("s2 pipe2 rows of 22", "k3s2", 6, 32, S2B, "WINO_S2_PIPE2", 16, 0, flags=RELU),
        Case("s2 pipe2 rows of 22 residual", "k3s2", 5, 64, S2B, "WINO_S2_PIPE2", 16, 1, flags=RELU | POST),
        Case("s2 pipe2 y 8 bytes off", "k3s2", 6, 32, S2A, "WINO_S2_PIPE2", 16, 0, off=dict(y=8)),
        Case("s2 std", "k3s2", 6, 32, S2A, "WINO_S2", 16, 0, bits=STD),
        Case("s2 std residual", "k3s2", 5, 64, S2A, "WINO_S2", 16, 1, flags=RELU | PRE, bits=STD),
        Case("s2 std rows of 22", "k3s2", 6, 32, S2B, "WINO_S2_V8", 16, 0, bits=STD),
        Case("s2 std rows of 22 residual", "k3s2", 5, 64, S2B, "WINO_S2_V8", 16, 1, flags=RELU | PRE, bits=STD),
        Case("s2 stats", "k3s2", 6, 32, S2A, "WINO_S2_PIPE4", 16, 12, entry="stats"),
        Case("s2 stats two groups", "k3s2", 5, 64, S2A, "WINO_S2_PIPE4", 16, 12, entry="stats"),
        Case("s2 stats std", "k3s2", 6, 32, S2A, None, entry="stats", bits=STD, refusal=(UNSUPPORTED, _STATS_S2)),
        Case("s2 stats rows of 22", "k3s2", 6, 32, S2B, None, entry="stats", refusal=(UNSUPPORTED, _STATS_S2)),
        Case("s2 stats x 4 bytes off", "k3s2", 6, 32, S2A, None, entry="stats", off=dict(x=4), refusal=(UNSUPPORTED, _STATS_ROWS)),
        # the direct configurations (KC = 2) with their three epilogues
        Case("s2 direct fast", "k3s2", 5, 32, S2A, "K3S2M1", 16, 1, flags=RELU, bits=DIRECT),
        Case("s2 direct fast residual", "k3s2", 5, 32, S2A, "K3S2M1", 16, 2, flags=RELU | PRE, bits=DIRECT),
        Case("s2 Cout 27", "k3s2", 5, 27, S2A, "K3S2M1", 16, 0, flags=RELU | PRE),
        Case("s2 odd width", "k3s2", 5, 32, (7, 9, 37), "K3S2M1", 4, 0, flags=RELU),
        Case("s2 M2 direct fast", "k3s2", 5, 64, S2A, "K3S2M2", 16, 1, bits=DIRECT),
        Case("s2 M2 direct fast residual", "k3s2", 5, 64, S2A, "K3S2M2", 16, 2, flags=RELU | POST, bits=DIRECT),
        Case("s2 M2 generic-epilogue bit", "k3s2", 5, 64, S2A, "K3S2M2", 16, 0, bits=DIRECT | GENERIC),
        Case("s2 M2 Sigmoid", "k3s2", 5, 40, S2A, "K3S2M2", 16, 0, flags=SIGMOID),
        Case("s2 planes", "k3s2", 6, 32, S2A, None, planes=True,
             refusal=(UNSUPPORTED, "snvc_conv3d_forward_ex: depth planes need a stride-1 Conv3d with Dout >= 2")),
    ]


K = (6, 7, 36)


def _k57():
    rows = []
    for key, wino, m1, m2, fast, bound in (("k5", "WINO_K5", "K5M1", "K5M2", True, "TIGHT"), ("k5d2", "WINO_K5D2", "K5D2M1", "K5D2M2", False, "TIGHT"),
                                            ("k7", "WINO_K7", "K7M1", "K7M2", True, "WINO7")):
        rows += [
            Case(f"{key} wino", key, 6, 32, K, wino, 16, 0, flags=RELU, bound=bound),
            Case(f"{key} wino residual", key, 5, 64, K, wino, 16, 1, flags=RELU | PRE, bound=bound),
            Case(f"{key} direct", key, 6, 32, K, m1, 16, 1 if fast else 0, flags=RELU, bits=DIRECT),
            Case(f"{key} direct residual", key, 5, 32, K, m1, 16, 2 if fast else 0, flags=RELU | PRE, bits=DIRECT),
            Case(f"{key} Cout 27", key, 5, 27, K, m1, 16, 0, flags=RELU),
            Case(f"{key} W 38", key, 5, 32, (6, 7, 38), m1, 4, 0),
            Case(f"{key} direct M2", key, 5, 64, K, m2, 16, 0, flags=RELU | POST, bits=DIRECT),
            Case(f"{key} M2 Cout 40", key, 6, 40, K, m2, 16, 0),
        ]
    return rows


P, T = (3, 5, 36), (3, 5, 8)


def _k1_and_small():
    return [
        Case("k1 M1", "k1", 12, 32, P, "K1M1", 16, 0, flags=RELU | PRE),
        Case("k1 M1 Cout 27, odd width", "k1", 12, 27, (3, 5, 37), "K1M1", 4, 0, flags=RELU),
        Case("k1 M2", "k1", 12, 64, P, "K1M2", 16, 0, flags=RELU | POST),
        Case("k1 M2 Cout 40 Sigmoid", "k1", 12, 40, P, "K1M2", 16, 0, flags=SIGMOID),
        # streaming forms and the sibling each takes
        Case("k1 to one", "k1", 6, 1, P, "POINTWISE_SMALL_1", 16, 0, flags=SIGMOID),
        Case("k1 to two", "k1", 6, 2, P, "POINTWISE_SMALL_2", 16, 0, flags=RELU | PRE),
        Case("k1 to one, voxels not in fours", "k1", 6, 1, (3, 5, 37), "K1M1", 4, 0),
        Case("k1 to two, x 8 bytes off", "k1", 6, 2, P, "K1M1", 4, 0, off=dict(x=8)),
        Case("k1 to two, residual 8 bytes off", "k1", 6, 2, P, "K1M1", 16, 0, flags=PRE, off=dict(res=8)),
        Case("k1 from one", "k1", 1, 32, P, "POINTWISE_EXPAND_1", 16, 0, flags=RELU),
        Case("k1 from two", "k1", 2, 40, P, "POINTWISE_EXPAND_2", 16, 0, flags=RELU | POST),
        Case("k1 from one, voxels not in fours", "k1", 1, 32, (3, 5, 37), "K1M1", 4, 0),
        Case("k1 from two, y 8 bytes off", "k1", 2, 40, P, "K1M2", 16, 0, off=dict(y=8)),
        Case("k1 from two, direct bit", "k1", 2, 40, P, "K1M2", 16, 0, bits=DIRECT),
        Case("k3 to one", "k3", 6, 1, (5, 6, 37), "K3_COUT1", 4, 0, flags=RELU | PRE),
        Case("k3 to one, planes", "k3", 6, 1, (5, 6, 37), "K3M1", 4, 0, planes=True),
        Case("dc to one", "dc", 6, 1, T, "DECONV_COUT1", 16, 0, flags=RELU | PRE),
        Case("dc to one, Win 6", "dc", 6, 1, (3, 5, 6), "DCM1_V8", 8, 0, flags=RELU),
    ]


Q = (1, 9, 36)


def _depth1():
    return [
        Case("p1", "p1", 40, 32, Q, "P1M1S", 16, 0, flags=RELU),
        Case("p1 Cout 64 residual", "p1", 40, 64, Q, "P1M1S", 16, 0, flags=RELU | PRE),
        Case("p1s2", "p1s2", 20, 32, Q, "P1S2M1S", 16, 0, flags=RELU),
        Case("p1s2 odd width", "p1s2", 20, 27, (1, 9, 37), "P1S2M1S", 4, 0),
        Case("p3 Cout 27", "p3", 20, 27, Q, "P3M1S", 16, 0, flags=RELU),
        Case("p3 fast", "p3", 20, 32, Q, "P3M1S", 16, 1, flags=RELU),
        Case("p3 fast residual", "p3", 20, 64, Q, "P3M1S", 16, 2, flags=RELU | PRE),
        Case("p3s2 fast", "p3s2", 12, 32, (1, 9, 40), "P3S2M1S", 16, 1, flags=RELU),
        Case("p3s2 fast residual", "p3s2", 12, 64, (1, 9, 40), "P3S2M1S", 16, 2, flags=RELU | POST),
        Case("p3s2 odd width", "p3s2", 12, 32, (1, 9, 37), "P3S2M1S", 4, 0),
        Case("p37", "p37", 6, 32, Q, "P7M1S", 16, 0, flags=RELU),
        Case("p37 Cout 40 residual, odd width", "p37", 6, 40, (1, 9, 37), "P7M1S", 4, 0, flags=RELU | PRE),
        Case("p3d2 fast", "p3d2", 20, 32, Q, "P3D2M1S", 16, 1, flags=RELU),
        Case("p3d2 fast residual", "p3d2", 20, 64, Q, "P3D2M1S", 16, 2, flags=RELU | PRE),
        Case("p3d2 Sigmoid", "p3d2", 20, 32, Q, "P3D2M1S", 16, 0, flags=SIGMOID),
        Case("dcp", "dcp", 6, 32, Q, "DCP", 16, 1, flags=RELU),
        Case("dcp residual", "dcp", 6, 64, Q, "DCP", 16, 2, flags=RELU | PRE),
        Case("dcp rows of 38", "dcp", 6, 32, (1, 9, 38), "DCP_V8", 8, 1, flags=RELU),
        Case("dcp odd width", "dcp", 6, 32, (1, 9, 37), "DCP", 4, 0),
        Case("dcp Cout 27", "dcp", 6, 27, Q, "DCP", 16, 0, flags=RELU),
        Case("dcp head", "dcp", 6, 32, Q, None, entry="head", gpu=False,
             refusal=(UNSUPPORTED, "snvc_conv3d_forward_head: layer is not a single-group transposed convolution")),
        # the depth-1 Winograd tile (1 x 16 x 32): forced, and unforced on either side of two jobs per CU
        Case("winop forced", "p3", 6, 32, (1, 34, 36), "WINO_P", 16, 0, flags=RELU, bits=BIG),
        Case("winop forced residual", "p3", 5, 64, (1, 34, 36), "WINO_P", 16, 1, flags=RELU | PRE, bits=BIG),
        Case("winop forced, rows of 38", "p3", 6, 32, (1, 34, 38), "P3M1S", 4, 0, bits=BIG),
        Case("winop two jobs per CU", "p3", 2, 32, (1, 256, 1024), "WINO_P", 16, 0, n=1, jobs_per_cu=1),
        Case("winop just under two jobs per CU", "p3", 2, 32, (1, 256, 992), "P3M1S", 16, 1, n=1, jobs_per_cu=-1),
    ]


def _transposed():
    head = "snvc_conv3d_forward_head: needs a transposed layer with 32 output channels"
    return [
        Case("dc M1", "dc", 6, 32, T, "DCM1", 16, 1, flags=RELU),
        Case("dc M1 Cout 64 residual", "dc", 6, 64, T, "DCM1", 16, 2, flags=RELU | PRE),
        Case("dc M2 Cout 40", "dc", 6, 40, T, "DCM2", 16, 0, flags=RELU | PRE),
        Case("dc M1 Win 6", "dc", 6, 32, (3, 5, 6), "DCM1_V8", 8, 1, flags=RELU),
        Case("dc M1 Win 6 residual", "dc", 6, 64, (3, 5, 6), "DCM1_V8", 8, 2, flags=RELU | POST),
        Case("dc M2 Win 6", "dc", 6, 40, (3, 5, 6), "DCM2_V8", 8, 0, flags=RELU),
        Case("dc M1 odd Win", "dc", 6, 32, (3, 5, 7), "DCM1", 4, 0, flags=RELU | PRE),
        Case("dc M1 Sigmoid", "dc", 6, 32, T, "DCM1", 16, 0, flags=SIGMOID),
        Case("dc M1 x 8 bytes off", "dc", 6, 32, T, "DCM1_V8", 8, 1, off=dict(x=8)),
        Case("dc head", "dc", 6, 32, T, "DCM1", 16, 3, flags=RELU, entry="head"),
        Case("dc head residual", "dc", 6, 32, T, "DCM1", 16, 4, flags=RELU | PRE, entry="head"),
        Case("dc head Win 6", "dc", 6, 32, (3, 5, 6), "DCM1_V8", 8, 3, flags=RELU, entry="head"),
        Case("dc head Cout 64", "dc", 6, 64, T, None, entry="head", refusal=(UNSUPPORTED, head)),
        Case("dc head odd Win", "dc", 6, 32, (3, 5, 7), None, entry="head", refusal=(UNSUPPORTED, head)),
        Case("dc stats", "dc", 6, 32, T, "DCM1", 16, 5, entry="stats"),
        Case("dc stats two groups", "dc", 6, 64, T, "DCM1", 16, 5, entry="stats"),
        Case("dc stats Win 6", "dc", 6, 32, (3, 5, 6), None, entry="stats", refusal=(UNSUPPORTED, _STATS_ROWS)),
        Case("dc y 4 bytes off", "dc", 6, 32, T, None, off=dict(y=4),
             refusal=(INVALID, "snvc_conv3d_forward: transposed y / residual must be 8-byte aligned")),
        Case("dc residual 4 bytes off", "dc", 6, 32, T, None, flags=PRE, off=dict(res=4),
             refusal=(INVALID, "snvc_conv3d_forward: transposed y / residual must be 8-byte aligned")),
    ]


def _host_only():
    """Empty batches and the refusals no wrapper passes on (they validate first, or never give such a pointer)."""
    h = dict(gpu=False)
    return [
        Case("k3 empty batch", "k3", 6, 32, A, None, n=0, **h),
        Case("dc empty batch", "dc", 6, 32, T, None, n=0, **h),
        Case("stats empty batch", "k3", 6, 32, A, None, n=0, entry="stats", refusal=(INVALID, "snvc_conv3d_forward_stats: empty batch"), **h),
        Case("null x", "k3", 6, 32, A, None, align=dict(x=0), refusal=(INVALID, "snvc_conv3d_forward: null pointer"), **h),
        Case("null y", "k3", 6, 32, A, None, align=dict(y=0), refusal=(INVALID, "snvc_conv3d_forward: null pointer"), **h),
        Case("side head null y_head", "k3", 6, 32, A, None, entry="side_head", align=dict(y_head=0),
             refusal=(INVALID, "snvc_conv3d_forward_side_head: null pointer"), **h),
        Case("residual flag, no residual", "k3", 6, 32, A, None, flags=PRE, align=dict(res=0),
             refusal=(INVALID, "snvc_conv3d_forward: residual flag without residual pointer"), **h),
        Case("both residual flags", "k3", 6, 32, A, None, flags=PRE | POST,
             refusal=(INVALID, "snvc_conv3d_forward: ADD_PRE and ADD_POST are exclusive"), **h),
        Case("sample of 2^31", "k1", 2, 32, (1024, 1024, 1024), None, n=1,
             refusal=(UNSUPPORTED, "snvc_conv3d_forward: one sample must stay below 2^31 elements"), **h),
        Case("no channels", "k3", 0, 32, A, None, refusal=(INVALID, "snvc_conv3d: sizes must be positive"), **h),
        Case("k5 stride 2", "k5s2", 6, 32, K, None, refusal=(UNSUPPORTED, "snvc_conv3d: (ksize,stride,dilation) not in"), **h),
        Case("k3 pad 0", "k3 pad 0", 6, 32, A, None, refusal=(UNSUPPORTED, "snvc_conv3d: pad must equal dilation*(ksize-1)/2"), **h),
        Case("depth-1 k5", "p5", 6, 32, Q, None, refusal=(UNSUPPORTED, "snvc_conv3d: depth-1 layers are built for"), **h),
        Case("transposed pad 0", "dc pad 0", 6, 32, T, None, refusal=(UNSUPPORTED, "snvc_conv3d: transposed conv supports k3,s2,p1,op1 only"), **h),
        Case("too many samples", "k3", 6, 32, A, None, n=65536, refusal=(UNSUPPORTED, "snvc_conv3d: too many channel groups or samples"), **h),
    ]


CASES = _k3() + _s2() + _k57() + _k1_and_small() + _depth1() + _transposed() + _host_only()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GPU_CASES = [c for c in CASES if c.gpu]


# ------------------------------------------------------------------------------------------------------------------ operands
def seed_of(case):
    return 4000 + CASES.index(BY_NAME[case.name])


def weight_shape(case):
    k, s, dil, pad, transposed, planar, kh = KEYS[case.key]
    io = (case.cin, case.cout) if transposed else (case.cout, case.cin)
    if planar:
        return io + ((1, 3, 3) if transposed else (1, kh or k, k))
    return io + (k, k, k)


def make_values(case, cus=256):
    """{name: float32 CPU tensor} of the row's operands, from its seed: x, weight, scale, bias (none for a statistics row), and
    residual / planes / head_w where the row has them."""
    r = np.random.default_rng(seed_of(case))
    sp = case.shape(cus)
    osp = out_spatial(case.key, sp)
    t = lambda *shape, s=1.0: torch.from_numpy((r.standard_normal(shape) * s).astype(np.float32))
    fan = case.cin * int(np.prod(weight_shape(case)[2:]))
    v = {"x": t(case.n, case.cin, *sp), "weight": t(*weight_shape(case), s=1.0 / np.sqrt(max(fan, 1)))}
    if case.entry != "stats":
        v["scale"] = 1.0 + t(case.cout, s=0.2)
        v["bias"] = t(case.cout, s=0.3)
    if case.residual:
        v["residual"] = t(case.n, case.cout, *osp)
    if case.planes:
        v["planes"] = t(case.n, case.cout, 3, *osp[1:], s=0.5)
    if case.entry in ("head", "side_head"):
        v["head_w"] = t(case.cout, s=0.3)
    return v


# ------------------------------------------------------------------------------------------------------------------ reference
def reference(case, v):
    """(y, y_head) in float64 on the CPU: the convolution, then snvc_hip.h's epilogue in its order -- depth planes before the affine,
    the affine, the residual before or after the activation -- then the depth-4 average and the one-channel projection."""
    k, s, dil, pad, transposed, planar, kh = KEYS[case.key]
    x, w = v["x"].double(), v["weight"].double()
    if transposed and planar:
        y = F.conv_transpose3d(x, w, None, (1, 2, 2), (0, 1, 1), (0, 1, 1))
    elif transposed:
        y = F.conv_transpose3d(x, w, None, 2, 1, 1)
    elif planar:
        khh = kh or k
        y = F.conv3d(x, w, None, (1, s, s), (0, dil * (khh - 1) // 2, pad), (1, dil, dil))
    else:
        y = F.conv3d(x, w, None, s, pad, dil)
    if case.planes:
        p = v["planes"].double()
        idx = torch.ones(y.shape[2], dtype=torch.long)
        idx[0], idx[-1] = 0, 2
        y = y + p[:, :, idx]
    if "scale" in v:
        y = y * v["scale"].double().view(1, -1, 1, 1, 1) + v["bias"].double().view(1, -1, 1, 1, 1)
    if case.flags & PRE:
        y = y + v["residual"].double()
    if case.flags & RELU:
        y = torch.relu(y)
    if case.flags & SIGMOID:
        y = torch.sigmoid(y)
    if case.flags & POST:
        y = y + v["residual"].double()
    if case.flags & POOL:
        n, c, d, h, ww = y.shape
        y = y.view(n, c, d // 4, 4, h, ww).mean(3)
    y_head = None
    if "head_w" in v:
        y_head = (y * v["head_w"].double().view(1, -1, 1, 1, 1)).sum(1, keepdim=True)
    return y, y_head
