"""Host side of the hourglass's duplicate tiles (include/snvc_hgdedup.h): the header against the binding against the library's
exports; the closed form of the representative (``snvc_hgdedup_tiles``) and the remap (``snvc_hgdedup_depth``) walked against the
predicate (``snvc_hgdedup_tile_pure``) and against a brute-force walk of the VOXEL rule in numpy for every (od, ow) of each shape;
the refusals' messages; and the rule itself against float64 torch on the oracle's cost volume.  No GPU.

The voxel rule (tests/test_wedge_dedup_host.py's: v2 = conv2's result does not depend on d at voxel (d, w)):
    d - 1 >= 1,   d + 1 <= D - 2,   w + 1 < W - 1,   q (w + 1) - (d - 1) - m0 + off < 0        (off = 4)
Tile (od0, ow0) of the stride-2 result on the 2 x 4 x 32 tiling reads planes 2 od0 - 1 .. 2 od0 + 3 and columns 2 ow0 - 1 .. 2 ow0 + 63
of v2 (plane or column -1 is padding: zero for every d) and is pure when every voxel of that image inside the tensor is marked and
none of its planes lies behind the tensor.

How tight the rule is.  The voxel rule carries sheared_geometry's off = 4: the right half first reaches conv2's neighbourhood of
(d, w) at q (w + 2) >= (d - 2) + m0, i.e. two planes in front of the first marked plane at q = 2 and three at q = 1 (measured here in
float64 and asserted: ONE plane in front of the first marked voxel the values are still equal, at that distance they differ).  At
tile level that slack is less than one tile step -- a step of 2 output planes is 4 planes of v2 -- so the tile in front of a column's
representative differs from it wherever the representative is set by the wedge and not by od0 >= 2.  Both are asserted.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_wedge_dedup_host import OFF, conv2_float64, marked_voxels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_hgdedup.h")
ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = 1, 2                          # include/snvc_hip.h
# (q, m0, D, W): cfg2; the GPU test's four; m0 != 0 at q 1 and q 2; odd D and W; more columns than the walk leaves out
SHAPES = [(2, 0, 192, 312), (1, 0, 96, 72), (2, 0, 148, 72), (1, 0, 160, 132), (1, 0, 10, 40), (1, 60, 40, 72), (2, 5, 80, 72),
          (2, 37, 121, 75), (1, 100, 200, 72), (1, 0, 400, 400)]


@pytest.fixture(scope="module")
def L():
    from snvc_amd import _hgdedup, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _hgdedup.lib()


def test_header_binding_and_exports_agree():
    """What is this header's own; names, parameters, exports and the ABI numbers are held by tests/test_abi_tables_host.py."""
    text = open(HEADER).read()
    # both forwards take snvc_alias_f16x3_conv3d_forward's arguments
    norm = lambda s: re.sub(r"\s+", " ", s).replace("in_desc", "in_alias").strip()  # noqa: E731
    alias = re.search(r"snvc_alias_f16x3_conv3d_forward\s*\(([^)]*)\)", open(os.path.join(ROOT, "include", "snvc_alias.h")).read()).group(1)
    for name in ("snvc_hgdedup_f16x3_conv3d_forward", "snvc_hgdedup_reader_f16x3_conv3d_forward"):
        assert norm(re.search(rf"{name}\s*\(([^)]*)\)", text).group(1)) == norm(alias), name


def out_dims(d_dim, w_dim):
    return (d_dim - 1) // 2 + 1, (w_dim - 1) // 2 + 1


def brute_force_pure(q, m0, d_dim, w_dim):
    """[tiles_d, tiles_w] bool from the VOXEL rule alone: every voxel of the tile's 5 x 65 (d, w) image is marked or is padding in
    front of the tensor (plane / column -1), and no plane of the image lies behind the tensor."""
    od, ow = out_dims(d_dim, w_dim)
    tiles_d, tiles_w = (od + 1) // 2, (ow + 31) // 32
    m = marked_voxels(q, m0, d_dim, w_dim)
    pure = np.zeros((tiles_d, tiles_w), dtype=bool)
    for td in range(tiles_d):
        for tw in range(tiles_w):
            ds, ws = np.arange(4 * td - 1, 4 * td + 4), np.arange(64 * tw - 1, 64 * tw + 64)
            if ds[-1] >= d_dim or ws[-1] >= w_dim:
                continue
            pure[td, tw] = m[np.ix_(ds[ds >= 0], ws[ws >= 0])].all() and ds[0] >= 0      # plane -1 is not d-invariant with plane 3: d0 >= 1 anyway
    return pure


@pytest.mark.parametrize("q,m0,d,w", SHAPES)
def test_closed_form_and_remap_against_the_predicate_and_the_voxel_rule(L, q, m0, d, w):
    from snvc_amd import ops
    desc = ops.wedge_desc(d, w, q, m0, OFF)
    od, ow = out_dims(d, w)
    tiles_d, tiles_w = (od + 1) // 2, (ow + 31) // 32
    pure = np.array([[ops.hg_tile_pure(desc, 2 * td, 32 * tw) for tw in range(tiles_w)] for td in range(tiles_d)])
    assert np.array_equal(pure, brute_force_pure(q, m0, d, w))        # the predicate is the voxel rule on the tile's image
    dups, first, last = ops.hg_dedup_tiles(desc)
    want_remap = np.repeat(np.arange(od)[:, None], ow, axis=1)
    want_dups = 0
    for tw in range(tiles_w):
        tds = np.flatnonzero(pure[:, tw])
        if len(tds) >= 2:
            assert np.array_equal(tds, np.arange(tds[0], tds[-1] + 1))      # consecutive
            assert (first[tw], last[tw]) == (int(tds[0]), int(tds[-1]))
            want_dups += len(tds) - 1
            for o in range(2 * (tds[0] + 1), 2 * tds[-1] + 2):
                want_remap[o, 32 * tw:32 * tw + 32] = 2 * tds[0] + (o & 1)
        else:
            assert (first[tw], last[tw]) == (-1, -1)
    assert dups == want_dups
    got = np.array([[ops.hg_alias_depth(desc, o, x) for x in range(ow)] for o in range(od)])
    assert np.array_equal(got, want_remap)
    assert int((want_remap != np.arange(od)[:, None]).sum()) == sum(2 * (l - f) * min(32, ow - 32 * tw) for tw, (f, l) in enumerate(zip(first, last)) if f >= 0)
    cols = sum(f >= 0 for f in first)
    assert cols == ops.hg_dedup_columns(d, w, q, m0, OFF)
    if (d, w) == (192, 312):          # cfg2: od0 = 70 .. 92 of tile column 0 are duplicates of od0 = 68: 12 of 48 depth tiles
        assert dups == 12 and (first[0], last[0]) == (34, 46) and cols == 1 and got[93, 31] == 69 and got[93, 32] == 93
    if (d, w) == (400, 400):
        assert cols == 5 > ops.hg_dedup_max_columns() == 4
    if (d, w) == (10, 40):
        assert dups == 0


@pytest.mark.parametrize("q,m0,d,w", SHAPES)
@pytest.mark.parametrize("tiles_h", [1, 3])
def test_live_walk_visits_every_tile_but_the_duplicates_once_in_raster_order(L, q, m0, d, w, tiles_h):
    """The walk of the stride-2 launch, by the function the kernel decodes a job with: exactly the tiles that are no duplicates, each
    once, in the plain launch's (td, th, tw) order, all inside the tile grid."""
    from snvc_amd import ops
    desc = ops.wedge_desc(d, w, q, m0, OFF)
    od, ow = out_dims(d, w)
    tiles_d, tiles_w = (od + 1) // 2, (ow + 31) // 32
    dups, first, last = ops.hg_dedup_tiles(desc)
    cols = sum(f >= 0 for f in first)
    got = ops.hg_live_tiles(desc, tiles_h)
    if dups == 0 or cols > ops.hg_dedup_max_columns():
        assert got == []
        return
    want = [(td, th, tw) for td in range(tiles_d) for th in range(tiles_h) for tw in range(tiles_w)
            if not (first[tw] >= 0 and first[tw] < td <= last[tw])]
    assert got == want and len(got) == tiles_d * tiles_h * tiles_w - dups * tiles_h
    assert L.snvc_hgdedup_live_tile(ctypes.byref(desc), 0, 0, None, None, None) == -1


def test_queries_check_their_arguments(L):
    from snvc_amd import _alias
    from snvc_amd._lib import lib
    desc = _alias.WedgeDesc(96, 72, 1, 0, OFF)
    assert L.snvc_hgdedup_depth(ctypes.byref(desc), 41, 3) == 36 + 1 and L.snvc_hgdedup_depth(ctypes.byref(desc), 41, 32) == 41
    assert L.snvc_hgdedup_depth(None, 0, 0) == -1
    assert L.snvc_hgdedup_depth(ctypes.byref(desc), 48, 0) == -1 and b"inside the stride-2 result" in lib().snvc_last_error_string()
    assert L.snvc_hgdedup_depth(ctypes.byref(desc), 0, 36) == -1 and L.snvc_hgdedup_depth(ctypes.byref(desc), -1, 0) == -1
    assert L.snvc_hgdedup_depth(ctypes.byref(_alias.WedgeDesc(96, 72, 3, 0, OFF)), 0, 0) == -1
    assert L.snvc_hgdedup_tile_pure(ctypes.byref(desc), 3, 0) == -1 and b"od0 % 2 == 0, ow0 % 32 == 0" in lib().snvc_last_error_string()
    assert L.snvc_hgdedup_tile_pure(ctypes.byref(desc), 2, 16) == -1 and L.snvc_hgdedup_tile_pure(None, 0, 0) == -1
    assert L.snvc_hgdedup_tile_pure(ctypes.byref(desc), 40, 0) == 1 and L.snvc_hgdedup_tile_pure(ctypes.byref(desc), 40, 32) == 0
    buf = (ctypes.c_int64 * 2)()
    assert L.snvc_hgdedup_tiles(None, buf, buf, 2) == -1 and b"max_tw entries to write" in lib().snvc_last_error_string()
    assert L.snvc_hgdedup_tiles(ctypes.byref(desc), None, None, 2) == -1
    assert L.snvc_hgdedup_tiles(ctypes.byref(desc), None, None, 0) == 4       # the count alone
    assert L.snvc_hgdedup_tiles(ctypes.byref(desc), buf, buf, 1) == 4 and buf[0] == 22


def test_forwards_refuse_what_they_are_not_built_for_before_anything_is_launched(L):
    """The refusals that need no device: a null descriptor, and a layer whose plan is not the form's (the message names the form; no
    pointer is read, nothing is launched -- the operands here are null).  A GPU run of the same refusals with real operands:
    tests/test_gpu_hourglass_dedup.py."""
    from snvc_amd import _alias, _lib
    from snvc_amd._lib import lib
    desc = _alias.WedgeDesc(96, 72, 1, 0, OFF)
    d = _lib.Conv3dDesc()
    d.N, d.Cin, d.Cout, d.Din, d.Hin, d.Win = 1, 32, 64, 96, 8, 72
    d.ksize, d.stride, d.pad, d.dilation, d.transposed = 3, 2, 1, 1, 0
    d.Dout, d.Hout, d.Wout = 48, 4, 36
    null = ctypes.c_void_p(0)
    one = ctypes.c_void_p(256)       # never read: every refusal below comes first
    args = (one, one, one, null, null, one, one, null)
    for fn, word in ((L.snvc_hgdedup_f16x3_conv3d_forward, b"null in_alias"), (L.snvc_hgdedup_reader_f16x3_conv3d_forward, b"null in_desc")):
        assert fn(ctypes.byref(d), *args, None, null) == ERR_INVALID_ARGUMENT and word in lib().snvc_last_error_string()
    d.algo = 0                       # the stride-2 layer off its persistent form
    assert L.snvc_hgdedup_f16x3_conv3d_forward(ctypes.byref(d), *args, ctypes.byref(desc), null) == ERR_UNSUPPORTED
    assert b"snvc_hgdedup_f16x3_conv3d_forward: built for the stride-2 3x3x3 layer on the 16x16x32 form" in lib().snvc_last_error_string()
    d.algo = _lib.ALGO_X3_Q16        # a stride-2 layer is not the reader's
    assert L.snvc_hgdedup_reader_f16x3_conv3d_forward(ctypes.byref(d), *args, ctypes.byref(desc), null) == ERR_UNSUPPORTED
    assert b"snvc_hgdedup_reader_f16x3_conv3d_forward: built for the stride-1 3x3x3 layer on the 16x16x32 form" in lib().snvc_last_error_string()
    other = _alias.WedgeDesc(100, 72, 1, 0, OFF)                      # a descriptor of another tensor
    assert L.snvc_hgdedup_f16x3_conv3d_forward(ctypes.byref(d), *args, ctypes.byref(other), null) == ERR_INVALID_ARGUMENT
    assert b"in_alias describes a [Din][.][Win] tensor" in lib().snvc_last_error_string()
    wide = _alias.WedgeDesc(400, 400, 1, 0, OFF)                      # five columns with duplicates
    d.Din, d.Win, d.Dout, d.Wout = 400, 400, 200, 200
    assert L.snvc_hgdedup_f16x3_conv3d_forward(ctypes.byref(d), *args, ctypes.byref(wide), null) == ERR_UNSUPPORTED
    assert b"more tile columns with duplicates than the live walk has runs" in lib().snvc_last_error_string()
    s1 = _lib.Conv3dDesc()           # the stride-1 layer behind it: the descriptor must be the one of the tensor in front of the stride-2 layer
    s1.N, s1.Cin, s1.Cout, s1.Din, s1.Hin, s1.Win, s1.Dout, s1.Hout, s1.Wout = 1, 64, 64, 48, 4, 36, 48, 4, 36
    s1.ksize, s1.stride, s1.pad, s1.dilation, s1.algo = 3, 1, 1, 1, _lib.ALGO_X3_Q16
    assert L.snvc_hgdedup_reader_f16x3_conv3d_forward(ctypes.byref(s1), *args, ctypes.byref(other), null) == ERR_INVALID_ARGUMENT
    assert b"in_desc describes the [2 Din][.][2 Win] tensor in front of the stride-2 layer" in lib().snvc_last_error_string()
    s1.algo = 0
    assert L.snvc_hgdedup_reader_f16x3_conv3d_forward(ctypes.byref(s1), *args, ctypes.byref(desc), null) == ERR_UNSUPPORTED
    assert b"snvc_hgdedup_reader_f16x3_conv3d_forward: built for the stride-1" in lib().snvc_last_error_string()


@pytest.mark.parametrize("q,m0,d,w", [(1, 0, 40, 24), (2, 7, 40, 24), (1, 60, 40, 72), (2, 5, 150, 72)])
def test_marked_voxels_and_pure_tiles_hold_their_representative_s_values_in_float64(L, q, m0, d, w):
    """v2 in float64 (conv1 -> affine -> ReLU -> conv2 on the oracle's volume): every voxel the voxel rule marks equals its column's
    first marked one; one plane in front of it the value is still the same and `back` planes in front it is not (the module's text).
    Then the stride-2 layer on v2, float64: every pure tile's 2 x H x 32 block equals the representative's, the tile in front of a
    wedge-bound representative does not, and the result gathered through the remap from a tensor whose duplicate rows hold NaN is the
    result."""
    from snvc_amd import ops
    h, back = 6, (2 if q == 2 else 3)
    y = conv2_float64(q, m0, d, h, w)                                  # [C, D, H, W]
    m = marked_voxels(q, m0, d, w)
    compared = differing = same_one_back = 0
    for col in range(w):
        ds = np.flatnonzero(m[:, col])
        if len(ds) == 0:
            continue
        for dd in ds[1:]:
            assert torch.equal(y[:, dd, :, col], y[:, ds[0], :, col]), (dd, col)
            compared += 1
        if ds[0] >= 5:
            same_one_back += int(torch.equal(y[:, ds[0] - 1, :, col], y[:, ds[0], :, col]))
            differing += int(not torch.equal(y[:, ds[0] - back, :, col], y[:, ds[0], :, col]))
    assert compared >= 200 and differing > 0 and same_one_back > 0
    w3 = torch.randn(8, y.size(0), 3, 3, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 0.1
    o = torch.nn.functional.conv3d(y[None], w3, stride=2, padding=1)[0]       # [8, OD, OH, OW]
    desc = ops.wedge_desc(d, w, q, m0, OFF)
    dups, first, last = ops.hg_dedup_tiles(desc)
    if w == 24:
        assert dups == 0                                               # no 65-column image fits: the voxel checks above are the test
        return
    assert dups > 0
    od, ow = out_dims(d, w)
    tight = 0
    for tw, (f, l) in enumerate(zip(first, last)):
        if f < 0:
            continue
        cols = slice(32 * tw, 32 * tw + 32)
        rep = o[:, 2 * f:2 * f + 2, :, cols]
        assert rep.abs().max() > 0
        for td in range(f + 1, l + 1):
            assert torch.equal(o[:, 2 * td:2 * td + 2, :, cols], rep), (tw, td)
        if f > 1:                                                      # the representative is set by the wedge, not by od0 >= 2
            assert not torch.equal(o[:, 2 * f - 2:2 * f, :, cols], rep), (tw, f)
            tight += 1
    assert tight > 0
    remap = torch.tensor([[ops.hg_alias_depth(desc, a, b) for b in range(ow)] for a in range(od)])
    dup = remap != torch.arange(od)[:, None]
    assert int(dup.sum()) > 0
    poisoned = torch.where(dup[None, :, None, :], torch.full_like(o, float("nan")), o)
    assert torch.equal(torch.gather(poisoned, 1, remap[None, :, None, :].expand_as(o)), o)
