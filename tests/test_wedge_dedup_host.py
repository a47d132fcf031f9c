"""Host side of the wedge deduplication (include/snvc_dedup.h): the header against the binding against the library's exports, the
tile query against a brute-force walk of the voxel rule in numpy, and the rule itself against float64 torch on the oracle's cost
volume: conv1 -> affine -> ReLU -> conv2 gives the same bits on every voxel the rule marks.  No GPU.

The voxel rule: conv2's output at (d, h, w) does not depend on d when
    2 <= d <= D - 3,   w + 1 < W - 1,   q * (w + 1) - (d - 1) - m0 + off < 0        (off = 4, models.submodule.sheared_geometry)
and a 4 x 32 (d, w) tile is pure when each of its voxels is such a voxel and lies inside the tensor.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_dedup.h")
OFF = 4


@pytest.fixture(scope="module")
def L():
    from snvc_amd import _dedup, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _dedup.lib()


def test_header_binding_and_exports_agree():
    """What is this header's own; names, parameters, exports and the ABI number are held by tests/test_abi_tables_host.py."""
    text = open(HEADER).read()
    # the deduplicated forward takes the plain one's arguments, declared in the same words
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    plain = re.search(r"snvc_fused_first_conv3d_forward\s*\(([^)]*)\)", open(os.path.join(ROOT, "include", "snvc_fused.h")).read()).group(1)
    dedup = re.search(r"snvc_dedup_fused_first_conv3d_forward\s*\(([^)]*)\)", text).group(1)
    assert norm(plain) == norm(dedup)


def marked_voxels(q, m0, d_dim, w_dim):
    """[D, W] bool: the voxel rule."""
    d, w = np.arange(d_dim)[:, None], np.arange(w_dim)[None, :]
    return (d >= 2) & (d <= d_dim - 3) & (w + 1 < w_dim - 1) & (q * (w + 1) - (d - 1) - m0 + OFF < 0)


def brute_force_tiles(q, m0, d_dim, w_dim):
    """(duplicates per (n, th), first, last) from the voxel rule alone: a tile is pure when all its 4 x 32 voxels are marked."""
    tiles_d, tiles_w = (d_dim + 3) // 4, (w_dim + 31) // 32
    m = np.zeros((tiles_d * 4, tiles_w * 32), dtype=bool)             # voxels past the tensor are not marked
    m[:d_dim, :w_dim] = marked_voxels(q, m0, d_dim, w_dim)
    pure = m.reshape(tiles_d, 4, tiles_w, 32).all(axis=(1, 3))
    first, last, dups = [], [], 0
    for tw in range(tiles_w):
        tds = np.flatnonzero(pure[:, tw])
        if len(tds) >= 2:
            assert np.array_equal(tds, np.arange(tds[0], tds[-1] + 1))      # consecutive
            first.append(int(tds[0])), last.append(int(tds[-1]))
            dups += len(tds) - 1
        else:
            first.append(-1), last.append(-1)
    return dups, first, last


@pytest.mark.parametrize("q,m0,d,w,want", [(2, 0, 192, 312, 40), (1, 0, 96, 40, None), (1, 60, 40, 72, None), (2, 5, 80, 72, None),
                                           (1, 0, 10, 40, 0)])
def test_tile_query_is_the_brute_force_walk_of_the_voxel_rule(L, q, m0, d, w, want):
    from snvc_amd import ops
    got = ops.fused_first_wedge_tiles(d, w, q, m0, OFF)
    assert got == brute_force_tiles(q, m0, d, w)
    if want is not None:
        assert got[0] == want
    if (d, w) == (192, 312):         # cfg2: 28 + 12 duplicates, d0 = 72 .. 184 and 136 .. 184
        assert got[1][:3] == [18, 34, -1] and got[2][:3] == [46, 46, -1]
    else:
        assert want == 0 or got[0] > 0


def test_tile_query_checks_its_arguments(L):
    from snvc_amd._lib import Conv3dDesc, lib
    d = Conv3dDesc()
    d.Din, d.Win = 96, 40
    buf = (ctypes.c_int64 * 2)()
    assert L.snvc_dedup_fused_first_tiles(ctypes.byref(d), 4, 0, OFF, buf, buf, 2) == -1 and b"q = 1 | 2" in lib().snvc_last_error_string()
    assert L.snvc_dedup_fused_first_tiles(None, 1, 0, OFF, buf, buf, 2) == -1
    assert L.snvc_dedup_fused_first_tiles(ctypes.byref(d), 1, 0, OFF, None, None, 2) == -1
    assert L.snvc_dedup_fused_first_tiles(ctypes.byref(d), 1, 0, OFF, None, None, 0) == 12      # the count alone
    first, last = (ctypes.c_int64 * 1)(), (ctypes.c_int64 * 1)()
    assert L.snvc_dedup_fused_first_tiles(ctypes.byref(d), 1, 0, OFF, first, last, 1) == 12 and (first[0], last[0]) == (10, 22)


def conv2_float64(q, m0, d_dim, h_dim, w_dim, c=4, seed=3):
    """conv2(relu(affine(conv1(cost volume)))) in float64 on torch's CPU kernels, the volume from the C oracle: [2c, D, H, W]."""
    from oracle import native
    g = np.random.default_rng(seed)
    left, right = g.standard_normal((2, 1, c, h_dim, w_dim))
    shift = ((m0 + np.arange(d_dim, dtype=np.float64)) / q)[None]
    vol = torch.from_numpy(native.cost_volume_forward(left, right, shift, 1))
    tg = torch.Generator().manual_seed(seed)
    w1 = torch.randn(2 * c, 2 * c, 3, 3, 3, generator=tg, dtype=torch.float64) * 0.1
    w2 = torch.randn(2 * c, 2 * c, 3, 3, 3, generator=tg, dtype=torch.float64) * 0.1
    sc, bi = torch.rand(2 * c, generator=tg, dtype=torch.float64) + 0.5, torch.randn(2 * c, generator=tg, dtype=torch.float64) * 0.3
    v1 = torch.relu(torch.nn.functional.conv3d(vol, w1, padding=1) * sc.view(1, -1, 1, 1, 1) + bi.view(1, -1, 1, 1, 1))
    return torch.nn.functional.conv3d(v1, w2, padding=1)[0]


@pytest.mark.parametrize("q,m0,d,w", [(1, 0, 40, 24), (2, 0, 40, 24), (2, 7, 40, 24), (1, 5, 40, 24),       # the voxel rule (W 24: no whole tile)
                                      (1, 60, 40, 72), (2, 5, 80, 72), (1, 0, 96, 40)])                      # and shapes with pure tiles
def test_marked_voxels_and_tiles_hold_their_representative_s_bits_in_float64(L, q, m0, d, w):
    """Every voxel the voxel rule marks equals the first marked voxel of its column, and every voxel of every tile the query marks
    equals the representative tile's first depth row: torch.equal in float64.  The rule is conservative (whole tiles need one bound)
    but not loose: the right half first reaches conv2's neighbourhood at q * (w + 2) >= (d - 2) + m0, which is two planes before
    the first marked one at q = 2 and three at q = 1, and there the values differ."""
    from snvc_amd import ops
    h, back = 6, (2 if q == 2 else 3)
    y = conv2_float64(q, m0, d, h, w)
    m = marked_voxels(q, m0, d, w)
    compared = differing = 0
    for col in range(w):
        ds = np.flatnonzero(m[:, col])
        if len(ds) == 0:
            continue
        for dd in ds[1:]:
            assert torch.equal(y[:, dd, :, col], y[:, ds[0], :, col]), (dd, col)
            compared += 1
        if ds[0] >= 5:
            differing += int(not torch.equal(y[:, ds[0] - back, :, col], y[:, ds[0], :, col]))
    assert compared >= 200 and differing > 0
    dups, first, last = ops.fused_first_wedge_tiles(d, w, q, m0, OFF)
    if w == 24:
        assert dups == 0
    else:
        assert dups > 0
    for tw, (f, l) in enumerate(zip(first, last)):
        if f < 0:
            continue
        rep = y[:, 4 * f, :, 32 * tw:32 * tw + 32]
        for dd in range(4 * f, 4 * l + 4):
            assert torch.equal(y[:, dd, :, 32 * tw:32 * tw + 32], rep), (tw, dd)
