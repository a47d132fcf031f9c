"""Host side of the aliased wedge duplicates (include/snvc_alias.h): the header against the binding against the library's exports,
the remap ``snvc_alias_depth`` against a brute-force walk of the tile rule in numpy -- for every (d, w) of each shape the first pure
tile of the voxel's tile column, the identity outside duplicates -- and the remap against float64 torch on the oracle's cost volume:
conv2's result gathered through the remap IS conv2's result, and the stride-2 layer behind it gives the same values on a tensor
whose duplicate rows were overwritten with NaN and read through the remap.  No GPU.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_wedge_dedup_host import OFF, brute_force_tiles, conv2_float64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_alias.h")
# cfg2; one column; m0 != 0 with duplicates in two columns of different length; half-pixel planes; a shape with none
SHAPES = [(2, 0, 192, 312), (1, 0, 96, 72), (1, 0, 96, 40), (1, 60, 40, 72), (2, 5, 80, 72), (2, 0, 148, 72), (1, 0, 10, 40)]


@pytest.fixture(scope="module")
def L():
    from snvc_amd import _alias, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _alias.lib()


def test_header_binding_and_exports_agree():
    """What is this header's own; names, parameters, exports and the ABI number are held by tests/test_abi_tables_host.py."""
    from snvc_amd import _alias
    text = open(HEADER).read()
    # the aliased forward takes the plain one's arguments, declared in the same words
    norm = lambda s: re.sub(r"\s+", " ", s).strip()  # noqa: E731
    plain = re.search(r"snvc_fused_first_conv3d_forward\s*\(([^)]*)\)", open(os.path.join(ROOT, "include", "snvc_fused.h")).read()).group(1)
    alias = re.search(r"snvc_alias_fused_first_conv3d_forward\s*\(([^)]*)\)", text).group(1)
    assert norm(plain) == norm(alias)
    # the struct's mirror: five int32 in the header's order
    fields = re.search(r"typedef struct snvc_wedge_desc \{(.*?)\} snvc_wedge_desc;", text, re.S).group(1)
    names = [n for line in re.findall(r"int32_t ([^;]*);", fields) for n in re.split(r",\s*", line)]
    assert names == [n for n, _ in _alias.WedgeDesc._fields_] and ctypes.sizeof(_alias.WedgeDesc) == 20


def brute_force_remap(q, m0, d_dim, w_dim):
    """[D, W] int: per voxel the plane that holds its bits, from the brute-force tile walk of tests/test_wedge_dedup_host.py."""
    dups, first, last = brute_force_tiles(q, m0, d_dim, w_dim)
    remap = np.repeat(np.arange(d_dim)[:, None], w_dim, axis=1)
    for tw, (f, l) in enumerate(zip(first, last)):
        if f < 0:
            continue
        for dd in range(4 * (f + 1), 4 * l + 4):
            remap[dd, 32 * tw:32 * tw + 32] = 4 * f + (dd & 3)
    return dups, remap


def library_remap(q, m0, d_dim, w_dim):
    from snvc_amd import ops
    desc = ops.wedge_desc(d_dim, w_dim, q, m0, OFF)
    return np.array([[ops.wedge_alias_depth(desc, d, w) for w in range(w_dim)] for d in range(d_dim)])


@pytest.mark.parametrize("q,m0,d,w", SHAPES)
def test_alias_depth_is_the_first_pure_tile_of_the_column_and_the_identity_elsewhere(L, q, m0, d, w):
    dups, want = brute_force_remap(q, m0, d, w)
    got = library_remap(q, m0, d, w)
    assert np.array_equal(got, want)
    moved = int((want != np.arange(d)[:, None]).sum())
    assert moved == dups * 4 * 32 and (dups > 0 or d == 10)          # every duplicate voxel moves, nothing else does
    if (d, w) == (192, 312):
        assert dups == 40 and got[184, 0] == 72 and got[187, 63] == 139 and got[187, 64] == 187


def test_alias_depth_checks_its_arguments(L):
    from snvc_amd import _alias
    from snvc_amd._lib import lib
    desc = _alias.WedgeDesc(96, 40, 1, 0, OFF)
    assert L.snvc_alias_depth(ctypes.byref(desc), 50, 3) == 40 + 2
    assert L.snvc_alias_depth(None, 0, 0) == -1
    assert L.snvc_alias_depth(ctypes.byref(desc), 96, 0) == -1 and b"inside [0, D) x [0, W)" in lib().snvc_last_error_string()
    assert L.snvc_alias_depth(ctypes.byref(desc), 0, 40) == -1 and L.snvc_alias_depth(ctypes.byref(desc), -1, 0) == -1
    assert L.snvc_alias_depth(ctypes.byref(_alias.WedgeDesc(96, 40, 3, 0, OFF)), 0, 0) == -1


@pytest.mark.parametrize("q,m0,d,w", [(1, 60, 40, 72), (2, 5, 80, 72), (1, 0, 96, 40)])
def test_readers_through_the_remap_see_the_full_tensor_in_float64(L, q, m0, d, w):
    """conv2's float64 result with every duplicate row overwritten by NaN, read through the remap: the tensor itself; and so the
    stride-2 layer behind it gives the same values.  The representative's rows hold values, and planes in front of it hold others:
    the remap is not a map inside a constant region (how tight the rule is: tests/test_wedge_dedup_host.py)."""
    h = 6
    y = conv2_float64(q, m0, d, h, w)                                 # [C, D, H, W]
    dups, remap = brute_force_remap(q, m0, d, w)
    assert dups > 0 and np.array_equal(remap, library_remap(q, m0, d, w))
    dup = torch.from_numpy(remap != np.arange(d)[:, None])            # [D, W]
    poisoned = torch.where(dup[None, :, None, :], torch.full_like(y, float("nan")), y)
    idx = torch.from_numpy(remap)[None, :, None, :].expand_as(y)
    seen = torch.gather(poisoned, 1, idx)                              # what an aliasing reader fetches
    assert torch.equal(seen, y)
    w3 = torch.randn(8, y.size(0), 3, 3, 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 0.1
    assert torch.equal(torch.nn.functional.conv3d(seen[None], w3, stride=2, padding=1), torch.nn.functional.conv3d(y[None], w3, stride=2, padding=1))
    tw = int(np.flatnonzero((remap != np.arange(d)[:, None]).any(axis=0))[0]) // 32
    rep = int(remap[:, 32 * tw][remap[:, 32 * tw] != np.arange(d)].min())
    cols = slice(32 * tw, 32 * tw + 32)
    assert y[:, rep, :, cols].abs().max() > 0 and any(not torch.equal(y[:, dd, :, cols], y[:, rep, :, cols]) for dd in range(rep))
