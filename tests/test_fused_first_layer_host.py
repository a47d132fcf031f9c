"""Host side of the fused sheared first layer (include/snvc_fused.h): the channel-interleaved layout's index function against a
numpy transpose, the buffer geometry against a brute-force walk of the G indices, and the argument checks that run before any
launch (the header against the binding: tests/test_abi_tables_host.py).  No GPU."""
import ctypes
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from snvc_amd import _fused, _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _fused.lib()


@pytest.mark.parametrize("c", [32, 40, 36])      # 36: the last group of 8 is partial (4 channels; the rest of its piece is never indexed)
@pytest.mark.parametrize("mode", [0, 1])
def test_il_index_is_the_numpy_transpose(L, c, mode):
    """A [3C, H, W] result (class-major oc = cls*C + co | class-minor oc = co*3 + cls) scattered through il_index equals the tensor
    regrouped by numpy: [cls][group][h][lp + x][8], pad columns and the channels past C untouched."""
    from snvc_amd import ops
    h_dim, w, pitch, lp, cls0, classes = 3, 5, 9, 2, 3, 6
    groups = (c + 7) // 8
    y = np.arange(3 * c * h_dim * w, dtype=np.float64).reshape(3 * c, h_dim, w) + 1.0
    flat = np.zeros(classes * groups * h_dim * pitch * 8)
    for oc in range(3 * c):
        for h in range(h_dim):
            for x in range(w):
                i = ops.il_index(mode, oc, c, h_dim, pitch, lp, cls0, h, x)
                assert 0 <= i < flat.size and flat[i] == 0.0          # inside the buffer, and no two elements share a slot
                flat[i] = y[oc, h, x]
    by_class = y.reshape(3, c, h_dim, w) if mode == 0 else y.reshape(c, 3, h_dim, w).transpose(1, 0, 2, 3)      # [cls][co][h][x]
    padded = np.zeros((3, groups * 8, h_dim, w))
    padded[:, :c] = by_class
    want = np.zeros((classes, groups, h_dim, pitch, 8))
    want[cls0:cls0 + 3, :, :, lp:lp + w] = padded.reshape(3, groups, 8, h_dim, w).transpose(0, 1, 3, 4, 2)
    assert np.array_equal(flat.reshape(want.shape), want)


def test_il_index_refuses_what_lies_outside(L):
    from snvc_amd import ops
    assert ops.il_index(0, 96, 32, 3, 9, 2, 0, 0, 0) == -1            # oc == 3C
    assert ops.il_index(1, 0, 32, 3, 9, 2, 0, 3, 0) == -1             # h == H
    assert ops.il_index(0, 0, 32, 3, 9, 2, 0, 0, 7) == -1             # lp + x == pitch
    assert ops.il_index(2, 0, 32, 3, 9, 2, 0, 0, 0) == -1


@pytest.mark.parametrize("q,m0,d,w", [(1, 0, 10, 40), (2, 0, 10, 40), (1, 3, 10, 40), (2, 5, 192, 311), (1, 0, 40, 8), (2, 0, 4, 1)])
def test_geometry_covers_every_index(q, m0, d, w):
    """pitch / lp hold every G index of a voxel of the tensor, every G' index of the last column, and both layers' own columns."""
    from snvc_amd import ops
    from snvc_amd.models.submodule import sheared_geometry
    off, wu, off_col, wu_col = sheared_geometry(q, m0, d, w)
    pitch, lp = ops.fused_il_geometry(q, m0, d, w, wu, off, wu_col, off_col)
    idx = [q * ww - dd - m0 + off for ww in range(w - 1) for dd in (0, d - 1)]
    idx += [q * (w - 1) - dd - m0 + off_col for dd in (0, d - 1)] + [0, wu - 1, wu_col - 1]
    assert lp + min(idx) >= 0 and lp + max(idx) < pitch
    assert pitch == max(idx) - min(idx) + 1                           # and nothing more


def test_the_c_calls_check_their_arguments_before_any_launch(L):
    from snvc_amd._lib import Conv3dDesc, lib
    err = lambda: lib().snvc_last_error_string()  # noqa: E731
    d = Conv3dDesc()
    d.N, d.Cin, d.Din, d.Hin, d.Win = 1, 32, 10, 6, 40
    d.Cout, d.Dout, d.Hout, d.Wout = 32, 10, 6, 40
    d.ksize, d.stride, d.dilation, d.pad = 3, 1, 1, 1
    d.algo = 0x8000
    one = 64        # a non-null, aligned stand-in: the checks below come before any pointer is read
    call = lambda q, pitch, lp, gi=one: L.snvc_fused_first_conv3d_forward(  # noqa: E731
        ctypes.byref(d), one, None, None, one, one, None, None, 1.0, None, gi, pitch, lp, one, one, one, q, 0, 4, 50, 1, None)
    assert call(1, 64, 8, None) == 1 and b"null pointer" in err()
    assert call(4, 64, 8) == 2 and b"q = 1 | 2" in err()
    assert call(1, 64, 2) == 1 and b"do not cover" in err()           # the first plane's index -9 + 4 needs lp >= 5
    assert call(1, 40, 8) == 1 and b"do not cover" in err()           # 39 + 50 + 8 >= 40
    assert L.snvc_fused_sheared_prep_x3(one, 1, 32, 6, 40, 1, 48, 4, 24, 50, one, one, 96, 1.0, 1.0, one, one, one, one, one, one, None, 64, 8,
                                        None) == 1 and b"gi is NULL" in err()
