"""CPU checks of the device read-out's host side (include/snvc_decode.h, snvc_amd/_decode.py, snvc_amd.decode.refine_boxes /
grid_bev_flat / to_update_dict) and of the cases tests/test_gpu_decode.py runs (tests/decode_cases.py): with the host route
alone, each case keeps and rejects what it is built to, and no kept instance sits where a last-bit difference of the device's
sin / cos / atan2 could show as more than a last-bit difference of the box (the yaw's branch cut, a degenerate fit).

A case of one instance cannot both keep and reject: "n1" is a kept instance, every other case has both kinds.
"""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import decode_cases as C
from test_decode import decode_case
from snvc_amd import _decode
from snvc_amd import decode as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_decode.h")


# ---------------------------------------------------------------------------------------------------- the binding
def test_header_and_binding_agree():
    """The mirrored constants and struct; names, parameters and the ABI number are held by tests/test_abi_tables_host.py."""
    text = open(HEADER).read()
    for name, value in (("SNVC_DECODE_GRID", _decode.GRID), ("SNVC_DECODE_COORDS_F32", _decode.COORDS_F32),
                        ("SNVC_DECODE_COORDS_F64", _decode.COORDS_F64)):
        assert int(re.search(rf"{name} = (\d+)", text).group(1)) == value
    assert ctypes.sizeof(_decode.DecodeConfig) == 48


def test_workspace_bytes():
    L = _decode.lib()
    for parts in (1, 9):
        assert L.snvc_decode_workspace_bytes(0, parts) == 0
        assert L.snvc_decode_workspace_bytes(3, parts) > 0 and L.snvc_decode_workspace_bytes(3, parts) % 8 == 0
        assert L.snvc_decode_workspace_bytes(-1, parts) < 0
    assert L.snvc_decode_workspace_bytes(3, 5) < 0 and L.snvc_decode_workspace_bytes(2 ** 31, 9) < 0


def test_the_c_call_checks_its_arguments_before_any_launch():
    from snvc_amd._lib import lib
    L = _decode.lib()
    cfg = _decode.DecodeConfig()
    cfg.x_range[:], cfg.z_range[:], cfg.min_val, cfg.max_val = [-1.6, 1.6], [-2.4, 2.4], -1.0, 2.0
    call = lambda c, n, parts, m: L.snvc_decode_boxes(c, None, None, None, n, parts, m, *([None] * 7))  # noqa: E731
    ref = ctypes.byref(cfg)
    assert call(None, 1, 9, 35) == 1
    assert call(ref, 0, 9, 35) == 0                                     # N = 0: nothing to do
    assert call(ref, 1, 9, 35) == 1 and b"null pointer" in lib().snvc_last_error_string()
    assert call(ref, 1, 5, 35) == 1 and b"1 or 9" in lib().snvc_last_error_string()
    assert call(ref, 1, 9, 0) == 1 and b"empty sequence" in lib().snvc_last_error_string()
    assert call(ref, -1, 9, 35) == 1
    cfg.source = 3
    assert call(ref, 1, 9, 35) == 1 and b"source" in lib().snvc_last_error_string()


def test_refine_boxes_refuses_what_cannot_run_in_the_kernel():
    c = C.case("m35")
    with pytest.raises(TypeError, match="Filter"):
        D.refine_boxes(c["cfg"], torch.from_numpy(c["ncf"]), c["samples"], c["grid"], filter_3d=object())
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        D.refine_boxes(c["cfg"], torch.from_numpy(c["ncf"]), c["samples"], c["grid"])
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        D.refine_boxes(c["cfg"], c["ncf"], c["samples"], c["grid"])


# ---------------------------------------------------------------------------------------------------- the grid
def test_grid_bev_flat_is_the_datasets():
    cfg = types.SimpleNamespace(x_range=(-1.5, 1.7), y_range=(-0.9, 1.1), z_range=(-2.3, 2.6), grid_resolution=(3, 5, 7))
    # refinementDataset._init_3d_grid, KITTIRefinement_dataset.py:271-281
    x_pts = np.linspace(cfg.x_range[0], cfg.x_range[1], cfg.grid_resolution[1])
    y_pts = np.linspace(cfg.y_range[0], cfg.y_range[1], cfg.grid_resolution[0])
    z_pts = np.linspace(cfg.z_range[0], cfg.z_range[1], cfg.grid_resolution[2])
    gx, gy, gz = np.meshgrid(x_pts, y_pts, z_pts, indexing="xy")
    grid_3d = np.concatenate([gx[None, :], gy[None, :], gz[None, :]])
    want = np.transpose(grid_3d.copy()[:, 0, :, :].squeeze(), (2, 1, 0)).reshape(-1, 3)
    got = D.grid_bev_flat(cfg)
    assert got.dtype == np.float64 and got.shape == (35, 3) and np.array_equal(got, want)
    assert np.array_equal(got[2 * 5 + 3], [x_pts[3], y_pts[0], z_pts[2]])


# ---------------------------------------------------------------------------------------------------- the dict
@pytest.mark.parametrize("parts", [9, 1])
def test_to_update_dict_has_the_references_list_semantics(parts):
    r = np.random.default_rng(parts)
    one, both = r.standard_normal((3, 7)), r.standard_normal((3, 7))
    conf = r.uniform(0, 1, (3, parts)).astype(np.float32)
    conf[1, 0] = np.nan
    keep = np.array([True, False, True])
    result = {"one_part": torch.from_numpy(one), "all_parts": torch.from_numpy(both) if parts > 1 else None,
              "confidence": torch.from_numpy(conf), "index": torch.zeros((3, parts), dtype=torch.int64), "keep_flags": torch.from_numpy(keep)}
    got = D.to_update_dict(result)
    assert set(got) == {"pred", "confidence", "keep_flags"}
    assert got["keep_flags"].dtype == np.bool_ and np.array_equal(got["keep_flags"], keep)
    assert got["confidence"].dtype == np.float32 and np.array_equal(got["confidence"], conf, equal_nan=True)
    if parts > 1:
        assert set(got["pred"]) == {"one_part", "all_parts"}
        assert np.array_equal(np.asarray(got["pred"]["one_part"]), one[[0, 2]])       # a rejected instance is absent here
        assert np.array_equal(np.asarray(got["pred"]["all_parts"]), both)             # and present, as its proposal, here
    else:
        assert set(got["pred"]) == {"one_part"}
        assert np.array_equal(np.asarray(got["pred"]["one_part"]), one)
    assert all(isinstance(b, np.ndarray) and b.shape == (7,) and b.dtype == np.float64 for v in got["pred"].values() for b in v)


def test_to_update_dict_feeds_the_kitti_writer():
    c = decode_case("argmax")
    host = D.ncf_to_update_2d(c["cfg"], c["ncf"], c["samples"].copy(), c["grid"], D.Filter())
    keep = host["keep_flags"]
    one = c["samples"].copy()
    one[keep] = np.asarray(host["pred"]["one_part"])
    result = {"one_part": torch.from_numpy(one), "all_parts": torch.from_numpy(np.asarray(host["pred"]["all_parts"])),
              "confidence": torch.from_numpy(host["confidence"]), "keep_flags": torch.from_numpy(keep)}
    a, b = {}, {}
    D.update_record(a, host, c["meta"])
    D.update_record(b, D.to_update_dict(result), c["meta"])
    assert a == b and a


# ---------------------------------------------------------------------------------------------------- the cases
def fit_terms(X, Y, W=None):
    """(h00 + h11, h01 - h10) of decode.rigid_transform_2d, the two arguments of its atan2."""
    xm, ym = X - X.mean(axis=1, keepdims=True), Y - Y.mean(axis=1, keepdims=True)
    if W is not None:
        xm = xm * np.asarray(W, dtype=np.float64).reshape(1, -1)
    H = xm @ ym.T
    return H[0, 0] + H[1, 1], H[0, 1] - H[1, 0]


def all_cases():
    return [(n, decode_case(n)) for n in ("argmax", "coordinates", "one_part_only")] + [(n, C.case(n)) for n in C.NAMES]


@pytest.mark.parametrize("name, c", all_cases(), ids=[n for n, _ in all_cases()])
def test_cases_meet_their_conditions(name, c):
    n, parts = c["ncf"].shape[:2]
    co = None if c["coordinates"] is None else c["coordinates"].astype(np.float64)
    host = D.ncf_to_update_2d(c["cfg"], c["ncf"], c["samples"].copy(), c["grid"], D.Filter(), coordinates=co)
    keep = host["keep_flags"]
    if "expect_keep" in c:
        assert np.array_equal(keep, c["expect_keep"])
    assert keep.any() and (n == 1 or not keep.all())
    if parts == 1:
        return
    boxes = np.asarray(host["pred"]["all_parts"])
    assert np.array_equal(boxes[~keep], c["samples"][~keep])
    flat = c["ncf"].reshape(n, parts, -1)
    for i in np.flatnonzero(keep):
        s = c["samples"][i]
        assert abs(boxes[i, 6]) <= np.pi - 1e-6, f"instance {i}: the yaw {boxes[i, 6]!r} is at the branch cut"
        # the two fits of register_BEV, from the definitions in decode.py
        if co is not None:
            off = np.stack([c["cfg"].x_range[0] + co[i, :, 0] * (c["cfg"].x_range[1] - c["cfg"].x_range[0]), np.zeros(parts),
                            c["cfg"].z_range[0] + co[i, :, 1] * (c["cfg"].z_range[1] - c["cfg"].z_range[0])], axis=1)
        else:
            off = c["grid"][flat[i].argmax(axis=1)] * np.array([1.0, 0.0, 1.0])
        dst = np.array([s[3], s[4] - 0.5 * s[0], s[5]])[None, :] + off @ (D.rotation_y(s[6]) @ D._OBJECT_AXES.T).T
        src = D.get_cam_cord(s)[[0, 2], :]
        a, b = fit_terms(src, dst[:, [0, 2]].T, host["confidence"][i])
        assert abs(a) + abs(b) >= 1e-6, f"instance {i}: the part fit is degenerate"
        R, T = D.rigid_transform_2d(src, dst[:, [0, 2]].T, host["confidence"][i])
        a, b = fit_terms(D.get_canonical(s[1], s[2]), R @ src + T)
        assert abs(a) + abs(b) >= 1e-6, f"instance {i}: the canonical fit is degenerate"


def test_cases_have_the_shapes_and_values_they_are_there_for():
    shapes = {n: C.case(n)["ncf"].shape for n in C.NAMES}
    assert shapes["m35"][2:] == (7, 5) and shapes["m1_coords"][2:] == (1, 1) and shapes["m1247_ties"][2:] == (43, 29)
    assert shapes["n1"][0] == 1 and shapes["n300"] == (300, 9, 7, 5) and shapes["p1"][1] == 1
    assert 43 * 29 == 1247 and 1247 // 4 > 256 and 1247 % 4 == 3
    assert C.case("coords_f32")["coordinates"].dtype == np.float32 and C.case("coords_f64")["coordinates"].dtype == np.float64
    ties = C.case("m1247_ties")["ncf"].reshape(3, 9, -1)
    for (i, p), (lo, hi) in C.TIES.items():
        row = ties[i, p]
        assert lo < hi and row[lo] == row[hi] == row.max() and (row == row.max()).sum() == 2 and row.argmax() == lo
    assert {(41 // 4) // 64, (1043 // 4) % 256 // 64} == {0} and {(1002 // 4) // 64, (800 // 4) // 64} == {3}
    e = C.case("edges")
    flat = e["ncf"].reshape(7, 9, -1)
    assert flat[0].max() == 2.0 and flat[0].min() == -1.0
    assert flat[1].max() > 2.0 and np.nextafter(flat[1].max(), np.float32(0)) == 2.0
    assert flat[2].min() < -1.0 and np.nextafter(flat[2].min(), np.float32(0)) == -1.0
    assert np.isposinf(flat[3]).sum() == 1 and np.isneginf(flat[4]).sum() == 1
    i, p, cells = C.NAN_AT
    assert np.flatnonzero(np.isnan(flat[i, p])).tolist() == list(cells) and np.isnan(flat).sum() == 2
    host = D.ncf_to_update_2d(e["cfg"], e["ncf"], e["samples"].copy(), e["grid"], D.Filter())
    assert np.isnan(host["confidence"][i, p]) and flat[i, p].argmax() == cells[0]
    assert not flat[6, 5].any() and flat[6, [0, 1, 2, 3, 4, 6, 7, 8]].any(axis=1).all() and host["confidence"][6, 5] == 0.0
