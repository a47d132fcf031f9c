"""CPU checks of the RoI cropper's specification as tests/roi_crop_ref.py restates it (DESIGN.md "RoI crops",
include/snvc_roicrop.h), of the cases the GPU test runs (tests/roi_crop_cases.py), and of the host side of
snvc_amd.geometry.RoICropper.

Tolerances.  Golden geometry: tests/golden/make_golden_roi_crop.py measured 2.274e-13 as the largest gap between the closed
form of `trans` and a float64 linear solve on the same float32 points (SOLVE_GAP); 16 times that is allowed for the solver's
rounding noise, and the allowance must stay below 1e-9 (2.6e-4 of a 1/1024 coordinate quantum at 256 px).  Key points: the
restatement repeats the reference's numpy operations, so they are equal; 1e-12 is allowed for a BLAS that sums in another order.
Hand answers are exact.  fixed5 against exact: |fixed5 - exact| <= 0.5 + 2 (1/64 + 2/1024) G, G the largest difference of
adjacent pixels, the zero border included: the 1/32 px coordinate grid moves a tap by at most 1/64 px, and the two roundings to
1/1024 add 2/1024, per axis; 0.5 is the final rounding.  (Measured while writing: 5 of the allowed 9.46 on the noise images.)
"""
import os
import re
import types

import numpy as np
import pytest
import torch

import roi_crop_cases as C
import roi_crop_ref as R
from snvc_amd import _roicrop
from snvc_amd.geometry import RoICropper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_roicrop.h")
GOLD = C.load_golden()
SOLVE_GAP = 2.274e-13
TRANS_TOL = 16 * SOLVE_GAP
KPTS_TOL = 1e-12


def sides(c, n):
    f = C.frame_of(c, n)
    return (("l", c["left"][f], c["P_left"][f]), ("r", c["right"][f], c["P_right"][f]))


# ---------------------------------------------------------------------------------------------------- golden geometry
@pytest.mark.parametrize("name", C.NAMES)
def test_geometry_matches_the_reference(name):
    assert TRANS_TOL < 1e-9
    c = C.case(name)
    worst = {"kpts": 0.0, "trans": 0.0, "local": 0.0}
    for n, s in enumerate(c["samples"]):
        for side, _, P in sides(c, n):
            kpts, trans, local = R.geometry(s, P, c["cfg"].grid_range, c["cfg"].aspect_ratio, c["cfg"].resolution)
            assert local.dtype == np.float32 and local.shape == (9, 2) and trans.shape == (2, 3) and kpts.shape == (9, 2)
            worst["kpts"] = max(worst["kpts"], np.abs(kpts - GOLD[f"{name}/kpts_{side}"][n]).max())
            worst["trans"] = max(worst["trans"], np.abs(trans - GOLD[f"{name}/trans_{side}"][n]).max())
            want = GOLD[f"{name}/local_{side}"][n]
            worst["local"] = max(worst["local"], (np.abs(local - want) / np.spacing(np.abs(want))).max())
    print(f"{name}: max |kpts - golden| {worst['kpts']:.3g}, |trans - golden| {worst['trans']:.3g}, local {worst['local']:.3g} ulp")
    assert worst["kpts"] <= KPTS_TOL
    assert worst["trans"] <= TRANS_TOL
    assert worst["local"] <= 1.0          # a float32 cast of float64 values that differ by the solver's noise


# ---------------------------------------------------------------------------------------------------- the cases themselves
@pytest.mark.parametrize("name", C.NAMES)
def test_cases_meet_their_conditions(name):
    c = C.case(name)
    wr, hr = c["cfg"].resolution
    seen = set()
    for n, s in enumerate(c["samples"]):
        for side, img, P in sides(c, n):
            _, trans, _ = R.geometry(s, P, c["cfg"].grid_range, c["cfg"].aspect_ratio, c["cfg"].resolution)
            margin = min(np.abs(a - np.floor(a) - 0.5).min() for a in R.fixed_arguments(trans, c["cfg"].resolution))
            assert margin >= C.ROUND_MARGIN, f"sample {n} {side}: a value handed to R(.) is {margin:.3g} from a half-integer"
            xs, ys = R.exact_coordinates(trans, c["cfg"].resolution)
            margin = min(np.abs(xs - np.rint(xs)).min(), np.abs(ys - np.rint(ys)).min())
            assert margin >= C.FLOOR_MARGIN, f"sample {n} {side}: an 'exact' source coordinate is {margin:.3g} from an integer"
            if side != "l":
                continue
            h, w = img.shape[:2]
            tags = c["tags"][n]
            seen.update(tags)
            raw = R.warp(img, trans, c["cfg"].resolution)
            zero = (raw == 0).all(axis=2)
            if "inside" in tags:
                assert xs.min() >= 0 and xs.max() <= w - 1 and ys.min() >= 0 and ys.max() <= h - 1 and not zero.any()
            if "outside" in tags:
                assert zero.all() and not R.warp(img, trans, c["cfg"].resolution, "exact").any()
                assert xs.min() > w or xs.max() < -1 or ys.min() > h or ys.max() < -1
            if "border_lt" in tags:
                assert xs.min() < -1 and ys.min() < -1 and xs.max() < w - 1 and ys.max() < h - 1
                assert zero[0].all() and zero[:, 0].all() and not zero[-1, -1]
            if "border_rb" in tags:
                assert xs.max() > w and ys.max() > h and xs.min() > 0 and ys.min() > 0
                assert zero[-1].all() and zero[:, -1].all() and not zero[0, 0]
            if "k>1" in tags:
                assert trans[0, 0] > 1.05 and trans[1, 1] > 1.05
            if "k<1" in tags:
                assert trans[0, 0] < 0.95 and trans[1, 1] < 0.95
    need = {"inside", "border_lt", "border_rb", "k>1"} | ({"outside", "k<1"} if name != "two_frames" else set())
    if name == "gradient_64":
        need.discard("outside")       # its fully-outside crops are the noise cases'
    assert need <= seen, need - seen


def test_cases_have_the_shapes_they_are_there_for():
    wide, tall = C.case("noise_24x16"), C.case("noise_16x24")
    assert wide["left"][0].shape == (37, 53, 3) and tall["left"][0].shape == (41, 29, 3)
    assert (53 * 3) % 4 and (29 * 3) % 4
    assert wide["cfg"].resolution == (24, 16) and tall["cfg"].resolution == (16, 24) and C.case("gradient_64")["cfg"].resolution == (64, 64)
    two = C.case("two_frames")
    assert [im.shape for im in two["left"]] == [(37, 53, 3), (41, 29, 3)] and set(two["frame"].tolist()) == {0, 1}
    assert wide["left"][0].min() >= 1


# ---------------------------------------------------------------------------------------------------- hand answers
IMG = C.noise_image(37, 53, 5)


def test_identity_returns_the_image():
    out = R.warp(IMG, np.array([[1.0, 0, 0], [0, 1.0, 0]]), (53, 37))
    assert np.array_equal(out, IMG)
    assert np.array_equal(R.warp(IMG, np.array([[1.0, 0, 0], [0, 1.0, 0]]), (53, 37), "exact"), IMG)


def test_integer_shift_moves_the_image_and_fills_with_zero():
    # trans maps source (x, y) to output (x + 3, y - 2)
    want = np.zeros_like(IMG)
    want[:-2, 3:] = IMG[2:, :-3]
    for mode in ("fixed5", "exact"):
        assert np.array_equal(R.warp(IMG, np.array([[1.0, 0, 3], [0, 1.0, -2]]), (53, 37), mode), want), mode


def test_half_pixel_shift_averages_horizontal_neighbours():
    # output u samples source u - 0.5: the mean of pixel u - 1 (the zero border at u = 0) and pixel u, rounded half up
    a = np.concatenate([np.zeros((37, 1, 3), dtype=np.int64), IMG[:, :-1].astype(np.int64)], axis=1)
    want = ((a + IMG.astype(np.int64) + 1) >> 1).astype(np.uint8)
    assert np.array_equal(R.warp(IMG, np.array([[1.0, 0, 0.5], [0, 1.0, 0]]), (53, 37)), want)


def test_resolution_is_width_first():
    out = R.warp(IMG, np.array([[1.0, 0, 0], [0, 1.0, 0]]), (24, 16))
    assert out.shape == (16, 24, 3) and np.array_equal(out, IMG[:16, :24])


# ---------------------------------------------------------------------------------------------------- fixed5 against exact
def largest_step(img):
    p = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)))
    return max(np.abs(np.diff(p, axis=0)).max(), np.abs(np.diff(p, axis=1)).max())


@pytest.mark.parametrize("which", ["noise", "gradient"])
def test_fixed5_stays_within_its_bound_of_exact(which):
    img = C.noise_image(37, 53, 10) if which == "noise" else C.gradient_image(40, 56)
    G = largest_step(img)
    bound = 0.5 + 2 * (1 / 64 + 2 / 1024) * G
    if which == "noise":
        assert G == 255 and abs(bound - 9.46) < 0.01
    transforms = [[[1.37, 0, -11.3], [0, 1.37, -7.9]], [[0.61, 0, 2.2], [0, 0.61, 3.3]], [[2.93, 0, 9.1], [0, 2.93, -30.7]],
                  [[1.0, 0, 0.26], [0, 1.0, 0.77]], [[5.11, 0, -100.4], [0, 5.11, -60.2]]]
    worst = 0
    for t in transforms:
        t = np.array(t, dtype=np.float64)
        d = np.abs(R.warp(img, t, (48, 40)).astype(np.int64) - R.warp(img, t, (48, 40), "exact").astype(np.int64)).max()
        worst = max(worst, int(d))
    print(f"{which}: G = {G}, bound {bound:.2f}, worst |fixed5 - exact| {worst}")
    assert worst <= bound


# ---------------------------------------------------------------------------------------------------- normalisation
def test_the_table_is_torchs_normalisation():
    cfg = C.cfg((24, 16))
    table = RoICropper(cfg).norm_table
    assert table.shape == (3, 256) and table.dtype == torch.float32
    levels = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)          # [1,256,3]: every level in every channel
    assert torch.equal(R.normalise(levels, cfg.img_mean, cfg.img_std)[:, 0, :], table)


# ---------------------------------------------------------------------------------------------------- the binding and the class
def test_header_and_binding_agree():
    """The mirrored constants and the workspace query; names, parameters and the ABI number are held by
    tests/test_abi_tables_host.py."""
    text = open(HEADER).read()
    for macro, value in (("SNVC_ROICROP_MAX_SIDE", _roicrop.MAX_SIDE), ("SNVC_ROICROP_MAX_SAMPLES", _roicrop.MAX_SAMPLES)):
        assert int(re.search(rf"#define {macro} (\d+)", text).group(1)) == value
    L = _roicrop.lib()
    assert L.snvc_roicrop_workspace_bytes(0) == 0 and L.snvc_roicrop_workspace_bytes(3) > 0 and L.snvc_roicrop_workspace_bytes(3) % 8 == 0
    assert L.snvc_roicrop_workspace_bytes(-1) < 0 and L.snvc_roicrop_workspace_bytes(_roicrop.MAX_SAMPLES + 1) < 0
    assert _roicrop.ctypes.sizeof(_roicrop.RoICropConfig) == 56


def test_the_c_call_checks_its_arguments_before_any_launch():
    from snvc_amd._lib import lib
    L = _roicrop.lib()
    cfg = _roicrop.RoICropConfig()
    cfg.out_w, cfg.out_h, cfg.aspect_ratio = 24, 16, 0.5
    cfg.grid_range[:] = [1.0, 1.0, 1.0]
    null = [None] * 2
    call = lambda c, n: L.snvc_roicrop(c, *null, 1, None, None, None, None, n, *([None] * 11))  # noqa: E731
    assert call(None, 1) == 1
    assert call(_roicrop.ctypes.byref(cfg), 0) == 0                      # N = 0: nothing to do
    assert call(_roicrop.ctypes.byref(cfg), 1) == 1 and b"null pointer" in lib().snvc_last_error_string()
    assert call(_roicrop.ctypes.byref(cfg), _roicrop.MAX_SAMPLES + 1) == 2
    cfg.out_w = _roicrop.MAX_SIDE + 1
    assert call(_roicrop.ctypes.byref(cfg), 1) == 1 and b"32767" in lib().snvc_last_error_string()
    cfg.out_w, cfg.aspect_ratio = 24, 0.0
    assert call(_roicrop.ctypes.byref(cfg), 1) == 1 and b"aspect_ratio" in lib().snvc_last_error_string()


def bad(**kw):
    base = dict(resolution=(24, 16), aspect_ratio=0.5, grid_range=(1.6, 1.8, 4.0), img_mean=C.MEAN, img_std=C.STD)
    base.update(kw)
    return types.SimpleNamespace(**base)


@pytest.mark.parametrize("kw, text", [
    (dict(resolution=(0, 16)), "positive"), (dict(resolution=(24, -1)), "positive"), (dict(resolution=(32768, 16)), "32767"),
    (dict(resolution=(24, 40000)), "32767"), (dict(aspect_ratio=0), "aspect_ratio"), (dict(grid_range=(1.6, 0.0, 4.0)), "grid_range"),
    (dict(img_std=(0.2, 0.0, 0.2)), "img_std"), (dict(resolution=(24.5, 16)), "integers")])
def test_bad_configurations_are_refused(kw, text):
    with pytest.raises(ValueError, match=text):
        RoICropper(bad(**kw))


def test_a_cpu_device_is_refused():
    c = C.case("noise_24x16")
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        RoICropper(c["cfg"]).generate(c["samples"], c["left"][0], c["right"][0], c["P_left"][0], c["P_right"][0], "cpu")
