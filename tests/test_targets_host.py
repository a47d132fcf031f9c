"""CPU checks of the training-target generator (snvc_amd.geometry.TargetGenerator, include/snvc_targets.h): the golden file
(tests/golden/targets_ref.npz, made by tests/golden/make_golden_targets.py) against the case table, the header against the
binding's table and the library's exports, and argument validation before any device work."""
import ctypes
import os
import re

import numpy as np
import pytest

import target_cases as TC
from snvc_amd import _lib, _targets
from snvc_amd.geometry import TargetGenerator

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_targets.h")


def test_golden_file_holds_what_the_cases_declare():
    gold = TC.load_golden()
    want = {f"{name}/{key}" for name in TC.SMALL + (TC.FULL,) for key in TC.expected_arrays(name)}
    assert set(gold.files) == want
    for name in TC.SMALL + (TC.FULL,):
        for key, (shape, dtype) in TC.expected_arrays(name).items():
            a = gold[f"{name}/{key}"]
            assert a.shape == shape and a.dtype == dtype, (name, key, a.shape, a.dtype)
    for name in TC.SMALL:
        assert set(np.unique(gold[f"{name}/occupancy"])) <= {-1, 0, 1}
    golden_dir = os.path.dirname(TC.GOLDEN_NPZ)
    others = [os.path.getsize(os.path.join(golden_dir, f)) for f in os.listdir(golden_dir) if f.endswith(".npz") and f != "targets_ref.npz"]
    assert os.path.getsize(TC.GOLDEN_NPZ) <= max(others) and os.path.getsize(TC.GOLDEN_NPZ) < 1 << 20


def test_the_small_cases_cover_what_they_are_for():
    gold = TC.load_golden()
    for name, full in (("small2d", 13 ** 2), ("small3d", 13 ** 3)):
        cells = (gold[f"{name}/fields"].reshape(3, 9, -1) != 0).sum(axis=2)
        assert cells[0, 0] == full and (cells[0] > 0).all()                     # label close by
        assert ((cells[1] > 0) & (cells[1] < full)).sum() >= 3                  # windows clipped by the border
        assert (cells[2] == 0).any()                                            # a channel of zeros
        occ = gold[f"{name}/occupancy"]
        assert all((occ[:2] == v).any() for v in (-1, 0, 1))
    c = TC.case("odd3d")
    assert all(e % 4 for e in (np.prod(c["cfg"].grid_resolution), c["cfg"].grid_resolution[2] * c["cfg"].grid_resolution[1]))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _targets.lib()


def test_header_table_and_exports_agree():
    """The mirrored constants and struct; names, exports and the ABI number are held by tests/test_abi_tables_host.py."""
    hdr = open(HEADER).read()
    assert f"SNVC_TARGETS_MAX_PARTS {_targets.MAX_PARTS}" in hdr and f"SNVC_TARGETS_MAX_SAMPLES {_targets.MAX_SAMPLES}" in hdr
    fields = re.search(r"typedef struct snvc_targets_grid \{(.*?)\} snvc_targets_grid;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", fields)
    assert names == [n for n, _ in _targets.TargetsGrid._fields_]


def test_the_main_header_is_untouched():
    hdr = open(os.path.join(ROOT, "include", "snvc_hip.h")).read()
    assert "snvc_targets" not in hdr


def test_arguments_are_checked_before_any_launch(L):
    """Every rejected call returns an error code without touching a device pointer (none of these point anywhere)."""
    p = 0x1000
    good = TargetGenerator(TC.case("small3d")["cfg"]).grid

    def grid(**kw):
        g = _targets.TargetsGrid.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(g, k, v)
        return ctypes.byref(g)

    def fields(g, n=1, **kw):
        a = dict(samples=p, labels=p, ws=p, out=p, corners=p)
        a.update(kw)
        return L.snvc_targets_fields(g, a["samples"], a["labels"], n, a["ws"], a["out"], a["corners"], None)

    def occupancy(g, n=1, total=8, pmax=8, f64=0, **kw):
        a = dict(samples=p, labels=p, points=p, slices=None, v2r=None, ws=p, occ=p, in_roi=None, in_fg=None)
        a.update(kw)
        return L.snvc_targets_occupancy(g, a["samples"], a["labels"], n, a["points"], f64, total, a["slices"], pmax, a["v2r"], a["ws"],
                                        a["occ"], a["in_roi"], a["in_fg"], None)

    for bad in (grid(num_parts=10), grid(num_parts=0), grid(sigma=0), grid(grid_type=4), grid(nh=0), grid(nw=-3),
                grid(nh=2048, nw=2048, nl=2048)):
        assert fields(bad) == 1 and occupancy(bad) == 1
    fields(grid(num_parts=10))
    assert "Only support less than or equal to 9 object parts" in _lib.lib().snvc_last_error_string().decode()
    g = grid()
    assert fields(g, n=-1) == 1 and fields(g, n=_targets.MAX_SAMPLES + 1) == 2
    assert "SNVC_TARGETS_MAX_SAMPLES" in _lib.lib().snvc_last_error_string().decode()
    for missing in ("samples", "labels", "ws", "out", "corners"):
        assert fields(g, **{missing: None}) == 1
    assert fields(g, out=p + 4) == 1                                 # the 16-byte stores need an aligned buffer
    for missing in ("samples", "labels", "ws", "occ", "points"):
        assert occupancy(g, **{missing: None}) == 1
    assert occupancy(g, occ=p + 8) == 1
    assert occupancy(g, in_roi=p) == 1                               # the masks come together
    assert occupancy(g, pmax=9) == 1 and occupancy(g, total=-1, pmax=0) == 1
    assert fields(g, n=0) == 0 and occupancy(g, n=0) == 0            # nothing to do: nothing launched
    assert L.snvc_targets_workspace_bytes(-1) < 0 and L.snvc_targets_workspace_bytes(_targets.MAX_SAMPLES + 1) < 0
    assert L.snvc_targets_workspace_bytes(0) == 0 and L.snvc_targets_workspace_bytes(3) == 3 * L.snvc_targets_workspace_bytes(1)
    assert L.snvc_targets_workspace_bytes(1) % 8 == 0


def test_cpu_device_is_refused():
    c = TC.case("odd3d")
    gen = TargetGenerator(c["cfg"])
    with pytest.raises(RuntimeError, match="needs a GPU device: Not implemented on the CPU"):
        gen.generate(c["samples"], c["label"], c["points"], "cpu")


def test_cfg_is_validated():
    cfg = lambda **kw: TC.make_cfg((5, 7, 11), kw.pop("sigma", 1), kw.pop("parts", 9), kw.pop("grid_type", "3D"), **kw)  # noqa: E731
    with pytest.raises((AssertionError, ValueError), match="Only support less than or equal to 9 object parts"):
        TargetGenerator(cfg(parts=10))
    for sigma in (1.5, 2.0, 0, -1, True):
        with pytest.raises(ValueError, match="sigma"):
            TargetGenerator(cfg(sigma=sigma))
    for grid_type in ("BEV", "3d", 3, None):
        with pytest.raises(ValueError, match="grid_type"):
            TargetGenerator(cfg(grid_type=grid_type))
    with pytest.raises(ValueError, match="positive"):
        TargetGenerator(cfg(spacing=(0.1, 0.0, 0.1)))
    gen = TargetGenerator(cfg(sigma=np.int64(2), grid_type="2D"))
    assert gen.field_shape(4) == (4, 9, 11, 7) and gen.sigma == 2
