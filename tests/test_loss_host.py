"""CPU checks of the training losses (snvc_amd.models.loss3d, include/snvc_loss.h): the float64 restatement of
tests/loss_cases.py and the module's torch route against what the reference computed (tests/golden/loss3d_ref.npz, made by
tests/golden/make_golden_loss.py), the header's constants and struct against the binding's, argument validation
before any device work, the names that are not built, and install_as_snvc."""
import ctypes
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import loss_cases as LC
from snvc_amd import _lib, _loss
from snvc_amd.models import loss3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "loss3d_ref.npz"))


def _against_golden(name, loss, grads, rel, elementwise=False):
    ref = torch.from_numpy(GOLD[f"loss64/{name}"])
    assert loss.shape == ref.shape, name
    assert float((loss.double() - ref).abs().max()) <= rel * float(ref.abs().max()), (name, loss, ref)
    for k, g in grads.items():
        gref = torch.from_numpy(GOLD[f"grad64/{name}/{k}"])
        assert g.shape == gref.shape, (name, k)
        err = (g.double() - gref).abs()
        if elementwise:
            assert bool((err <= rel * gref.abs()).all()), (name, k)
        else:
            assert float(err.max()) <= rel * float(gref.abs().max()), (name, k, float(err.max()))


def test_golden_file_covers_every_small_case():
    assert {k.split("/")[1] for k in GOLD.files if k.startswith("loss64/")} == set(LC.SMALL)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "loss3d_ref.npz")) < 1 << 20
    assert all(GOLD[f"e32/{n}"].shape == (2,) for n in LC.SMALL)


@pytest.mark.parametrize("name", sorted(LC.SMALL))
def test_restatement_matches_the_reference_in_float64(name):
    loss, grads = LC.loss_and_grads(lambda x: LC.restate(name, x), LC.inputs(name))
    _against_golden(name, loss, grads, 1e-12, elementwise=name == "occ_edge")


@pytest.mark.parametrize("name", sorted(LC.SMALL))
def test_torch_route_matches_the_reference_in_float64(name):
    loss, grads = LC.loss_and_grads(lambda x: LC.call(loss3d, name, x), LC.inputs(name))
    assert torch.is_tensor(loss)
    _against_golden(name, loss, grads, 1e-12, elementwise=name == "occ_edge")


@pytest.mark.parametrize("name", sorted(LC.SMALL))
def test_cpu_float32_runs_on_the_torch_route(name):
    loss, grads = LC.loss_and_grads(lambda x: LC.call(loss3d, name, x), LC.inputs(name, torch.float32))
    assert loss.dtype == torch.float32
    _against_golden(name, loss, grads, 1e-5, elementwise=name == "occ_edge")


@pytest.mark.parametrize("name", ["occ_empty", "offset_empty", "depth_empty"])
def test_empty_mask_gives_a_zero_tensor_with_zero_gradient(name):
    x = LC.inputs(name)
    out = LC.call(loss3d, name, x)
    assert torch.is_tensor(out) and out.dim() == 0 and float(out.detach()) == 0.0 and out.requires_grad
    out.backward()
    for t in x["diff"].values():
        assert t.grad is not None and not bool(t.grad.any())


def test_coordinate_loss_leaves_the_callers_gt_alone():
    x = LC.inputs("coord_norm")
    before = x["const"]["corners"].clone()
    LC.call(loss3d, "coord_norm", x)
    assert torch.equal(x["const"]["corners"], before)


def test_input_checks_raise_at_once_on_the_torch_route():
    x = LC.inputs("msew")
    x["const"]["gt"][:, 1] = -1.0                    # part 1 without a positive target
    with pytest.raises(loss3d.LossInputError):
        LC.call(loss3d, "msew", x)
    x = LC.inputs("focal_w")
    x["const"]["targets"][0, 0] = 2.0
    with pytest.raises(loss3d.LossInputError, match="0 or 1"):
        LC.call(loss3d, "focal_w", x)


def test_names_that_are_not_built_exist_and_say_why():
    t = torch.zeros(2, 7)
    cfg3d = types.SimpleNamespace(head_reg_type="vector3d")
    calls = [lambda: loss3d.RPN3DLoss(types.SimpleNamespace()), lambda: loss3d.disentangled_loss(t, t, t[:, 0]), lambda: loss3d.map2corners(t),
             lambda: loss3d.compute_IoU_loss_corner(t, t), lambda: loss3d.approximated_3d_iou_pt(t, t, [0, 2, 5, 4, 6]),
             lambda: loss3d.BboxLoss(cfg3d), lambda: loss3d.CoordinateLoss(LC.COORD_CFG, enable_IoU=True)]
    for fn in calls:
        with pytest.raises(NotImplementedError, match="nowhere in the reference|global detector"):
            fn()
    for name in ("sigmoid_focal_loss_multi_target", "smooth_l1_loss", "W_loss", "calc_disp_loss", "DepthLoss", "VoxelMSELoss",
                 "OccupancyLoss", "OffsetLoss", "compute_area_4pts", "ShapeLoss", "BboxLoss", "CoordinateLoss", "VoxelMSELossWeighted",
                 "INF", "CFG_NAMES", "SELECT_IND1", "SELECT_IND2", "depth_regression_loss", "check"):
        assert hasattr(loss3d, name), name
    with pytest.raises(NotImplementedError):
        loss3d.calc_disp_loss({}, None, None, loss_type="other")
    square = torch.tensor([[[[0., 0.], [2., 0.], [2., 3.], [0., 3.]]]])
    assert float(loss3d.compute_area_4pts(square)) == 6.0 and float(loss3d.compute_area_4pts(square, "edge-product")) == 6.0


def test_install_as_snvc_resolves_loss3d(tmp_path, monkeypatch):
    """`from snvc.models.loss3d import ...` gives this package's module (a stand-in package tree for the reference)."""
    pkg = tmp_path / "snvc" / "models"
    pkg.mkdir(parents=True)
    (tmp_path / "snvc" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "loss3d.py").write_text("raise ImportError('the reference loss3d must not be imported')\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == "snvc" or k.startswith("snvc.")]:
        monkeypatch.delitem(sys.modules, k)
    import snvc_amd
    snvc_amd.install_as_snvc(backbone=False)
    try:
        from snvc.models.loss3d import OccupancyLoss, VoxelMSELoss, calc_disp_loss
        assert sys.modules["snvc.models.loss3d"] is loss3d and OccupancyLoss is loss3d.OccupancyLoss and VoxelMSELoss is loss3d.VoxelMSELoss
        assert calc_disp_loss is loss3d.calc_disp_loss
    finally:
        for k in [k for k in sys.modules if k == "snvc" or k.startswith("snvc.")]:
            del sys.modules[k]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _loss.lib()


def test_header_table_and_exports_agree():
    """The mirrored constants, enumerators and struct; names, exports and the ABI number are held by
    tests/test_abi_tables_host.py."""
    hdr = open(os.path.join(ROOT, "include", "snvc_loss.h")).read()
    assert f"SNVC_LOSS_MAX_ROWS {_loss.MAX_ROWS}" in hdr
    kinds = re.findall(r"^\s*SNVC_LOSS_(\w+) = (\d+)", hdr, re.M)
    for name, value in kinds:
        if hasattr(_loss, name):
            assert getattr(_loss, name) == int(value), name
    assert {"MSE_ROWS", "MSE_POSNEG", "OCCUPANCY", "OFFSET", "SMOOTH_L1_MASKED", "SIGMOID_FOCAL", "SMOOTH_L1_ROWS"} <= {n for n, _ in kinds}
    fields = re.search(r"typedef struct snvc_loss_desc \{(.*?)\} snvc_loss_desc;", hdr, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert [n for n in names if n in dict(_loss.LossDesc._fields_)] == [n for n, _ in _loss.LossDesc._fields_]


def _desc(kind, rows=1, cols=16, group=1, p0=1.0, **ptrs):
    d = _loss.LossDesc()
    d.kind, d.rows, d.cols, d.group, d.p0 = kind, rows, cols, group, p0
    for k in ("a", "b", "fin", "partials", "loss", "flag", "gout", "ga"):
        setattr(d, k, 0x1000)
    for k, v in ptrs.items():
        setattr(d, k, v)
    return d


def test_arguments_are_checked_before_any_launch(L):
    """Every rejected call returns an error code without touching a device pointer (none of these point anywhere)."""
    p = 0x1000
    bad = [_desc(99), _desc(_loss.OCCUPANCY, rows=2), _desc(_loss.MSE_POSNEG, rows=7, group=3), _desc(_loss.OFFSET, rows=6, group=3),
           _desc(_loss.SMOOTH_L1_ROWS, cols=10, group=3, roww=p), _desc(_loss.SMOOTH_L1_ROWS, cols=9, group=3),
           _desc(_loss.SMOOTH_L1_MASKED, p0=0.0), _desc(_loss.OCCUPANCY, a=None), _desc(_loss.OCCUPANCY, fin=None),
           _desc(_loss.MSE_POSNEG, rows=0), _desc(_loss.OCCUPANCY, cols=-1)]
    for d in bad:
        assert L.snvc_loss_forward(ctypes.byref(d), None) != 0
        assert L.snvc_loss_backward(ctypes.byref(d), None) != 0
    assert L.snvc_loss_forward(ctypes.byref(_desc(_loss.MSE_POSNEG, rows=70000, group=1)), None) == 2      # unsupported
    assert "SNVC_LOSS_MAX_ROWS" in _lib.lib().snvc_last_error_string().decode()
    assert L.snvc_loss_forward(ctypes.byref(_desc(_loss.OCCUPANCY, loss=None)), None) != 0
    assert L.snvc_loss_backward(ctypes.byref(_desc(_loss.OCCUPANCY, gout=None)), None) != 0
    assert L.snvc_loss_partials_count(ctypes.byref(_desc(99))) < 0
    assert L.snvc_loss_partials_count(ctypes.byref(_desc(_loss.MSE_POSNEG, rows=6, cols=5001, group=3))) == 6 * 5 * 4   # scalar tiles of 1024
    assert L.snvc_loss_wdist_forward(p, p, p, None, p, 1, 4, 16, None, p, p, p, None) != 0                 # no mask
    assert L.snvc_loss_wdist_forward(p, p, p, p, p, 1, -4, 16, None, p, p, p, None) != 0
    assert L.snvc_loss_wdist_backward(p, p, p, p, p, 1, 4, 16, None, None, None, p, p, None) != 0          # neither gpix nor gout
    assert L.snvc_loss_depth_regression_forward(p, p, p, 1, 0, 16, p, p, p, None) != 0                     # D = 0
    assert L.snvc_loss_depth_regression_forward(p, None, p, 1, 4, 16, p, p, p, None) != 0
    assert L.snvc_loss_depth_regression_backward(p, p, p, 1, 4, 16, p, None, p, None) != 0
    assert L.snvc_loss_disparity_regression_backward(p, None, p, 1, 4, 16, None) != 0
    assert L.snvc_loss_disparity_regression_backward(p, p, p, 1, 70000, 16, None) == 2
    assert L.snvc_loss_wdist_partials_count(1, -1, 4, 0) < 0 and L.snvc_loss_depth_regression_partials_count(-1, 4) < 0


def test_the_binding_rejects_cpu_and_misshapen_operands():
    a = torch.zeros(4, 6)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _loss.elementwise(_loss.OCCUPANCY, a, a)
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _loss.depth_regression_loss(torch.zeros(1, 4, 2, 2), torch.zeros(4), torch.zeros(1, 2, 2))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _loss.wdist(torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 2, 2), torch.zeros(1, 2, 2), torch.zeros(1, 2, 2, dtype=torch.uint8), torch.zeros(4))
