"""CPU checks of the rotated-box IoU / NMS family (include/snvc_iou3d.h, snvc_amd/extension/iou3d_nms): the host
BEV IoU against the reference's own compiled CPU function (tests/golden/iou3d_ref.npz, made by
tests/golden/make_golden_iou3d.py), argument validation, and that importing / aliasing the module leaves the GPU alone
(the header against the binding's table and the library's exports: tests/test_abi_tables_host.py)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import abi_tables
from snvc_amd import _iou3d, _lib
from snvc_amd.extension.iou3d_nms import iou3d_nms_utils as U
from snvc_amd.extension.iou3d_nms import numerical_jaccobian as NJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "iou3d_ref.npz"))
BEV_CASES = sorted({k.split("_")[1] for k in GOLD.files if k.startswith("bev_")})


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _iou3d.lib()


@pytest.mark.parametrize("case", BEV_CASES)
def test_host_iou_bev_matches_the_reference(L, case):
    a, b = GOLD[f"bev_{case}_a"], GOLD[f"bev_{case}_b"]
    ref, valid = GOLD[f"bev_{case}_iou"], GOLD[f"bev_{case}_valid"]
    got = U.boxes_bev_iou_cpu(a, b)                                  # numpy in, numpy out
    assert isinstance(got, np.ndarray) and got.shape == ref.shape and got.dtype == np.float32
    err = np.abs(got - ref)[valid]
    assert err.max() < 2e-5, (case, float(err.max()))
    t = U.boxes_bev_iou_cpu(torch.from_numpy(a), torch.from_numpy(b))  # tensor in, tensor out
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), got)


def test_pybind_name_fills_in_place(L):
    a = torch.from_numpy(GOLD["bev_edge_a"])
    ans = torch.full((len(a), len(a)), -1.0)
    assert U.iou3d_nms_cuda.boxes_iou_bev_cpu(a, a, ans) == 1
    valid = GOLD["bev_edge_valid"]
    assert np.abs(ans.numpy() - GOLD["bev_edge_iou"])[valid].max() < 2e-5


def test_margin_semantics_on_the_host(L):
    """The reference's definition, not exact geometry: a 5 mm gap still overlaps through the 1e-2 margin."""
    b = np.array([[0, 0, 0, 2, 2, 2, 0], [2.005, 0, 0, 2, 2, 2, 0], [2.05, 0, 0, 2, 2, 2, 0]], np.float32)
    iou = U.boxes_bev_iou_cpu(b, b)
    assert abs(iou[0, 1] - 0.01 / 7.99) < 1e-6 and iou[0, 2] == 0 and np.allclose(np.diag(iou), 1, atol=1e-6)


def test_empty_inputs_on_the_host(L):
    z = np.zeros((0, 7), np.float32)
    b = GOLD["bev_edge_a"][:3]
    assert U.boxes_bev_iou_cpu(z, b).shape == (0, 3) and U.boxes_bev_iou_cpu(b, z).shape == (3, 0)


def test_argument_errors(L):
    p = ctypes.c_void_p(0)
    assert L.snvc_iou3d_pairwise(p, -1, p, 0, 1, 0, p, p, p) == 1
    assert L.snvc_iou3d_pairwise(p, 1, p, 1, 3, 0, p, p, p) == 1    # unknown `what`
    assert L.snvc_iou3d_pairwise(p, 2, p, 3, 1, 1, p, p, p) == 1    # one-by-one with num_b != num_a
    assert L.snvc_iou3d_pairwise(p, 2, p, 3, 1, 0, p, p, p) == 1    # null pointers
    assert L.snvc_iou3d_pairwise(p, 0, p, 5, 1, 0, p, p, p) == 0    # nothing to do
    assert L.snvc_iou3d_nms(p, _iou3d.NMS_MAX_BOXES + 1, 0.5, 0, p, p, p, p) == 1
    assert b"65536" in _lib.lib().snvc_last_error_string()
    assert L.snvc_iou3d_nms(p, 10, 0.5, 2, p, p, p, p) == 1          # unknown kind
    assert L.snvc_iou3d_nms(p, 10, 0.5, 0, p, p, p, p) == 1          # null pointers
    assert L.snvc_iou3d_backward(p, p, p, 4, 0.0, p, p) == 1          # eps must be positive
    assert L.snvc_iou3d_boxes_iou_bev_cpu(p, -1, p, 2, p) == 1
    assert L.snvc_iou3d_nms_workspace_bytes(65536) == 65536 * 1024 * 8 + 65536 * 80
    assert L.snvc_iou3d_nms_workspace_bytes(65537) == -1
    with pytest.raises(AssertionError):
        U.boxes_bev_iou_cpu(np.zeros((2, 6), np.float32), np.zeros((2, 7), np.float32))


def test_gpu_functions_refuse_cpu_tensors():
    a = torch.zeros((4, 7))
    for fn in (lambda: U.boxes_iou_bev(a, a), lambda: U.boxes_iou3d_gpu(a, a), lambda: U.nms_gpu(a, torch.rand(4), 0.5),
               lambda: U.nms_normal_gpu(a, torch.rand(4), 0.5), lambda: U.boxes_iou3d_gpu_differentiable(a, a),
               lambda: U.iou3d_nms_cuda.boxes_overlap_bev_gpu(a, a, torch.zeros(4, 4)),
               lambda: U.iou3d_nms_cuda.nms_gpu(a, torch.zeros(4, dtype=torch.long), 0.5)):
        with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
            fn()


def test_numerical_jacobian_on_the_host():
    """The module the reference ships broken (torch._six) works: central differences of a row-wise function."""
    x = torch.tensor([[1.0, 2.0], [3.0, -1.0]], dtype=torch.float64)
    y = torch.tensor([[0.5, 0.5], [2.0, 1.0]], dtype=torch.float64)
    jac = NJ.get_numerical_jacobian(lambda inp: (inp[0] ** 2 * inp[1]).sum(1), (x, y), x, eps=1e-3)
    assert torch.allclose(jac, 2 * x * y, atol=1e-9)
    assert torch.equal(x, torch.tensor([[1.0, 2.0], [3.0, -1.0]], dtype=torch.float64))   # restored


def test_import_and_alias_leave_the_gpu_untouched(tmp_path):
    """A fresh interpreter: importing the module, every binding module and install_as_snvc() (which imports every alias)
    neither load the library, nor bind a table, nor initialise the GPU; the reference's import line resolves to this package."""
    tables = ", ".join(row.module for row in abi_tables.ROWS[1:])
    assert len(abi_tables.ROWS) == 17 and "_iou3d" in tables
    for pkg in ("snvc", "snvc/extension"):
        (tmp_path / pkg).mkdir(parents=True)
        (tmp_path / pkg / "__init__.py").write_text("")
    (tmp_path / "snvc/extension/iou3d_nms").mkdir()            # upstream: a directory without __init__.py
    code = (
        "import sys\n"
        f"sys.path[:0] = [{ROOT!r}, {str(tmp_path)!r}]\n"
        "import torch\n"
        "import snvc_amd\n"
        f"from snvc_amd import _lib, {tables}\n"
        "import snvc_amd.extension.iou3d_nms.iou3d_nms_utils\n"
        "snvc_amd.install_as_snvc(backbone=False)\n"
        "from snvc.extension.iou3d_nms.iou3d_nms_utils import nms_gpu, boxes_iou3d_gpu, iou3d_nms_cuda\n"
        "from snvc.extension.iou3d_nms import iou3d_nms_utils as m\n"
        "assert m is snvc_amd.extension.iou3d_nms.iou3d_nms_utils and nms_gpu is m.nms_gpu\n"
        f"assert _lib._lib is None and not any(m.lib.loaded() for m in ({tables})), 'library loaded at import'\n"
        "assert not torch.cuda.is_initialized(), 'GPU initialised at import'\n"
        "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
