"""CPU checks of the HRNet backbone (snvc_amd.models.hrnet, include/snvc_hrnet.h): the module tree and state-dict keys
against the reference's (tests/golden/hrnet_ref.npz, made by tests/golden/make_golden_hrnet.py), argument validation
before any device work, and the wiring into VernierScale and install_as_snvc.  The header against the binding's table and
the library's exports: tests/test_abi_tables_host.py."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from benchlib import hrnet as B
from snvc_amd import _hrnet, _lib
from snvc_amd.models import hrnet as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "hrnet_ref.npz"))


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _hrnet.lib()


def _keys(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


@pytest.mark.parametrize("name,cfg", [("w32", B.W32), ("w48", B.W48)])
def test_keys_and_shapes_equal_the_reference(name, cfg):
    m = H.get_model(copy.deepcopy(cfg), False)
    shapes = [tuple(int(d) for d in s if d >= 0) for s in GOLD[f"shapes/{name}"]]
    assert _keys(m) == list(zip(GOLD[f"keys/{name}"].tolist(), shapes))
    assert sum(isinstance(x, torch.nn.Conv2d) for x in m.modules()) == 305
    sd = {k: torch.randn(v.shape) if v.is_floating_point() else v for k, v in m.state_dict().items()}
    other = H.get_model(copy.deepcopy(cfg), False)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(a, sd[k]) for k, a in other.state_dict().items())


def test_add_xy_and_head_types_keep_the_reference_layout():
    cfg = copy.deepcopy(B.SMALL["s_add_xy"][0])
    m = H.get_model(cfg, False)
    keys = list(m.state_dict())
    assert keys[-1] == "conv1.weight" and m.conv1.weight.shape == (64, 5, 3, 3)       # re-registered last, as the reference
    assert not hasattr(H.get_model(B.W32, False, head_type="heatmap_regression"), "conv1")
    cls = H.get_model(B.W32, False, head_type="classification")
    assert cls.classifier.weight.shape == (1000, 2048) and len(cls.incre_modules) == 4


def test_init_weights_loads_the_matching_keys(tmp_path):
    cfg = copy.deepcopy(B.SMALL["s_basic"][0])
    m = H.get_model(cfg, False)
    part = {"conv2.weight": torch.full_like(m.conv2.weight, 0.25), "not_a_key": torch.zeros(1)}
    torch.save(part, tmp_path / "pre.pth")
    m.init_weights(str(tmp_path / "pre.pth"))
    assert torch.equal(m.conv2.weight, part["conv2.weight"]) and torch.equal(m.bn1.weight, torch.ones(64))


def _forward(L, ptrs, factors, extents, out=0x1000, shape=(1, 4, 8, 8)):
    t, f, e = _hrnet.host_arrays(ptrs, factors, extents)
    return L.snvc_hrnet_fuse_forward(t, f, e, out, *shape, 1, None)


def _error():
    return _lib.lib().snvc_last_error_string().decode()


def test_entry_points_reject_bad_arguments_on_the_host(L):
    """Rejected before any launch: the pointers below are never dereferenced (no device is touched)."""
    a, b = 0x1000, 0x2000
    assert _forward(L, [None, a], [1, 2], [8, 8, 4, 4]) == 1 and "term 0" in _error()
    assert _forward(L, [a, b], [1, 3], [8, 8, 3, 3]) == 1 and "factor 3" in _error()
    assert _forward(L, [a, b], [1, 16], [8, 8, 1, 1]) == 1 and "factor 16" in _error()
    assert _forward(L, [a, b], [1, 2], [8, 8, 5, 4]) == 1 and "5 x 4" in _error()       # an input that is not a multiple of 32
    assert _forward(L, [a, b], [1, 2], [8, 8, 4, 4], out=b) == 1 and "alias" in _error()
    rc = L.snvc_hrnet_fuse_backward(a, b, None, None, a, None, 1, 4, 6, 6, 1, None)      # 6 x 6 has no 4 x 4 blocks
    assert rc == 1 and "factor 4" in _error()
    assert L.snvc_hrnet_fuse_backward(None, b, a, None, None, None, 1, 4, 8, 8, 1, None) == 1


def test_cpu_input_raises():
    m = H.get_model(copy.deepcopy(B.SMALL["s_basic"][0]), False).eval()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m(torch.zeros(1, 3, 64, 64))


def test_get_feat_extraction_builds_our_hrnet():
    from snvc_amd.models import vernier as V
    for cfg in (B.W32, B.W48):
        m = V.get_feat_extraction(copy.deepcopy(cfg), False)
        assert isinstance(m, H.HighResolutionNet)
    assert isinstance(V.get_feat_extraction(type("C", (), {"name": "identity"})()), torch.nn.Identity)


def test_install_as_snvc_hip_backbone(tmp_path):
    """A fresh interpreter with a stand-in reference package whose hrnet module must not be used: backbone="hip" resolves
    snvc.models.hrnet to this package's, and VernierScale's factory builds it; nothing touches the GPU."""
    for pkg in ("snvc", "snvc/models", "snvc/extension", "snvc/extension/roiaware_pool3d"):
        (tmp_path / pkg).mkdir(parents=True)
        (tmp_path / pkg / "__init__.py").write_text("")
    (tmp_path / "snvc/models/hrnet.py").write_text("raise ImportError('the reference hrnet must not be imported')\n")
    code = (
        "import sys, copy\n"
        f"sys.path[:0] = [{ROOT!r}, {str(tmp_path)!r}]\n"
        "import torch\n"
        "import snvc_amd\n"
        "snvc_amd.install_as_snvc(backbone='hip')\n"
        "import snvc.models.hrnet as h\n"
        "from snvc.models.hrnet import HighResolutionNet, get_model, blocks_dict, BN_MOMENTUM\n"
        "import snvc_amd.models.hrnet as ours\n"
        "import snvc_amd.models.vernier as v\n"
        "from benchlib import hrnet as B\n"
        "assert h is ours and HighResolutionNet is ours.HighResolutionNet\n"
        "assert isinstance(v.get_feat_extraction(copy.deepcopy(B.W32), False), ours.HighResolutionNet)\n"
        "assert not torch.cuda.is_initialized(), 'GPU initialised'\n"
        "print('ok')\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
