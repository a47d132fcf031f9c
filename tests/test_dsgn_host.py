"""CPU checks of the DSGN image backbone (snvc_amd.models.submodule.feature_extraction / BasicBlock, include/snvc_dsgn.h):
the module tree and state-dict keys against the reference's (tests/golden/dsgn_ref*.npz, made by
tests/golden/make_golden_dsgn.py), the torch route's arithmetic against the stored outputs, argument validation before
any device work, and install_as_snvc."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import dsgn_cases as DC
from benchlib.common import seeded_state
from snvc_amd import _dsgn, _lib
from snvc_amd.models import submodule as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {}
for _f, _names in DC.FILES.items():
    _z = np.load(os.path.join(ROOT, "tests", "golden", _f))
    GOLD.update({k: _z[k] for k in _z.files})


def _layout(m):
    return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def _gold_layout(name):
    return list(zip(GOLD[f"keys/{name}"].tolist(), [tuple(int(d) for d in s if d >= 0) for s in GOLD[f"shapes/{name}"]]))


@pytest.mark.parametrize("backbone", DC.BACKBONES)
def test_every_backbone_has_the_reference_layout(backbone):
    assert _layout(S.feature_extraction(DC.cfg(backbone=backbone))) == _gold_layout(backbone)


@pytest.mark.parametrize("name", sorted(DC.GOLDEN))
def test_golden_configs_have_the_reference_layout_and_load_strict(name):
    m = S.feature_extraction(DC.cfg(**DC.GOLDEN[name][0]))
    assert _layout(m) == _gold_layout(name)
    sd = {k: torch.randn(v.shape) if v.is_floating_point() else v for k, v in m.state_dict().items()}
    other = S.feature_extraction(DC.cfg(**DC.GOLDEN[name][0]))
    other.load_state_dict(sd, strict=True)        # a state dict in the reference's layout
    assert all(torch.equal(a, sd[k]) for k, a in other.state_dict().items())


def test_switches_build_what_the_reference_builds():
    m = S.feature_extraction(DC.cfg(**DC.GOLDEN["rpn_ac"][0]))
    assert not hasattr(m, "lastconv") and len(m.rpnconv) == 4 and isinstance(m.rpnconv[2][1], torch.nn.BatchNorm2d)
    gn = S.feature_extraction(DC.cfg(GN=True, RPN3D_ENABLE=True, cat_img_feature=True, RPN_CONVDIM=48, img_feature_relu=False))
    assert len(gn.rpnconv) == 1 and gn.rpnconv[0][1].num_groups == 16 and gn.branch1[1][1].num_groups == 32
    assert isinstance(gn.firstconv[0][1], torch.nn.GroupNorm) and isinstance(gn.layer4[0].downsample[1], torch.nn.GroupNorm)
    fixfirst = S.feature_extraction(DC.cfg(GN=True, backbone="reslike-det-small-fixfirst"))
    assert isinstance(fixfirst.firstconv[0][1], torch.nn.BatchNorm2d)            # first_dim 16 < 32: BatchNorm
    assert fixfirst.layer4[1].conv1[0][0].dilation == (2, 2) and fixfirst.layer4[1].conv1[0][0].padding == (2, 2)
    with pytest.raises(ValueError):
        S.feature_extraction(DC.cfg(backbone="resnet"))
    b = S.BasicBlock(8, 8, 1, None, 1, 2, gn=False)
    assert [k for k in b.state_dict()][:2] == ["conv1.0.0.weight", "conv1.0.1.weight"]


@pytest.mark.parametrize("name", ["tiny_nobranch", "rpn_ac"])
def test_torch_route_matches_the_stored_reference_outputs(name):
    """The torch route is the reference's arithmetic (the golden configurations small enough to run here)."""
    fields, shape, wseed, xseed = DC.GOLDEN[name]
    m = S.feature_extraction(DC.cfg(**fields))
    m.load_state_dict(seeded_state(m, wseed), strict=True)
    with torch.no_grad():
        feat, rpn = m.eval()._forward_torch(DC.image(shape, xseed))
    for key, got in ((f"out/{name}", feat), (f"rpn/{name}", rpn)):
        if key in GOLD:
            ref = torch.from_numpy(GOLD[key])
            assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5, key
        else:
            assert got is None


def test_cpu_input_raises():
    m = S.feature_extraction(DC.cfg(backbone="reslike50-det-tiny", branch=False)).eval()
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        m(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        S.BasicBlock(8, 8, 1, None, 1, 1)(torch.zeros(1, 8, 8, 8))
    with pytest.raises(RuntimeError, match="Not implemented on the CPU"):
        _dsgn.spp_pool(torch.zeros(1, 4, 64, 64))


def test_install_as_snvc_resolves_feature_extraction(tmp_path, monkeypatch):
    """`from snvc.models.submodule import feature_extraction, BasicBlock` gives this package's classes (a stand-in
    package tree for the reference checkout)."""
    pkg = tmp_path / "snvc" / "models"
    pkg.mkdir(parents=True)
    (tmp_path / "snvc" / "__init__.py").write_text("")
    (pkg / "__init__.py").write_text("")
    (pkg / "submodule.py").write_text("raise ImportError('the reference submodule must not be imported')\n")
    monkeypatch.syspath_prepend(str(tmp_path))
    for k in [k for k in sys.modules if k == "snvc" or k.startswith("snvc.")]:
        monkeypatch.delitem(sys.modules, k)
    import snvc_amd
    snvc_amd.install_as_snvc(backbone=False)
    try:
        from snvc.models.submodule import BasicBlock, feature_extraction
        assert feature_extraction is S.feature_extraction and BasicBlock is S.BasicBlock
    finally:
        for k in [k for k in sys.modules if k == "snvc" or k.startswith("snvc.")]:
            del sys.modules[k]


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _dsgn.lib()


def test_header_table_and_exports_agree():
    """The mirrored constant; names, exports and the ABI number are held by tests/test_abi_tables_host.py."""
    hdr = open(os.path.join(ROOT, "include", "snvc_dsgn.h")).read()
    assert f"SNVC_DSGN_MAX_CELLS {_dsgn.MAX_CELLS}" in hdr


def test_arguments_are_checked_before_any_launch(L):
    """Every rejected call returns an error code without touching a device pointer (none of these point anywhere)."""
    p = 0x1000
    assert L.snvc_dsgn_spp_pool(p, 0, p, p, p, p, 1, 4, 63, 128, None) != 0          # the 64 window does not fit
    assert L.snvc_dsgn_spp_pool(p, 0, p, p, p, None, 1, 4, 64, 64, None) != 0        # a missing output
    assert L.snvc_dsgn_spp_pool(p, 0, p, p, p, p, 1, 4, 1024, 1024, None) == 2       # too many 8 x 8 cells: unsupported
    assert L.snvc_dsgn_spp_pool(p, 5, p, p, p, p, 2, 4, 64, 64, None) != 0           # batch stride below a sample
    maps = (_dsgn.c_p * 4)(p, p, p, None)
    ext = (_dsgn.c_i64 * 8)(1, 4, 3, 9, 6, 19, 12, 39)
    assert L.snvc_dsgn_spp_upsample(maps, ext, p, 0, 1, 32, 96, 312, 0, None) != 0   # a NULL map
    maps = (_dsgn.c_p * 4)(p, p, p, p)
    big = (_dsgn.c_i64 * 8)(1, 4, 3, 9, 6, 19, 97, 39)
    assert L.snvc_dsgn_spp_upsample(maps, big, p, 0, 1, 32, 96, 312, 0, None) != 0   # a map taller than the output
    assert "map 3" in _lib.lib().snvc_last_error_string().decode()


def test_dilated_depth1_layer_plan(L):
    """The depth-1 dilation-2 layer is accepted for 3 x 3 / stride 1 / pad 2 only, and carries no Winograd weights."""
    import ctypes
    from snvc_amd import ops

    def desc(k, s, dil, pad, hin=16, win=32):
        d = ops.Conv3dDesc()
        d.N, d.Cin, d.Din, d.Hin, d.Win, d.Cout, d.Dout = 1, 32, 1, hin, win, 32, 1
        d.Hout, d.Wout = (hin + 2 * pad - dil * (k - 1) - 1) // s + 1, (win + 2 * pad - dil * (k - 1) - 1) // s + 1
        d.ksize, d.stride, d.dilation, d.pad, d.ksize_d = k, s, dil, pad, 1
        return d
    count = _lib.lib().snvc_conv3d_packed_weight_count
    assert count(ctypes.byref(desc(3, 1, 2, 2))) == 32 * 32 * 9             # the direct packing alone
    assert count(ctypes.byref(desc(3, 1, 1, 1))) > 32 * 32 * 9              # dilation 1 also carries the Winograd weights
    for bad in (desc(3, 1, 2, 1), desc(3, 2, 2, 2), desc(1, 1, 2, 0), desc(5, 1, 2, 4)):
        assert count(ctypes.byref(bad)) < 0
