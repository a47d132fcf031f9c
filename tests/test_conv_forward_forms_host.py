"""CPU checks of the fp32 forward convolution's dispatcher (conv3d_forward_impl in csrc/conv3d.hip, asked through
snvc_conv3d_forward_form of include/snvc_forms.h): the table of tests/conv_forward_cases.py against what the dispatcher itself
decides.  No GPU: without a device the CU count falls back to 256, which is also an MI355X's own count; the one pair of rows that
depends on it is sized for 256 here and for the device's count in tests/test_gpu_conv_forward_forms.py.
"""
import ctypes
import os
import re

import pytest

import conv_forward_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "snvc_forms.h")).read()
CUS = 256


def _enum():
    from snvc_amd import _forms
    return _forms.enum_names(HEADER, "CF")


def _query(case, **over):
    from snvc_amd import _forms
    d = CC.geometry(case)._desc(*CC.desc_args(case, CUS))
    a = dict(zip(("x_align", "y_align", "res_align", "planes_align", "y_head_align"), CC.alignments(case)))
    a.update(over)
    return _forms.conv3d_forward(d, CC.ENTRIES[case.entry], **a)


@pytest.mark.parametrize("case", [c for c in CC.CASES if c.form], ids=str)
def test_the_row_takes_its_form_with_its_launch_numbers(case):
    names = {v: k for k, v in _enum().items()}
    rc, info, text = _query(case)
    assert rc > 0, text
    assert names[rc] == case.form
    assert info == CC.expected_numbers(case, CUS)
    # under the SNVC_ALGO_DIRECT bit no Winograd form is taken, whatever else the row says
    if case.bits & 0xff == CC.DIRECT:
        assert CC.FORMS[case.form][0] != "wino"


@pytest.mark.parametrize("case", [c for c in CC.CASES if c.refusal], ids=str)
def test_the_row_is_refused_with_the_entry_points_status_and_text(case):
    from snvc_amd import _forms
    d = CC.geometry(case)._desc(*CC.desc_args(case, CUS))
    info = (ctypes.c_int64 * _forms.INFO)(*([7] * _forms.INFO))
    rc = _forms.lib().snvc_conv3d_forward_form(ctypes.byref(d), CC.ENTRIES[case.entry], *CC.alignments(case), ctypes.cast(info, ctypes.c_void_p))
    status, words = case.refusal
    assert rc == -status
    assert _forms._lib.lib().snvc_last_error_string().decode().startswith(words)
    assert not any(info)


def test_an_empty_batch_launches_nothing():
    empty = [c for c in CC.CASES if c.n == 0 and c.refusal is None]
    assert len(empty) >= 2
    for case in empty:
        rc, info, _ = _query(case)
        assert rc == 0 and not any(info.values()), case


def test_the_launcher_gives_the_same_refusal_before_it_reads_a_pointer():
    """The descriptor refusals through the entry point itself: make_plan runs before the pointer check, so null operands do."""
    from snvc_amd import _lib
    L = _lib.lib()
    for name in ("no channels", "k5 stride 2", "k3 pad 0", "depth-1 k5", "transposed pad 0", "too many samples"):
        case = CC.BY_NAME[name]
        d = CC.geometry(case)._desc(*CC.desc_args(case, CUS))
        assert L.snvc_conv3d_forward(ctypes.byref(d), None, None, None, None, None, None, None) == case.refusal[0], name
        assert L.snvc_last_error_string().decode().startswith(case.refusal[1]), name
    case = CC.BY_NAME["k3 empty batch"]
    d = CC.geometry(case)._desc(*CC.desc_args(case, CUS))
    assert L.snvc_conv3d_forward(ctypes.byref(d), None, None, None, None, None, None, None) == 0


def test_the_query_refuses_what_is_no_alignment_or_entry_point():
    from snvc_amd import _forms
    case = CC.BY_NAME["k3 n3"]
    for over in (dict(x_align=12), dict(y_align=32), dict(res_align=-4)):
        rc, info, text = _query(case, **over)
        assert rc == -CC.INVALID and text.startswith("snvc_conv3d_forward_form:") and not any(info.values())
    d = CC.geometry(case)._desc(*CC.desc_args(case, CUS))
    assert _forms.conv3d_forward(d, 4)[0] == -CC.INVALID


def test_the_alignment_of_each_operand_is_read():
    """One operand at a time 8 and 4 bytes off, on the default form with a residual and depth planes: each leaves it."""
    names = {v: k for k, v in _enum().items()}
    case = CC.BY_NAME["k3 n3 residual after, planes"]
    assert names[_query(case)[0]] == "WINO_N3"
    for operand in ("x_align", "y_align", "res_align", "planes_align"):
        assert names[_query(case, **{operand: 8})[0]] == "WINO_N8", operand
        assert names[_query(case, **{operand: 4})[0]] == "K3M2", operand
    side = CC.BY_NAME["k3 side head"]
    assert _query(side)[0] > 0 and _query(side, y_head_align=8)[0] == -CC.UNSUPPORTED


def test_the_depth1_winograd_pair_sits_on_either_side_of_two_jobs_per_cu():
    a, b = CC.BY_NAME["winop two jobs per CU"], CC.BY_NAME["winop just under two jobs per CU"]
    assert a.shape(CUS) == a.sp and b.shape(CUS) == b.sp             # the table's literal extents are those of 256 CUs
    assert _query(a)[1]["tiles"] == 2 * CUS and 16 * (b.sp[2] // 32) == 2 * CUS - 16


def test_every_form_of_the_header_is_a_rows_expected_form():
    enum = _enum()
    assert sorted(enum.values()) == list(range(1, len(enum) + 1)) and len(enum) == 44
    assert set(enum) == set(CC.FORMS)
    expected = {c.form for c in CC.CASES if c.form}
    assert expected == set(enum), sorted(set(enum) - expected)
    # and on the device: every form has a row that runs there
    assert {c.form for c in CC.GPU_CASES if c.form} == set(enum)
    # each epilogue variant that a descriptor can reach (DCM2's fast epilogues cannot: the configuration only takes Cout % 32 != 0,
    # which the fast epilogues exclude)
    variants = {}
    for c in CC.CASES:
        if c.form:
            variants.setdefault(c.form, set()).add(c.epi)
    for form in ("K3S2M1", "K3S2M2", "K5M1", "K7M1", "P3M1S", "P3S2M1S", "P3D2M1S"):
        assert variants[form] == {0, 1, 2}, form
    assert variants["DCM1"] == {0, 1, 2, 3, 4, 5} and variants["DCM1_V8"] >= {0, 1, 2, 3} and variants["DCP"] == {0, 1, 2}
    assert variants["WINO_N3"] == {0, 1, 2, 3, 4, 8, 12} and variants["WINO_S2_PIPE4"] == {0, 1, 12}
    for form in ("WINO_N", "WINO_N8", "WINO"):
        assert variants[form] >= {0, 3}, form


def test_every_bound_is_one_of_the_two_the_suite_holds():
    for c in CC.CASES:
        assert c.bound == ("WINO7" if c.form == "WINO_K7" else "TIGHT"), c


def test_binding_matches_the_header():
    from snvc_amd import _forms
    params = re.search(r"SNVC_API[^;(]*\bsnvc_conv3d_forward_form\s*\(([^)]*)\)", HEADER).group(1)
    assert len(_forms.SIGNATURES["snvc_conv3d_forward_form"][1]) == params.count(",") + 1 == 8
    assert len(_forms.CONV_FWD_INFO) == _forms.INFO and _forms.lib().snvc_forms_abi_version() == _forms._ABI == 4
    entries = _forms.enum_names(HEADER, "CFE")
    assert entries == {"FORWARD": _forms.ENTRY_FORWARD, "HEAD": _forms.ENTRY_HEAD, "SIDE_HEAD": _forms.ENTRY_SIDE_HEAD,
                       "STATS": _forms.ENTRY_STATS} and {k.upper(): v for k, v in CC.ENTRIES.items()} == entries
