"""CPU checks of the weight gradient's plan (plan_wgrad in csrc/conv3d_bwd.hip, asked through snvc_conv3d_wgrad_form of
include/snvc_forms.h): the workspace query against what the ladder-shaped dispatcher before it returned (tests/golden/
wgrad_workspace_table.json, recorded by tests/golden/make_golden_wgrad_plan.py), and the form column of tests/wgrad_cases.py
against the plan the launcher itself makes.  No GPU: without a device the CU count falls back to 256, which is also an MI355X's
own count; the recorded bytes and the literal plan numbers are those of 256 CUs.
"""
import ctypes
import json
import os
import re

import pytest

import wgrad_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "snvc_forms.h")).read()
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "wgrad_workspace_table.json")))
CUS = 256


def _enum():
    from snvc_amd import _forms
    return _forms.enum_names(HEADER, "WG")


def _workspace_bytes(fields):
    from snvc_amd import _lib
    return int(_lib.lib().snvc_conv3d_wgrad_workspace_bytes(ctypes.byref(WC.make_desc(fields)) if fields is not None else None))


def _query(group, name, variant, x_align=16, g_align=16):
    from snvc_amd import _forms
    return _forms.conv3d_wgrad(WC.make_desc(WC.case_desc_fields(group, name, variant)), x_align, g_align)


# ======================================================================================================== (a) workspace golden
def test_workspace_bytes_of_every_case_are_the_recorded_ones():
    assert GOLDEN["fields"] == list(WC.DESC_FIELDS)
    assert [(g, n) for g, n, _ in GOLDEN["cases"]] == WC.all_cases()
    for g, n, nbytes in GOLDEN["cases"]:
        for variant in WC.VARIANTS:
            assert _workspace_bytes(WC.case_desc_fields(g, n, variant)) == nbytes, (g, n, variant)


def test_workspace_bytes_of_the_sweep_are_the_recorded_ones():
    sweep = WC.sweep_desc_fields()
    assert len(sweep) == len(GOLDEN["sweep"]) == 200
    for fields, row in zip(sweep, GOLDEN["sweep"]):
        assert [fields[k] for k in WC.DESC_FIELDS] == row[:-1]
        assert _workspace_bytes(fields) == row[-1], fields


@pytest.mark.parametrize("what", sorted(WC.refusal_desc_fields()))
def test_descriptor_refusals_are_the_recorded_ones(what):
    """Status and text of the launcher (null pointers: nothing can be launched) and of the query, and the workspace query's answer."""
    from snvc_amd import _forms, _lib
    fields = WC.refusal_desc_fields()[what]
    status, text, nbytes = GOLDEN["refusals"][what]
    assert status != 0
    d = ctypes.byref(WC.make_desc(fields)) if fields is not None else None
    L = _lib.lib()
    assert L.snvc_conv3d_wgrad_amax(d, None, None, None, None, None, None, None) == status
    assert L.snvc_last_error_string().decode() == text
    assert L.snvc_conv3d_wgrad(d, None, None, None, None, None) == status and L.snvc_last_error_string().decode() == text
    assert _workspace_bytes(fields) == nbytes
    if text.endswith("null pointer"):          # the query does not see pointers: this descriptor is accepted
        assert _forms.conv3d_wgrad(WC.make_desc(fields))[0] > 0
    else:
        info = (ctypes.c_int64 * _forms.INFO)(*([7] * _forms.INFO))
        assert _forms.lib().snvc_conv3d_wgrad_form(d, 16, 16, ctypes.cast(info, ctypes.c_void_p)) == -status
        assert L.snvc_last_error_string().decode() == text and not any(info)


def test_later_refusals_keep_the_launchers_code_and_text():
    """The checks behind the pointer check, through the query: sample size, channel pairs, unsupported keys, bad alignment values."""
    from snvc_amd import _forms
    rc, info, text = _forms.conv3d_wgrad(WC.make_desc(WC.desc_fields((1, 2, 1, (1024, 1024, 1024), 1, 1, 1))))
    assert rc == -2 and text == "snvc_conv3d_wgrad: one sample must stay below 2^31 elements" and not any(info.values())
    rc, _, text = _forms.conv3d_wgrad(WC.make_desc(WC.desc_fields((1, 32 * 256, 32 * 256, (1, 1, 4), 1, 1, 1))))
    assert rc == -2 and text == "snvc_conv3d_wgrad: too many channel pairs"
    for case in WC.UNSUPPORTED_CASES.values():
        rc, _, text = _forms.conv3d_wgrad(WC.make_desc(WC.desc_fields(case)))
        assert rc == -2 and text.startswith("snvc_conv3d_wgrad: (ksize,stride,dilation) not in")
    rc, _, text = _forms.conv3d_wgrad(WC.make_desc(WC.desc_fields(WC.DEPTH1_CASES["k3 d1"])), 12, 16)
    assert rc == -1 and text.startswith("snvc_conv3d_wgrad_form:")


# ======================================================================================================== (b) the form column
@pytest.mark.parametrize("variant", WC.VARIANTS)
@pytest.mark.parametrize("case", WC.all_cases(), ids=lambda c: f"{c[0]}: {c[1]}")
def test_the_form_column_states_what_the_launcher_plans(case, variant):
    group, name = case
    names = {v: k for k, v in _enum().items()}
    promised = _workspace_bytes(WC.case_desc_fields(group, name, variant))
    for xa in WC.ALIGNMENTS:
        for ga in WC.ALIGNMENTS:
            rc, info, text = _query(group, name, variant, xa, ga)
            assert rc > 0, (xa, ga, text)
            form = names[rc]
            assert form == WC.expected_form(group, name, variant, xa, ga), (xa, ga)
            assert 0 < info["ws_bytes"] <= promised, (xa, ga, form)       # a launch never outgrows what the query promised
            assert info["piece_bytes"] in (16, 8, 4) and info["grid_x"] > 0 and info["grid_yz"] > 0 and info["threads"] > 0
            numbers = WC.expected_numbers(group, name, variant, form, CUS)
            if numbers is not None:
                assert (info["parts"], info["per_part"]) == tuple(numbers), (xa, ga, form)
            if (xa, ga) == (16, 16):
                literal = WC.PLAN_256.get(case, {}).get(variant)
                assert (literal is not None) == (form in WC.SPLIT_FORMS + WC.UNIT_FORMS + ("K1_STREAM",)), form
                if literal is not None:
                    assert (info["parts"], info["per_part"]) == literal
                assert info["piece_bytes"] == WC.PIECE_BYTES.get(case, {}).get(variant, 4 if form == "TAPS" else 16)


def test_the_depth_part_and_pair_cases_still_cover_what_they_are_for():
    for name, (c, parts256, last256) in WC.DPART_CASES.items():
        _, info, _ = _query("dparts", name, "auto")
        assert info["parts"] == parts256 > 1 and c[3][0] // c[5] - (parts256 - 1) * info["per_part"] == last256
    for name, c in WC.PAIRS_CASES.items():
        _, info, _ = _query("pairs", name, "fp32")
        assert info["parts"] == 1 and 8 * info["per_part"] >= WC.channel_pairs(c[1], c[2]) > WC.wgrad_unit_count(CUS)


def test_the_column_limits_sit_where_the_new_cases_say():
    """One column fewer and the layer keeps its split-operand form: 256 columns of 4 x 32 voxels, 512 of 2 x 32 at stride 2."""
    from snvc_amd import _forms
    enum = _enum()
    for name, th, form, below in (("k3 257 columns", 4, "WINO", "X3"), ("k3s2 513 columns", 2, "S2", "X3S2")):
        n, cin, cout, (d, h, w), k, stride, dil = WC.COLUMN_LIMIT_CASES[name]
        assert _query("columns", name, "auto")[0] == enum[form]
        fewer = (n, cin, cout, (d, h - th * stride, w), k, stride, dil)
        assert _forms.conv3d_wgrad(WC.make_desc(WC.desc_fields(fewer)))[0] == enum[below]


# ======================================================================================================== (c) enum and binding
def test_every_form_of_the_header_is_reached_by_an_accepted_row():
    enum = _enum()
    assert sorted(enum.values()) == list(range(1, 8)) and len(enum) == 7
    taken = {}
    for group, name in WC.all_cases():
        for variant in WC.VARIANTS:
            for xa, ga in ((16, 16), (16, 8), (4, 4)):
                rc, info, _ = _query(group, name, variant, xa, ga)
                taken.setdefault(rc, set()).add(info["piece_bytes"])
    assert set(taken) == set(enum.values())
    assert 8 in taken[enum["X3"]] and 16 in taken[enum["X3"]]             # both row variants of the split-operand kernel
    assert 8 in taken[enum["KSPLIT"]] and 16 in taken[enum["KSPLIT"]]     # vec == 2 and vec == 4
    assert set(WC.FORMS) == set(WC.all_cases()) and {f for e in WC.FORMS.values() for v in e.values() for f in v} == set(enum)


def test_binding_matches_the_header():
    from snvc_amd import _forms
    params = re.search(r"SNVC_API[^;(]*\bsnvc_conv3d_wgrad_form\s*\(([^)]*)\)", HEADER).group(1)
    assert len(_forms.SIGNATURES["snvc_conv3d_wgrad_form"][1]) == params.count(",") + 1 == 4
    assert len(_forms.WGRAD_INFO) == _forms.INFO and _forms.lib().snvc_forms_abi_version() == _forms._ABI == 4
