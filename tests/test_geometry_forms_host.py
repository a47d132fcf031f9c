"""CPU checks of the geometry launchers' form decisions (include/snvc_forms.h): the binding against the header, and the case table
of tests/geometry_cases.py against the library's own decision functions -- the ones the launchers call.  No GPU: without a device
the CU count falls back to 256, and no number in the table depends on it.
"""
import os
import re

import pytest

import geometry_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "snvc_forms.h")).read()


def _enum(entry):
    from snvc_amd import _forms
    return _forms.enum_names(HEADER, GC.ENUM_PREFIX[entry])


def test_header_and_binding_agree():
    """The info slots and the gather kinds; names, parameters and the ABI numbers are held by tests/test_abi_tables_host.py."""
    from snvc_amd import _forms
    assert int(re.search(r"SNVC_FORMS_INFO = (\d+)", HEADER).group(1)) == _forms.INFO
    for info in (_forms.CV_FWD_INFO, _forms.CV_BWD_INFO, _forms.GATHER_FWD_INFO, _forms.GATHER_BWD_INFO, _forms.WGRAD_INFO,
                 _forms.CONV_FWD_INFO, _forms.FIRST_LAYER_INFO):
        assert len(info) == _forms.INFO
    assert {k: v for k, v in _forms.enum_names(HEADER, "GATHER").items()} == {"F32": 0, "C8": 1, "SPLIT": 2} == {k.upper(): v for k, v in GC.KIND.items()}


@pytest.mark.parametrize("c", [c for c in GC.CASES if c.form is not None], ids=str)
def test_the_table_states_what_the_launcher_decides(c):
    """Form and launch numbers of every accepted row, with every operand 16-byte aligned."""
    rc, info, text = GC.query(c)
    names = {v: k for k, v in _enum(c.entry).items()}
    assert rc > 0 and names[rc] == c.form, (rc, text)
    assert {k: info[k] for k in c.info} == c.info


@pytest.mark.parametrize("c", [c for c in GC.CASES if c.form is not None], ids=str)
def test_the_second_placement_of_the_guard_suite_keeps_the_form(c):
    """tests/test_gpu_guard_ops.py places the operands ``place`` bytes off a 256-byte boundary: 16 keeps everything aligned; at 4 the
    operands the test places are not 16-byte aligned (outputs and workspaces, which the wrappers allocate, still are) and the form must be the same."""
    from snvc_amd import _forms
    assert c.place in (4, 16)
    aligned = _forms.ALIGNED_ALL if c.place == 16 else _forms.ALIGNED_OUT
    assert GC.query(c, aligned)[0] == GC.query(c)[0]
    if c.place == 16 and c.kind == "f32":          # and 16 is needed: off alignment the row would take another form (the 8-channel
        assert GC.query(c, _forms.ALIGNED_OUT)[0] != GC.query(c)[0]        # LDS forms fetch one coordinate per lane and would not)


def test_every_form_id_of_the_header_is_taken_by_an_accepted_row():
    for entry, prefix in GC.ENUM_PREFIX.items():
        enum = _enum(entry)
        assert len(enum) >= 3 and sorted(enum.values()) == list(range(1, len(enum) + 1)), (prefix, enum)
        taken = {c.form for c in GC.BY_ENTRY[entry] if c.form is not None}
        assert taken == set(enum), (prefix, taken ^ set(enum))
        for c in GC.BY_ENTRY[entry]:
            if c.form is not None:
                assert GC.query(c)[0] == enum[c.form], c.name


@pytest.mark.parametrize("c", [c for c in GC.CASES if c.form is None], ids=str)
def test_refusals_come_back_with_the_launchers_code_and_text(c):
    rc, info, text = GC.query(c)
    status, start = c.refusal
    entry_point = start.split(":")[0]
    assert rc == -status and text.startswith(start) and entry_point.startswith("snvc_") and entry_point in text
    assert not any(info.values())


def test_queries_for_empty_and_invalid_sizes():
    """0 = the launcher returns SNVC_OK without a launch; sizes the entry points refuse come back as -(status) with their text."""
    from snvc_amd import _forms
    assert _forms.cost_volume_forward(0, 2, 4, 8, 3, 1, GC.F32)[0] == 0
    assert _forms.cost_volume_forward(1, 2, 4, 8, 0, 1, GC.F32, right_only=True)[0] == 0
    rc, _, text = _forms.cost_volume_forward(1, 1, 3, 4, 1, 2, GC.F32)
    assert rc == -1 and "multiples of downsample" in text
    rc, _, text = _forms.cost_volume_forward(1, 1, 4, 4, 1, 1, 7)
    assert rc == -2 and "dtype" in text
    assert _forms.cost_volume_backward(1, 0, 4, 8, 3, 1, GC.F32)[0] == 0
    assert _forms.cost_volume_backward(1, 1, 4, 8, 3, 0, GC.F32)[0] == -1
    assert _forms.voxel_gather_forward(GC.KIND["f32"], 0, 8, 7, 9, 100, GC.ODD)[0] == 0
    rc, _, text = _forms.voxel_gather_forward(GC.KIND["c8"], 1, 12, 7, 9, 100, GC.ODD)
    assert rc == -1 and text.startswith("snvc_voxel_gather_forward_f16: bad sizes")
    rc, _, text = _forms.voxel_gather_forward(GC.KIND["c8"], 1, 8, 7, 9, 100, GC.ODD, aligned=_forms.ALIGNED_IN)
    assert rc == -1 and "16-byte aligned" in text
    assert _forms.voxel_gather_forward(3, 1, 8, 7, 9, 100, GC.ODD)[0] == -1
    # fp32 gather without an aligned workspace, or with F % 4 != 0: the plain kernel
    plain = _enum("gather_fwd")["PLAIN"]
    assert _forms.voxel_gather_forward(GC.KIND["f32"], 2, 8, 7, 9, 332, GC.ODD, aligned=_forms.ALIGNED_IN)[0] == plain
    assert _forms.voxel_gather_backward(1, 3, 6, 6, 0, True)[0] == 0 == _forms.voxel_gather_backward(1, 3, 6, 6, 0, False)[0]
    rc, _, text = _forms.voxel_gather_backward(40000, 3, 6, 6, 10, True)
    assert rc == -2 and text.startswith("snvc_voxel_gather_backward_det: batch")
    rc, _, text = _forms.voxel_gather_backward(70000, 3, 6, 6, 10, False)
    assert rc == -2 and text.startswith("snvc_voxel_gather_backward: feature plane or batch")


def test_thresholds_of_the_decisions():
    """Each threshold between two forms, one step to either side."""
    from snvc_amd import _forms
    cvf, cvb, gf, gb = (_enum(e) for e in ("cv_fwd", "cv_bwd", "gather_fwd", "gather_bwd"))
    assert _forms.cost_volume_forward(1, 1, 2, 2048, 3, 1, GC.F32)[0] == cvf["ROWS"]
    assert _forms.cost_volume_forward(1, 1, 2, 2052, 3, 1, GC.F32)[0] == cvf["F32X4"]
    assert _forms.cost_volume_forward(1, 1, 2, 2052, 3, 1, GC.F32, aligned=0)[0] == cvf["GENERIC_F32"]
    assert _forms.cost_volume_forward(1, 1, 2, 2052, 3, 1, GC.F32, right_only=True)[0] == -2
    # depth split: D / (2 * dsplit) >= 8 asks for D >= 16 for the first split, and a full grid (N*C*hblocks >= 2048) stops it
    assert _forms.cost_volume_forward(1, 2, 6, 312, 15, 1, GC.F32)[1]["dsplit"] == 1
    assert _forms.cost_volume_forward(1, 2, 6, 312, 16, 1, GC.F32)[1]["dsplit"] == 2
    assert _forms.cost_volume_forward(1, 2, 6, 312, 200, 1, GC.F32)[1]["dsplit"] == 16
    assert _forms.cost_volume_forward(8, 128, 8, 312, 200, 1, GC.F32)[1]["dsplit"] == 1
    # the plane walk's grid limit
    assert _forms.cost_volume_forward(6, 32, 1, 3, 200, 1, GC.F32)[1]["grid_y"] == 65535
    assert _forms.cost_volume_forward(5, 32, 1, 3, 200, 1, GC.F32)[1]["grid_y"] == 64000
    assert _forms.cost_volume_backward(1, 1, 3, 2, 4, 1, GC.F32)[0] == cvb["ROWS"]
    assert _forms.cost_volume_backward(1, 1, 3, 1, 4, 1, GC.F32)[0] == cvb["GATHER_F32"]
    assert _forms.cost_volume_backward(1, 1, 3, 2, 4, 1, GC.F64)[0] == cvb["GATHER_F64"]
    # LDS forms: V >= 4096 and the plane's capacity (4608 pixels in both slice widths)
    for kind, lds, other in (("f32", "LDS", "CL_X4"), ("c8", "LDS_C8", "CL_C8")):
        k = GC.KIND[kind]
        assert _forms.voxel_gather_forward(k, 1, 8, 64, 72, 4096, GC.ODD)[0] == gf[lds]
        assert _forms.voxel_gather_forward(k, 1, 8, 64, 72, 4092, GC.ODD)[0] == gf[other]
        assert _forms.voxel_gather_forward(k, 1, 8, 1, 4609, 4096, GC.ODD)[0] == gf[other]
    # the run grows in whole 4096-voxel steps once V exceeds 4096 runs' worth of workgroups
    big = _forms.voxel_gather_forward(GC.KIND["f32"], 1, 32, 64, 64, 32 * 128 * 192, GC.POW2)[1]
    assert big["run"] % 4096 == 0 and big["run"] * big["nruns"] >= 32 * 128 * 192 > big["run"] * (big["nruns"] - 1)
    # adjoint: two planes of 8192 pixels are exactly 64 KiB
    assert _forms.voxel_gather_backward(1, 2, 64, 128, 500, False)[0] == gb["LDS_ATOMICS"]
    assert _forms.voxel_gather_backward(1, 2, 64, 129, 500, False)[0] == gb["GLOBAL_ATOMICS"]
    assert _forms.voxel_gather_backward(1, 64, 7, 9, 500, True)[1]["passes"] == 1
    assert _forms.voxel_gather_backward(1, 65, 7, 9, 500, True)[1]["passes"] == 2
