"""CPU check of the host side of snvc_amd/csrc/conv3d_f16.hip: which kernel form a descriptor gets shows in the packed weight bytes of
the fp16-storage and the split route and in the statistics workspace's bytes, and a rejected descriptor in its error text.  All of it
is held row by row to tests/golden/f16_plan_table.json -- what the library returned while the forms were an enum, spread over lists
and switches (tests/golden/make_golden_f16_plan.py, run against that commit's library).  The calls take a descriptor, or null
pointers that are refused before anything is launched: no device is needed."""
import json
import os
import re

import pytest

import f16_plan_cases as C
from snvc_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(HERE, "golden", "f16_plan_table.json")) as f:
        g = json.load(f)
    assert g["fields"] == C.FIELDS and g["probes"] == C.PROBES
    return g


def test_plan_decisions_match_the_recorded_table(gold):
    L = _lib.lib()
    nf = len(C.FIELDS)
    assert [row[:nf] for row in gold["rows"]] == [[f[k] for k in C.FIELDS] for _, f in C.plan_cases()]     # the table is the cases' record
    wrong = []
    for row in gold["rows"]:
        got = C.probe(L, dict(zip(C.FIELDS, row[:nf])))
        if got != row[nf:]:
            wrong.append((row[:nf], got, row[nf:]))
    assert not wrong, f"{len(wrong)} of {len(gold['rows'])} rows differ; the first: {wrong[:5]}"
    for name in C.PROBES:
        assert getattr(L, name)(None) == -1


def test_the_table_reaches_every_form_record(gold):
    """Every FORM_<name> record of conv3d_f16.hip is listed in f16_plan_cases.FORMS with a (key, Cout, algo) that selects it, and the
    table holds an accepted row for each; the rejections are there with their texts."""
    with open(os.path.join(os.path.dirname(HERE), "snvc_amd", "csrc", "conv3d_f16.hip")) as f:
        records = re.findall(r"^constexpr F16Form FORM_(\w+)\s*=", f.read(), re.M)
    assert len(records) == len(set(records)) and set(records) == set(C.FORMS)
    nf = len(C.FIELDS)
    seen = set()
    for row in gold["rows"]:
        d = dict(zip(C.FIELDS, row[:nf]))
        key = (d["ksize"], d["stride"], d["dilation"]) + ((1,) if d["transposed"] else ())
        for split, value in ((False, row[nf]), (True, row[nf + 2])):
            if value >= 0:
                seen.add((split, key, d["Cout"], d["algo"]))
    for name, (split, key, cout, algo) in C.FORMS.items():
        assert (split, tuple(key), cout, algo) in seen, name
    rejected = [row for row in gold["rows"] if row[nf] < 0 and row[nf + 2] < 0]
    texts = {row[nf + 1] for row in rejected} | {row[nf + 3] for row in rejected}
    assert len(rejected) >= 40 and len(texts) >= 14
    assert all(t.startswith(("snvc_f16_conv3d: ", "snvc_f16x3_conv3d: ")) for t in texts)
