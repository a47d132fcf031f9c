"""CPU check of ``snvc_conv3d_packed_weight_count``: the packed fp32 weight buffer is [direct MFMA packing][Winograd packing]
[raw tail], and the packer, the count and the forward dispatcher must agree on where each section lies.  The count is held row by
row to tests/golden/packed_count_table.json -- what the function returned while each of the three still spelled the layout out
by hand (tests/golden/make_golden_packed_count.py, run against that commit's library).  The calls take a descriptor only: nothing
is launched, no pointer is passed."""
import ctypes
import json
import os

from snvc_amd import _lib

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_count_table.json")
CHANNELS = {1, 2, 3, 31, 32, 33, 64, 96}


def _table():
    with open(TABLE) as f:
        gold = json.load(f)
    assert gold["fields"] == ["N", "Cin", "Din", "Hin", "Win", "Cout", "Dout", "Hout", "Wout", "ksize", "stride", "dilation", "pad",
                              "transposed", "ksize_d", "ksize_h"]
    return gold["fields"], gold["rows"]


def test_packed_weight_count_matches_the_recorded_table():
    fields, rows = _table()
    L = _lib.lib()
    wrong = []
    for row in rows:
        desc = dict(zip(fields, row))
        want = row[len(fields)]
        got = L.snvc_conv3d_packed_weight_count(ctypes.byref(_lib.Conv3dDesc(**desc)))
        if got != want:
            wrong.append((desc, got, want))
        elif want < 0 and L.snvc_last_error_string().decode() != row[len(fields) + 1]:
            wrong.append((desc, L.snvc_last_error_string().decode(), row[len(fields) + 1]))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ; the first: {wrong[:5]}"
    assert L.snvc_conv3d_packed_weight_count(None) == -1


def test_the_table_covers_every_plan_key():
    """The table is only worth what it covers: every key of make_plan with every channel count, and the rejections."""
    fields, rows = _table()
    seen = {}
    for row in rows:
        d = dict(zip(fields, row))
        if row[len(fields)] >= 0:
            key = (d["transposed"], d["ksize_d"], d["ksize"], d["stride"], d["dilation"], d["ksize_h"])
            seen.setdefault(key, set()).add((d["Cout"], d["Cin"]))
    cubic = {(0, 0, k, s, dil, 0) for k, s, dil in ((1, 1, 1), (3, 1, 1), (3, 2, 1), (5, 1, 1), (5, 1, 2), (7, 1, 1))}
    planar = {(0, 1, k, s, dil, kh) for k, s, dil, kh in ((1, 1, 1, 0), (1, 2, 1, 0), (3, 1, 1, 0), (3, 1, 1, 3), (3, 2, 1, 0), (7, 1, 1, 3),
                                                          (3, 1, 2, 0))}
    transposed = {(1, 0, 3, 2, 1, 0), (1, 1, 3, 2, 1, 0)}
    assert cubic | planar | transposed <= set(seen)
    for key in cubic | planar | transposed:
        assert {(co, ci) for co in CHANNELS for ci in CHANNELS} <= seen[key], key
    rejected = [row for row in rows if row[len(fields)] < 0]
    assert all(row[len(fields)] == -1 and row[len(fields) + 1].startswith("snvc_conv3d: ") for row in rejected)
    assert len(rejected) >= 25 and len({row[-1] for row in rejected}) >= 12
