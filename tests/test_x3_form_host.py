"""CPU checks of the split-mode launch-size rule ``ops.x3_form``: which of the five kernel forms a layer gets at a launch size.
The constants in the rule were measured on hardware, and a slip in it would only show as a slower, still-correct benchmark, so it
is held row by row to tests/golden/x3_form_table.json -- what the rule returned while it was still a method of
``Conv3dLayerX3`` (tests/golden/make_golden_x3_form.py, run at that commit)."""
import itertools
import json
import os

import pytest

from snvc_amd import _lib, ops

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "x3_form_table.json")
KNOBS = ("X3_Q16", "X3_Q16_K5", "X3_Q16_S2")


@pytest.fixture
def default_knobs():
    saved = {k: getattr(ops, k)[0] for k in KNOBS}
    assert saved == dict.fromkeys(KNOBS, True) and ops.X3_Q16_MIN_JOBS == [256] and ops.X3_SMALL_BELOW == {"stride2": 0, "transposed": 4096}, \
        "the table was recorded with the default knobs"
    yield saved
    for k, v in saved.items():
        getattr(ops, k)[0] = v


def test_x3_form_matches_the_recorded_table(default_knobs):
    with open(TABLE) as f:
        gold = json.load(f)
    order, axes, forms, rows = gold["order"], gold["axes"], gold["forms"], gold["rows"]
    assert order == ["knobs", "cout", "ksize", "geometry", "n", "out_sp", "plain", "split_out", "forced"]
    assert forms == [0, _lib.ALGO_X3_SERIAL, _lib.ALGO_X3_NARROW, _lib.ALGO_X3_SMALL, _lib.ALGO_X3_Q16]
    grid = list(itertools.product(*(axes[k] for k in order)))
    assert len(grid) == len(rows) and set(rows) == set("01234")
    wrong = []
    for (knobs, cout, ksize, (stride, transposed, dilation), n, out_sp, plain, split_out, forced), digit in zip(grid, rows):
        for k, v in default_knobs.items():
            getattr(ops, k)[0] = knobs.get(k, v)
        got = ops.x3_form(cout, ksize, stride, dilation, transposed, n, tuple(out_sp), plain, split_out, forced)
        if got != forms[int(digit)]:
            wrong.append((knobs, cout, ksize, stride, transposed, dilation, n, out_sp, plain, split_out, forced, got, forms[int(digit)]))
    assert not wrong, f"{len(wrong)} of {len(rows)} rows differ; the first: {wrong[:5]}"


def test_x3_form_depends_on_its_arguments_only(default_knobs):
    """The same arguments give the same form whatever was asked in between (the rule once fell back to the form of the last launch)."""
    a = (32, 3, 1, 1, False, 2, (8, 12, 40), False, False, None)           # 24 tiles, a residual: half-height tiles
    b = (64, 3, 2, 1, True, 2, (8, 12, 40), False, False, None)            # a transposed layer below 4096 workgroups
    c = (64, 5, 1, 1, False, 1, (2, 2, 3), True, True, None)               # 5^3 below 512 jobs: the default form
    d = (8, 3, 1, 1, False, 1, (2, 2, 3), False, False, None)              # Cout % 32 != 0: nothing to pick from
    first = [ops.x3_form(*args) for args in (a, b, c, d)]
    assert first == [_lib.ALGO_X3_SMALL, _lib.ALGO_X3_SMALL, 0, _lib.ALGO_X3_SMALL]
    others = [(32, 3, 1, 1, False, 1, (192, 96, 312), True, True, None), (64, 3, 2, 1, False, 1, (96, 48, 156), True, True, None),
              (64, 3, 1, 1, False, 1, (96, 48, 156), False, False, None), (96, 3, 1, 1, False, 1, (96, 48, 156), False, False, None),
              (32, 3, 1, 1, False, 1, (2, 2, 3), False, False, _lib.ALGO_X3_Q16), (32, 7, 1, 1, False, 1, (96, 48, 156), True, True, None)]
    assert [ops.x3_form(*args) for args in others] == [_lib.ALGO_X3_Q16, _lib.ALGO_X3_Q16, _lib.ALGO_X3_SERIAL, _lib.ALGO_X3_NARROW,
                                                      _lib.ALGO_X3_Q16, _lib.ALGO_X3_Q16]
    for args, form in zip((d, c, b, a), reversed(first)):
        for other in others:
            ops.x3_form(*other)
            assert ops.x3_form(*args) == form
    # the geometries the rule does not cover give 0 unless a form is forced -- never what an earlier call picked
    for args in ((1, 3, 1, 1, False, 1, (192, 96, 312), True, True), (32, 3, 2, 1, False, 2, (8, 12, 40), True, True),
                 (8, 5, 1, 1, False, 1, (16, 32, 512), False, False)):
        ops.x3_form(*others[0])
        assert ops.x3_form(*args, None) == 0
        assert ops.x3_form(*args, _lib.ALGO_X3_SMALL) == _lib.ALGO_X3_SMALL and ops.x3_form(*args, 0) == 0
