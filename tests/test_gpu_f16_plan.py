"""The launches behind every kernel form record of snvc_amd/csrc/conv3d_f16.hip, per call kind that the form accepts or rejects:
status, error text and -- for an accepted call -- the sha256 of the packed weights and of every output buffer, held to
tests/golden/f16_plan_gpu.json (tests/golden/make_golden_f16_plan.py --gpu, recorded on an MI355X from the library of the commit
before the forms became records).  The kernels are deterministic and their code is what it was, so equal launch arguments give
equal bits: a mismatch means the host side hands a kernel other arguments, or another kernel.  Shapes: tests/f16_plan_cases.py
(Cin 16, N = 2, more than one tile and a ragged edge).  The fused first layer's route is held by tests/test_gpu_fused_first_layer.py.
One buffer was recorded again later: the scale / shift / mean / var rows of the `stats` call on the twelve cells that accept it, when the
statistics epilogues began to sum in float64 from the first value on (tests/test_gpu_stats_epilogue.py holds their values); the float32
result of that call and every other cell are the first record's."""
import json
import os

import pytest
import torch

import f16_plan_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f16_plan_gpu.json")) as f:
        return json.load(f)


def test_the_record_covers_every_form_and_call_kind(gold):
    assert set(gold) == set(C.FORMS) | {"K3X, x batch stride + 64"}
    for name, cells in gold.items():
        split = C.FORMS[name.split(",")[0]][0]
        assert set(cells) == {"packed"} | set(C.KINDS if split else C.PLAIN_KINDS), name
    accepted = {(name, kind) for name, cells in gold.items() for kind, v in cells.items() if kind != "packed" and v[0] == 0}
    # every form runs at least one call; every call kind is accepted by some form and, but for the plain split call, rejected by another
    assert {name for name, _ in accepted} == set(gold)
    for kind in C.KINDS:
        takes = {name for name, k in accepted if k == kind}
        assert takes and (kind == "split" or takes != {n for n in gold if C.FORMS[n.split(",")[0]][0]}), kind


def _check(name, gold, x_pad=0):
    got = C.run_form(name.split(",")[0], torch, torch.device("cuda:0"), x_pad=x_pad)
    want = gold[name]
    assert set(got) == set(want)
    wrong = {k: (got[k], want[k]) for k in got if (got[k] if k == "packed" else list(got[k])) != want[k]}
    assert not wrong, wrong


@pytest.mark.parametrize("name", sorted(C.FORMS))
def test_launches_match_the_record(name, gold):
    _check(name, gold)


def test_a_padded_batch_stride_matches_the_record(gold):
    _check("K3X, x batch stride + 64", gold, x_pad=64)
    assert gold["K3X, x batch stride + 64"]["split"][2]["y"] == gold["K3X"]["split"][2]["y"]        # the same values, laid out apart
