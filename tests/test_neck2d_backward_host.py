"""tests/neck2d_backward_cases.py without a GPU: the table covers what the code can take, its float64 reference is reproduced by
torch's own float32 autograd to a tenth of the tolerance the GPU test allows, and the ReLU masks stay small.

Measured here (max error over max |reference|, float32 CPU autograd against the float64 reference): see
profiles/neck2d_backward/measured_errors.txt.
"""
import itertools

import pytest
import torch

import neck2d_backward_cases as NB


def test_the_table_reaches_every_combination_the_code_can_take():
    have = {(r.kind, r.norm, r.act, r.residual) for r in NB.ROWS}
    want = {c for c in itertools.product(NB.KINDS, NB.NORMS, NB.ACTS, NB.RESIDUALS) if NB.can_take(*c)}
    assert want <= have, sorted(want - have)
    # what is left out of the product is left out by name
    left_out = set(itertools.product(NB.KINDS, NB.NORMS, NB.ACTS, NB.RESIDUALS)) - want
    assert all(k == NB.DECONV and (n == "bias" or a not in NB.DECONV_ACTS or r not in NB.DECONV_RESIDUALS) for k, n, a, r in left_out)
    assert "deconv_bias" in NB.REFUSED and {"bias_with_norm", "dilated_training", "out_training"} <= set(NB.REFUSED)
    assert len({r.name for r in NB.ROWS}) == len(NB.ROWS)


def test_the_named_rows_are_the_ones_the_backward_decides_on():
    """Each host decision of ``_Conv2dNormActFn.backward`` has its row: odd extents through both stride-2 kinds, ragged widths, the
    residual forms, every ``needs`` variant, the forced Winograd form, the transposed input."""
    by = NB.BY_NAME
    odd = lambda r: r.h % 2 == 1 or r.w % 2 == 1      # noqa: E731
    assert odd(by["k1s2_odd_bn_relu"]) and by["k1s2_odd_bn_relu"].h % 2 and by["k1s2_odd_bn_relu"].w % 2
    assert by["k3s2_odd_bn_relu"].h % 2 and by["k3s2_odd_bn_relu"].w % 2
    assert by["k3s2_odd_w_frozen_res"].h % 2 == 0 and by["k3s2_odd_w_frozen_res"].w % 2 == 1
    assert all(by[n].cin % 8 or by[n].cout % 8 for n in ("k1s1_ragged_bn_relu_res", "k1s2_odd_bn_relu", "k3s1_ragged_bn_relu_res",
                                                         "k3s2_odd_bn_relu", "deconv_bn_relu_res"))
    assert (by["k1s2_frozen_res_no_act"].act, by["k1s2_frozen_res_no_act"].residual) == ("none", "before")
    assert (by["k3s1_gn_relu_res_after"].norm, by["k3s1_gn_relu_res_after"].residual) == ("gn", "after")
    assert by["deconv_gn_relu_res_n1"].n == 1 and by["whole_bias_sigmoid"].n == 3
    assert by["k3s1_wino_bn_relu_res"].variant == "ALGO_WINO_TILE_BIG" and min(by["k3s1_wino_bn_relu_res"].h, by["k3s1_wino_bn_relu_res"].w) >= 32
    variants = [r for r in NB.ROWS if r.same_as]
    assert {r.needs for r in variants} == {frozenset(("residual",)), frozenset(("weight", "affine", "residual")), frozenset(("x", "residual"))}
    for r in variants:
        base = by[r.same_as]
        assert base.needs == NB.ALL and r._replace(name="", needs=base.needs, pins="", same_as=None) == base._replace(name="", pins="")
        a, b = NB.build(r), NB.build(base)
        assert all(torch.equal(a[k], b[k]) for k in a)
    assert by["k3s1_transposed_input"].transposed_input and by["k3s1_transposed_input"].h != by["k3s1_transposed_input"].w


@pytest.mark.parametrize("row", NB.ROWS, ids=[r.name for r in NB.ROWS])
def test_the_reference_is_float32_reproducible_and_the_mask_is_small(row):
    data = NB.build(row)
    ref = NB.reference(row, data)
    assert ref["masked"] <= NB.MASK_CAP and (row.act == "relu" or ref["masked"] == 0.0), ref["masked"]
    assert set(NB.requested(row)) <= set(ref) and all(ref[k] is not None for k in NB.requested(row))
    f32 = NB.evaluate(row, data, torch.float32, ref["gy"])
    errs = {k: NB.rel_err(f32[k], ref[k]) for k in ["y"] + NB.requested(row)}
    print(f"{row.name}: masked {100 * ref['masked']:.2f} %; float32 CPU vs float64: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))
    assert max(errs.values()) <= NB.F32_CAP, errs
    if NB.residual_gradient_is_gy(row) and "residual" in row.needs:
        assert torch.equal(ref["dres"].float(), ref["gy"])


@pytest.mark.parametrize("c", NB.COMPOSITIONS, ids=[c.name for c in NB.COMPOSITIONS])
def test_composition_references(c):
    """Internal pre-activations keep ``INTERNAL_MARGIN`` from zero in float64; the last ReLU is masked through gy; float32 reproduces."""
    ref = NB.comp_reference(c)
    margin = min((float(t.abs().min()) for t in ref["internal"]), default=float("inf"))
    count = sum(t.numel() for t in ref["internal"])
    assert margin >= NB.INTERNAL_MARGIN, (margin, count)
    assert ref["masked"] <= NB.MASK_CAP, ref["masked"]
    if c.what != "fuse_sum":
        assert count >= 200, "a composition has internal ReLUs"
    f32 = NB.comp_evaluate(c, torch.float32, ref["gy"])
    errs = {"y": max(NB.rel_err(a, b) for a, b in zip(f32["ys"], ref["ys"]))}
    for i, (a, b) in enumerate(zip(f32["dx"], ref["dx"])):
        assert (a is None) == (b is None) == (i == c.frozen)
        if b is not None:
            errs[f"dx{i}"] = NB.rel_err(a, b)
    wanted = {k for k, v in ref.get("params", {}).items() if v is not None}
    if c.what == "fuse_row":            # only row FUSE_ROW reaches the loss
        assert wanted and all(k.startswith(f"fuse_layers.{NB.FUSE_ROW}.") for k in wanted)
    for k in wanted:
        errs[k] = NB.rel_err(f32["params"][k], ref["params"][k])
    print(f"{c.name}: {count} internal pre-activations, nearest to zero {margin:.2e}; masked {100 * ref['masked']:.2f} %; "
          f"float32 CPU vs float64 worst {max(errs.values()):.1e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) <= NB.F32_CAP, errs
