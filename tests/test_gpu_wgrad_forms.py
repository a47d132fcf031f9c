"""Every form behind snvc_conv3d_wgrad (csrc/conv3d_bwd.hip) against the float64 weight gradient of tests/wgrad_cases.py (itself
pinned to the kernel's definition by tests/test_wgrad_ref_host.py), at the shapes where its dispatcher changes its mind; and the data
gradient of the k5 / dilated k5 / k7 layers.  The case tables and what each shape is for: tests/wgrad_cases.py.

Every weight-gradient test first asks the library's own plan (snvc_conv3d_wgrad_form, include/snvc_forms.h) which form its shape takes
at its operands' real alignment on this device, and requires the form of the case table's column (wgrad_cases.FORMS): a case that stops
reaching its form fails instead of passing on a sibling.  It then calls ops.conv3d_wgrad twice and requires equal bits (no float atomics: the partial slabs are summed in a
fixed order), then applies test_gpu_parity.check with the project's bounds for the form, relative to max|ref|:
    5e-6  exact-fp32 FMA chains summed in a fixed order: SNVC_ALGO_DIRECT, the generic tap-chunk kernel of the k5 / k5d2 / k7 keys
          under every variant, the k1 streaming form
    2e-5  the Winograd-domain and split-operand forms (and, as in test_conv3d_wgrad_vs_float64, whatever else `auto` / `fp32` reach)
"""
import functools
import os

import numpy as np
import pytest
import torch

import wgrad_cases as WC
from test_gpu_parity import TIGHT, WINO7, check, dev

pytestmark = pytest.mark.gpu

DIRECT_TOL, FORM_TOL = 5e-6, 2e-5


def _bits(variant):
    from snvc_amd import _lib
    return {"auto": 0, "fp32": _lib.ALGO_WGRAD_FP32, "direct": _lib.ALGO_DIRECT}[variant]


def _tol(variant):
    return DIRECT_TOL if variant == "direct" else FORM_TOL


def _wgrad_twice(x_dev, g_dev, args, bits):
    from snvc_amd import ops
    with ops.conv_variant(bits):
        dw = ops.conv3d_wgrad(x_dev, g_dev, *args)
        dw2 = ops.conv3d_wgrad(x_dev, g_dev, *args)
    assert torch.equal(dw, dw2), "the weight gradient is deterministic"
    return dw.cpu().numpy()


def _conv_args(case):
    k, stride, dil = case[4:]
    return k, stride, dil * (k - 1) // 2, dil


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


_HEADER = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snvc_forms.h")).read()


def _align(t):
    return 16 if t.data_ptr() % 16 == 0 else (8 if t.data_ptr() % 8 == 0 else 4)


def _planned(group, case, variant, x_dev, g_dev, algo=None):
    """(form name, info) of the launcher's plan for this case, variant and the operands' real alignment on this device; asserts the
    case table's form and, for the split-operand and 12-wave forms, the restated plan numbers."""
    from snvc_amd import _forms
    fields = WC.case_desc_fields(group, case, variant)
    if algo is not None:
        fields["algo"] = algo
    with torch.cuda.device(x_dev.device):
        rc, info, text = _forms.conv3d_wgrad(WC.make_desc(fields), _align(x_dev), _align(g_dev))
    assert rc > 0, text
    form = {v: k for k, v in _forms.enum_names(_HEADER, "WG").items()}[rc]
    assert form == WC.expected_form(group, case, variant, _align(x_dev), _align(g_dev)), (case, variant, _align(x_dev), _align(g_dev))
    numbers = WC.expected_numbers(group, case, variant, form, _cus() // 8 * 8)
    if numbers is not None:
        assert (info["parts"], info["per_part"]) == tuple(numbers), (case, variant, form)
    return form, info


# ======================================================================================================== k5 / k5d2 / k7
@pytest.mark.parametrize("variant", ["auto", "direct"])
@pytest.mark.parametrize("case", sorted(WC.K57_CASES))
def test_generic_tap_chunk_kernel_vs_float64(case, variant):
    """Keys 511 / 512 / 711: conv3d_wgrad_kernel<WgradCfg<...>>, the only form these keys have, under `auto` and `direct`: two W tiles
    with a narrow second one, H odd against TH = 2, channel blocks of 8 and 24, rows of 16 / 8 / 4 bytes, and for k7 the ragged
    second tap chunk (3 of KHG = 4 kernel rows)."""
    x, g, ref = WC.conv_case("k57", case)
    xd, gd = x.to(dev()), g.to(dev())
    assert _planned("k57", case, variant, xd, gd)[0] == "TAPS"
    got = _wgrad_twice(xd, gd, _conv_args(WC.K57_CASES[case]), _bits(variant))
    check(got, ref.astype(np.float32), DIRECT_TOL, f"wgrad {case} ({variant})")


@pytest.mark.parametrize("case", WC.SCALAR_STAGING_CASES)
def test_generic_kernel_scalar_staging_agrees(case):
    """The 16-byte-row shape of each key with SNVC_ALGO_SCALAR_STAGING: meets the float64 bound, and the two stagings agree to twice
    that bound (each is within it; bit equality is not part of the contract).  Today launch_wgrad gives the tap-split configurations
    scalar staging whatever the rows' alignment -- the vector path is built for the K-split 3x3x3 ones only -- so the flag changes
    nothing for these keys; the case holds the two together should that change."""
    from snvc_amd import _lib
    x, g, ref = WC.conv_case("k57", case)
    args = _conv_args(WC.K57_CASES[case])
    xd, gd = x.to(dev()), g.to(dev())
    assert _planned("k57", case, "auto", xd, gd)[0] == _planned("k57", case, "auto", xd, gd, algo=_lib.ALGO_SCALAR_STAGING)[0] == "TAPS"
    plain = _wgrad_twice(xd, gd, args, 0)
    scalar = _wgrad_twice(xd, gd, args, _lib.ALGO_SCALAR_STAGING)
    check(scalar, ref.astype(np.float32), DIRECT_TOL, f"wgrad {case} (scalar staging)")
    diff = np.abs(scalar.astype(np.float64) - plain.astype(np.float64)).max()
    assert diff <= 2 * DIRECT_TOL * np.abs(ref).max(), f"{case}: the two stagings differ by {diff:.3e}"


# ======================================================================================================== role swap
@pytest.mark.parametrize("variant", ["auto", "fp32", "direct"])
@pytest.mark.parametrize("case", sorted(WC.ROLE_SWAP_CASES))
def test_role_swapped_call_vs_float64_transposed(case, variant):
    """The call _ConvNormActFn.backward makes for a ConvTranspose3d(k3, s2, p1, op1): x := the output gradient on the doubled grid,
    g := the layer's input; the result must be nn.ConvTranspose3d's [Cin_d][Cout_d][27] as it stands."""
    gy_big, x_small, ref = WC.swap_case(case)
    xd, gd = gy_big.to(dev()), x_small.to(dev())
    _planned("swap", case, variant, xd, gd)
    got = _wgrad_twice(xd, gd, (3, 2, 1, 1), _bits(variant))
    assert got.shape == (x_small.shape[1], gy_big.shape[1], 3, 3, 3)
    check(got, ref.astype(np.float32), _tol(variant), f"role-swapped wgrad {case} ({variant})")


# ======================================================================================================== depth 1 (the 2D neck)
@pytest.mark.parametrize("variant", ["auto", "fp32", "direct"])
@pytest.mark.parametrize("case", sorted(WC.DEPTH1_CASES))
def test_depth_one_vs_float64(case, variant):
    """The 2D neck's calls: 5-D tensors with D = 1, k3/s1, k3/s2 (Din = 1, Dout = 1: not the exact halving the split-operand stride-2
    form needs) and k1."""
    c = WC.DEPTH1_CASES[case]
    assert c[3][0] == 1
    if c[5] == 2:
        assert c[3][0] != 2 * WC.out_extent(c[3][0], 3, 2, 1)
    x, g, ref = WC.conv_case("depth1", case)
    xd, gd = x.to(dev()), g.to(dev())
    _planned("depth1", case, variant, xd, gd)
    got = _wgrad_twice(xd, gd, _conv_args(c), _bits(variant))
    check(got, ref.astype(np.float32), _tol(variant), f"wgrad {case} ({variant})")


# ======================================================================================================== depth parts
@pytest.mark.parametrize("case", sorted(WC.DPART_CASES))
def test_depth_parts_vs_float64(case):
    """The split-operand forms with the column cut along d (`dparts` > 1, a ragged last part).  The part count is the dispatcher's
    own loop over this device's CU count, restated in wgrad_cases.expected_dparts; were it 1 the case would no longer cover what it
    is for."""
    c, parts256, last256 = WC.DPART_CASES[case]
    parts, dchunk, last = WC.expected_dparts(c, _cus())
    print(f"{case}: {_cus()} CUs -> {parts} parts of {dchunk} planes, the last {last}")
    assert parts > 1, f"{case}: one depth part on a device of {_cus()} CUs"
    if _cus() == 256:
        assert (parts, last) == (parts256, last256)
    x, g, ref = WC.conv_case("dparts", case)
    xd, gd = x.to(dev()), g.to(dev())
    form, info = _planned("dparts", case, "auto", xd, gd)
    if form in WC.SPLIT_FORMS:               # (operands off 16 bytes stage scalars: no depth parts to ask about)
        assert (info["parts"], info["per_part"]) == (parts, dchunk) and info["parts"] > 1
        if _cus() == 256:
            assert (info["parts"], info["per_part"]) == WC.PLAN_256[("dparts", case)]["auto"]
    got = _wgrad_twice(xd, gd, _conv_args(c), 0)
    check(got, ref.astype(np.float32), FORM_TOL, f"wgrad {case}")


# ======================================================================================================== more pairs than units
@pytest.mark.parametrize("case,variant", [("k3 99 pairs", "auto"), ("k3 99 pairs", "fp32"),
                                          ("k3s2 99 pairs", "auto"), ("k3s2 99 pairs", "fp32"), ("k3s2 99 pairs", "direct")])
def test_more_channel_pairs_than_units(case, variant, request):
    """99 channel pairs (352 -> 288) against 8 * (CUs / 8 / 3) units: the 12-wave forms' units take several rounds (wgrad_units),
    the split-operand forms' job list is longer than the device."""
    from snvc_amd import ops
    c = WC.PAIRS_CASES[case]
    pairs, units = WC.channel_pairs(c[1], c[2]), WC.wgrad_unit_count(_cus())
    assert pairs > units, f"{pairs} pairs fit the {units} units of a {_cus()}-CU device"
    request.addfinalizer(ops.release_workspaces)          # 512 partitions x 99 pairs of slabs: not kept for the rest of the session
    x, g, ref = WC.conv_case("pairs", case)
    xd, gd = x.to(dev()), g.to(dev())
    form, info = _planned("pairs", case, variant, xd, gd)
    if form in WC.UNIT_FORMS:                # one partition, and the units of every XCD hold all the pairs in rounds
        assert info["parts"] == 1 and 8 * info["per_part"] >= pairs > units and info["grid_x"] == 3 * 8 * info["per_part"]
    elif form in WC.SPLIT_FORMS:             # one job per (column, pair of the job list): more jobs than units
        assert info["parts"] == 1 and info["grid_x"] > units
    else:                                    # generic forms: grid.y = pairs
        assert info["grid_yz"] == pairs * info["per_part"] and pairs > units
    got = _wgrad_twice(xd, gd, _conv_args(c), _bits(variant))
    check(got, ref.astype(np.float32), _tol(variant), f"wgrad {case} ({variant})")


# ======================================================================================================== batch-strided operands
def _channel_slice(t, lo):
    """``t`` as channels [lo, lo + C) of a device buffer STRIDED_EXTRA_CHANNELS wider whose other channels hold STRIDED_FILL."""
    from snvc_amd import ops
    n, c = t.shape[:2]
    buf = torch.full((n, c + WC.STRIDED_EXTRA_CHANNELS) + tuple(t.shape[2:]), WC.STRIDED_FILL, dtype=torch.float32, device=dev())
    view = buf[:, lo:lo + c]
    view.copy_(t.to(dev()))
    s = t[0, 0].numel()
    assert view.stride(0) == (c + WC.STRIDED_EXTRA_CHANNELS) * s != c * s and ops._dense_inner(view) and not view.is_contiguous()
    assert view.data_ptr() - buf.data_ptr() == 4 * lo * s and buf.data_ptr() % 16 == 0
    return view


@pytest.mark.parametrize("variant", ["auto", "fp32", "direct"])
@pytest.mark.parametrize("case", sorted(WC.STRIDED_CASES))
def test_batch_strided_operands(case, variant):
    """x and g as channel slices (x_bs / g_bs != C * D*H*W, the other channels = 1e3).  `aligned`: both slices start on 16 bytes, the
    vector and split-operand forms run on them; `unaligned`: a slice starts 4 bytes off, which every alignment predicate has to see."""
    x, g, ref, args, lo = WC.strided_case(case)
    xs, gs = _channel_slice(x, lo), _channel_slice(g, lo)
    aligned = xs.data_ptr() % 16 == 0 and gs.data_ptr() % 16 == 0
    assert aligned == case.endswith(" aligned")
    _planned("strided", case, variant, xs, gs)
    got = _wgrad_twice(xs, gs, args, _bits(variant))
    check(got, ref.astype(np.float32), _tol(variant), f"strided wgrad {case} ({variant})")


# ======================================================================================================== k1 streaming form
@pytest.mark.parametrize("case", sorted(WC.K1_STREAM_CASES))
def test_k1_streaming_form_vs_float64(case):
    """wgrad_k1_small_partial<1|2> + wgrad_k1_small_final: two output channels, three samples, two voxel chunks, a last workgroup
    with idle channels (Cin % 4 != 0); and a voxel count that is no multiple of 4, which has to fall through to key 111 and still be
    right.  Per-thread fp32 chains and a fixed LDS tree: the direct forms' bound."""
    c, streaming, chunks = WC.K1_STREAM_CASES[case]
    s = int(np.prod(c[3]))
    assert (c[2] <= 2 and s % 4 == 0) == streaming and (not streaming or WC.ceil_div(s // 4, 16384) == chunks)
    x, g, ref = WC.conv_case("k1", case)
    xd, gd = x.to(dev()), g.to(dev())
    assert xd.data_ptr() % 16 == 0 and gd.data_ptr() % 16 == 0
    form, info = _planned("k1", case, "auto", xd, gd)
    assert (form == "K1_STREAM") == streaming and (not streaming or info["parts"] == chunks)
    got = _wgrad_twice(xd, gd, _conv_args(c), 0)
    check(got, ref.astype(np.float32), DIRECT_TOL, f"wgrad {case}")


# ======================================================================================================== the column limits
@pytest.mark.parametrize("variant", ["auto", "fp32"])
@pytest.mark.parametrize("case", sorted(WC.COLUMN_LIMIT_CASES))
def test_column_limit_cases_vs_float64(case, variant):
    """One column more than the split-operand forms' partial slabs hold (257 of 4 x 32 voxels, 513 of 2 x 32 at stride 2): the layer
    takes its key's 12-wave form under `auto` as under `fp32`, and is right."""
    c = WC.COLUMN_LIMIT_CASES[case]
    x, g, ref = WC.conv_case("columns", case)
    xd, gd = x.to(dev()), g.to(dev())
    form, _ = _planned("columns", case, variant, xd, gd)
    if _align(xd) == _align(gd) == 16:
        assert form == ("WINO" if c[5] == 1 else "S2")
    got = _wgrad_twice(xd, gd, _conv_args(c), _bits(variant))
    check(got, ref.astype(np.float32), FORM_TOL, f"wgrad {case} ({variant})")


# ======================================================================================================== rows of 8 bytes
@pytest.mark.parametrize("variant", ["auto", "fp32", "direct"])
@pytest.mark.parametrize("case", sorted(WC.ROWS8_CASES))
def test_rows_of_eight_bytes_vs_float64(case, variant):
    """The float2-piece variants: X3 on rows with W % 4 == 2 on both grids, and X3S2 / S2 / KSPLIT with vec == 2 (16-byte input rows,
    Wo % 4 == 2)."""
    c = WC.ROWS8_CASES[case]
    x, g, ref = WC.conv_case("rows8", case)
    xd, gd = x.to(dev()), g.to(dev())
    form, info = _planned("rows8", case, variant, xd, gd)
    if _align(xd) == _align(gd) == 16 and form != "TAPS":
        assert info["piece_bytes"] == 8
    got = _wgrad_twice(xd, gd, _conv_args(c), _bits(variant))
    check(got, ref.astype(np.float32), _tol(variant), f"wgrad {case} ({variant})")


# ======================================================================================================== unsupported keys
@pytest.mark.parametrize("case", sorted(WC.UNSUPPORTED_CASES))
def test_unsupported_keys_fail_cleanly(case):
    """k5 / stride 2 and k3 / dilation 2 have no kernel: the dispatcher's own error, nothing launched (the device is still in order
    and the next call is right)."""
    from snvc_amd import _lib, ops
    c = WC.UNSUPPORTED_CASES[case]
    x, g = WC.conv_inputs(c, 1)
    with pytest.raises(_lib.Unsupported, match=r"\(ksize,stride,dilation\) not in"):
        ops.conv3d_wgrad(x.to(dev()), g.to(dev()), *_conv_args(c))
    torch.cuda.synchronize()
    ok = (c[0], c[1], c[2], c[3], 3, 1, 1)
    x, g = WC.conv_inputs(ok, 2)
    check(_wgrad_twice(x.to(dev()), g.to(dev()), _conv_args(ok), 0), WC.wgrad_ref64(x, g, 3, 1, 1).astype(np.float32), FORM_TOL, "after the error")


# ======================================================================================================== k5 / k7 layers: dx, dW, dgamma, dbeta
_LAYER_SHAPES = {"32->32": (2, 32, 32, (6, 7, 36)), "6->64": (1, 6, 64, (5, 9, 38)), "40->24": (1, 40, 24, (3, 5, 33))}
_LAYER_KD = {"k5": (5, 1), "k5d2": (5, 2), "k7": (7, 1)}


@functools.lru_cache(maxsize=None)
def _layer_case(kd, shape):
    """State dict, x, gy and the float64 autograd gradients of sum(bn_eval(conv(x)) * gy) on the CPU; shared by both routes."""
    from oracle import torch_ref as T
    k, dil = _LAYER_KD[kd]
    n, cin, cout, shp = _LAYER_SHAPES[shape]
    seed = 1900 + 10 * sorted(_LAYER_KD).index(kd) + sorted(_LAYER_SHAPES).index(shape)
    ref = T.convbn_3d(cin, cout, k, 1, dil * (k - 1) // 2, dilation=dil)
    sd = T.seeded_state_dict(ref, seed)
    ref.load_state_dict(sd)
    ref = ref.double().eval()
    r = np.random.default_rng(seed)
    x = torch.from_numpy(r.standard_normal((n, cin) + shp).astype(np.float32))
    gy = torch.from_numpy(r.standard_normal((n, cout) + shp).astype(np.float32))
    xr = x.double().requires_grad_()
    (ref(xr) * gy.double()).sum().backward()
    return sd, x, gy, xr.grad.numpy(), {name: p.grad.numpy() for name, p in ref.named_parameters()}


@pytest.mark.parametrize("exact", [False, True], ids=["default", "exact"])
@pytest.mark.parametrize("shape", sorted(_LAYER_SHAPES))
@pytest.mark.parametrize("kd", sorted(_LAYER_KD))
def test_k57_layer_backward_vs_float64(kd, shape, exact, request):
    """convbn_3d(cin, cout, k, 1, pad, dilation) with frozen BatchNorm and no activation -- the backward is linear, no ReLU mask --
    through `fused` under autograd: x.grad is _dgrad_layer's flipped-weight convolution (the forward kernels of these keys, which no
    other single-layer test reaches), weight.grad the generic weight-gradient kernel behind the autograd route, both with
    TRAIN_EXACT_K57 off (Winograd F(4,5) / F(4,7) data gradient) and on (direct kernels).
    Bounds, the project's own for these kernels in the forward direction: TIGHT, and WINO7 for k7 on Winograd.  They apply to x.grad
    and to dgamma = sum gy * xhat, whose xhat comes from the forward convolution on the same route; weight.grad (x and the scaled gy
    only) and dbeta (a sum of gy) do not pass through a convolution kernel's forward and get TIGHT on every route."""
    from snvc_amd.models import submodule as S
    S.TRAIN_EXACT_K57[0] = exact
    request.addfinalizer(lambda: S.TRAIN_EXACT_K57.__setitem__(0, False))
    k, dil = _LAYER_KD[kd]
    n, cin, cout, shp = _LAYER_SHAPES[shape]
    sd, x, gy, gx_ref, gp_ref = _layer_case(kd, shape)
    ours = S.convbn_3d(cin, cout, k, 1, dil * (k - 1) // 2, dilation=dil)
    ours.load_state_dict(sd)
    ours = ours.eval().to(dev())
    xo = x.to(dev()).requires_grad_()
    (ours.fused(xo) * gy.to(dev())).sum().backward()
    route = WINO7 if (k == 7 and not exact) else TIGHT
    what = f"{kd} {shape} ({'exact' if exact else 'default'})"
    check(xo.grad.cpu().numpy(), gx_ref.astype(np.float32), route, f"{what} dx")
    got = {name: p.grad.detach().cpu().numpy() for name, p in ours.named_parameters()}
    assert set(got) == set(gp_ref) == {"0.weight", "1.weight", "1.bias"}
    check(got["0.weight"], gp_ref["0.weight"].astype(np.float32), TIGHT, f"{what} dW")
    check(got["1.weight"], gp_ref["1.weight"].astype(np.float32), route, f"{what} dgamma")
    check(got["1.bias"], gp_ref["1.bias"].astype(np.float32), TIGHT, f"{what} dbeta")
