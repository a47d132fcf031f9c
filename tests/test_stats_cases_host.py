"""tests/stats_cases.py on the CPU, on its float64 reference alone: the inputs give what the table promises (the |mean| / std range of
the `offset` kind, an offset that is bit-constant up to the last border row, a constant channel, a bound that stays small on ordinary
data), the host side sizes the two fold cases' workspaces as the table says, and a lossy accumulator -- float32 over runs of only 8
values, float64 from there -- misses the bound of tests/test_gpu_stats_epilogue.py by two orders of magnitude on every `offset` case:
that test can fail."""
import ctypes
import functools

import numpy as np
import pytest

import stats_cases as SC

CONV = [("fp32", k) for k in SC.FP32_LAYERS if k not in SC.FP32_UNSUPPORTED] + [("x3", k) for k in {**SC.X3_LAYERS, **SC.X3_FOLD_LAYERS}]
ALL = CONV + [("sheared", k) for k in SC.SHEARED]


@functools.lru_cache(maxsize=None)
def _raw64(route, name, kind):
    """The float64 reference of the raw result, read-only."""
    if route == "sheared":
        g, gcol, planes, offs = SC.sheared_inputs(name, kind)
        raw = SC.sheared_ref(name, g, gcol, planes, offs)
    else:
        x, w = SC.conv_inputs(route, name, kind)
        _, _, _, st, tr, _ = SC.layer_of(route, name)
        raw = SC.conv_ref(x, w, st, tr)
    raw.setflags(write=False)
    return raw


def _moments(raw):
    r = np.moveaxis(raw.reshape(raw.shape[0], raw.shape[1], -1), 0, 1).reshape(raw.shape[1], -1)
    return r.mean(1), r.std(1)


@pytest.mark.parametrize("route,name", ALL, ids=lambda v: v.replace(" ", "_"))
def test_offset_kind_has_the_mean_to_spread_ratio(route, name):
    for kind in ("offset", "near-constant"):
        mean, std = _moments(_raw64(route, name, kind))
        live = slice(None, -1) if kind == "near-constant" else slice(None)
        ratio = np.abs(mean[live]) / std[live]
        assert SC.RATIO[0] <= ratio.min() and ratio.max() <= SC.RATIO[1], (route, name, kind, ratio.min(), ratio.max())


@pytest.mark.parametrize("route,name", CONV, ids=lambda v: v.replace(" ", "_"))
def test_the_offset_is_bit_constant_over_the_output(route, name):
    """Channel 0 alone through its weights: c at every output voxel, borders and the last odd row of the transposed layers included."""
    ci, co, sp, st, tr, c = SC.layer_of(route, name)
    x, w = SC.conv_inputs(route, name, "offset")
    x0, w0 = np.zeros_like(x), np.zeros_like(w)
    x0[:, 0] = x[:, 0]
    if tr:
        w0[0] = w[0]
    else:
        w0[:, 0] = w[:, 0]
    part = SC.conv_ref(x0, w0, st, tr)
    assert part.shape == (SC.N, co) + SC.out_extents(sp, st, tr)
    assert (part == c).all() and float(c) == 2.0 ** round(np.log2(c))


@pytest.mark.parametrize("route,name", ALL, ids=lambda v: v.replace(" ", "_"))
def test_near_constant_channel_is_one_value_whose_square_is_no_float32(route, name):
    raw = _raw64(route, name, "near-constant")
    v = float(SC.NEAR_CONSTANT)
    assert (raw[:, -1] == v).all()
    assert float(np.float32(v * v)) != v * v
    assert np.ptp(raw[:, 0]) > 0.0          # the other channels are not constant


@pytest.mark.parametrize("route,name", ALL, ids=lambda v: v.replace(" ", "_"))
def test_cap_holds_on_ordinary_data_and_the_reference_meets_its_own_bound(route, name):
    raw = _raw64(route, name, "ordinary").astype(np.float32)
    gamma, beta = SC.gamma_beta(raw.shape[1])
    err, ref, bounds = SC.stats_errors(raw, gamma, beta, [ref_k.astype(np.float32) for ref_k in
                                                         SC.ER.norm_stats_ref(raw, gamma, beta, raw.shape[1], False, SC.EPS)])
    assert SC.cap_holds(ref, bounds)
    assert all((e <= b).all() for e, b in err.values())       # float64 statistics stored as float32 pass check_stats' comparison


@pytest.mark.parametrize("route,name", ALL, ids=lambda v: v.replace(" ", "_"))
def test_a_lossy_accumulator_misses_the_offset_bound_a_hundredfold(route, name):
    raw = _raw64(route, name, "offset").astype(np.float32)
    gamma, beta = SC.gamma_beta(raw.shape[1])
    mean, var = SC.lossy_stats(raw)
    scale, shift, _, _ = SC.ER.norm_stats_ref(raw, gamma, beta, raw.shape[1], False, SC.EPS)
    err, _, _ = SC.stats_errors(raw, gamma, beta, [scale, shift, mean, var])
    e, b = err["var"]
    print(f"{route} {name}: lossy var error / bound {np.min(e / b):.0f} .. {np.max(e / b):.0f}")
    assert (e / b).max() >= 100.0
    with pytest.raises(AssertionError):
        SC.check_stats(raw, gamma, beta, [scale, shift, mean, var], False, "lossy")
    exact = SC.ER.norm_stats_ref(raw, gamma, beta, raw.shape[1], False, SC.EPS)
    SC.check_stats(raw, gamma, beta, exact, False, "float64")


def test_lossy_accumulator_on_the_constant_channel():
    """What `near-constant` is for: float32 sums of 3.7f and its rounded square leave E x^2 - mean^2 away from 0 by far more than the
    bound, on either side of it (var >= 0 is asserted apart); float64 sums from the first value on give exactly 0."""
    raw = np.full((2, 1, 4, 8, 16), SC.NEAR_CONSTANT, np.float32)
    mean, var = SC.lossy_stats(raw)
    _, ev, _, _ = SC.ER.norm_stats_bounds(raw, None, 1, False, SC.EPS)
    assert abs(var[0, 0]) > 100 * ev[0, 0]
    r64 = raw.astype(np.float64)
    assert (r64 * r64).mean() - r64.mean() ** 2 == 0.0


def test_fold_cases_carry_and_lack_the_first_round_scratch():
    """snvc_f16x3_conv3d_stats_workspace_bytes (host code): the case above 4096 slots per sample is sized with the scratch term of the
    first fold round, its neighbour at exactly 4096 without."""
    from snvc_amd import _lib
    L = _lib.lib()
    seen = []
    for name, (ci, co, sp, st, tr, _) in SC.X3_FOLD_LAYERS.items():
        out = SC.out_extents(sp, st, tr)
        d = _lib.Conv3dDesc(N=SC.N, Cin=ci, Din=sp[0], Hin=sp[1], Win=sp[2], Cout=co, Dout=out[0], Hout=out[1], Wout=out[2], ksize=3, stride=2,
                            dilation=1, pad=1, transposed=1, algo=0)
        slots = SC.x3_slots(name)
        assert slots == SC.X3_FOLD_SLOTS[name]
        doubles, scratch = SC.x3_workspace_doubles(SC.N, co, slots)
        assert int(L.snvc_f16x3_conv3d_stats_workspace_bytes(ctypes.byref(d))) == 8 * doubles, name
        seen.append(scratch)
    assert seen[0] == SC.N * 65 * 64 and seen[1] == 0


@pytest.mark.parametrize("name", list({**SC.X3_LAYERS, **SC.X3_FOLD_LAYERS}), ids=lambda v: v.replace(" ", "_"))
def test_split_cases_take_the_forms_the_table_names(name):
    """ops.x3_form, the rule Conv3dLayerX3 launches by (host code): the table's form per case; both MFMA shapes are among them."""
    from snvc_amd import ops
    ci, co, sp, st, tr, _ = SC.layer_of("x3", name)
    forced = SC.x3_algo(SC.X3_FORCED[name]) if name in SC.X3_FORCED else None
    got = ops.x3_form(co, 3, st, 1, tr, SC.N, SC.out_extents(sp, st, tr), True, False, forced)
    assert got == SC.x3_algo(SC.X3_FORM[name])
    assert {"Q16", "SMALL", "0"} <= set(SC.X3_FORM.values())
