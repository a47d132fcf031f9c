"""tests/wgrad_cases.py against the definition in the header comment of csrc/conv3d_bwd.hip,

    dW[cg][cx][t] = sum_n sum_o  G[n, cg, o] * X[n, cx, o * stride - pad + t * dil]        (pad = dil * (k - 1) / 2),

written out as explicit loops over the taps on zero-padded float64 arrays: the GPU tests (tests/test_gpu_wgrad_forms.py) rest on the
float64 torch autograd helpers, so those are pinned to the definition first -- one tiny case per (ksize, stride, dilation) key the
entry point accepts, and the role-swapped call of the transposed layers with its [Cin_d][Cout_d][27] layout."""
import numpy as np
import pytest

import wgrad_cases as WC


def _close(a, b, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b).max()
    assert err <= 1e-12 * max(np.abs(b).max(), 1e-300), f"{what}: {err:.3e} of {np.abs(b).max():.3e}"


def definition(x_big, g_small, k, stride, dil):
    """The header's sum, tap by tap: [Cg, Cx, k, k, k] in float64."""
    x, g = np.asarray(x_big, dtype=np.float64), np.asarray(g_small, dtype=np.float64)
    pad = dil * (k - 1) // 2
    do, ho, wo = g.shape[2:]
    # zero padding on both sides, wide enough for the last output position's last tap whatever the grid's parity
    need = [(o - 1) * stride + (k - 1) * dil + 1 for o in (do, ho, wo)]
    xp = np.zeros(x.shape[:2] + tuple(max(nd, pad + e) for nd, e in zip(need, x.shape[2:])))
    xp[:, :, pad:pad + x.shape[2], pad:pad + x.shape[3], pad:pad + x.shape[4]] = x
    dw = np.zeros((g.shape[1], x.shape[1], k, k, k))
    for kd in range(k):
        for kh in range(k):
            for kw in range(k):
                win = xp[:, :, kd * dil: kd * dil + (do - 1) * stride + 1: stride,
                         kh * dil: kh * dil + (ho - 1) * stride + 1: stride,
                         kw * dil: kw * dil + (wo - 1) * stride + 1: stride]
                for cg in range(g.shape[1]):
                    for cx in range(x.shape[1]):
                        dw[cg, cx, kd, kh, kw] = (g[:, cg] * win[:, cx]).sum()
    return dw


HOST_CASES = {
    # key: (N, Cin, Cout, (D, H, W), k, stride, dil)
    "111": (2, 3, 2, (2, 3, 5), 1, 1, 1),
    "311": (2, 3, 2, (3, 4, 5), 3, 1, 1),
    "321": (2, 3, 2, (4, 6, 8), 3, 2, 1),
    "321 odd extents": (1, 2, 3, (3, 5, 7), 3, 2, 1),
    "511": (1, 2, 3, (3, 6, 7), 5, 1, 1),
    "512": (2, 2, 2, (5, 4, 10), 5, 1, 2),        # D = 5, H = 4 below the effective extent 9
    "711": (1, 3, 2, (4, 5, 9), 7, 1, 1),
}


@pytest.mark.parametrize("key", sorted(HOST_CASES))
def test_wgrad_ref64_is_the_definition(key):
    case = HOST_CASES[key]
    x, g = WC.conv_inputs(case, WC.seed_of("host", HOST_CASES, key))
    k, stride, dil = case[4:]
    assert g.shape[2:] == WC.out_shape(case[3], k, stride, dil)
    ref = WC.wgrad_ref64(x, g, k, stride, dil)
    assert ref.dtype == np.float64 and ref.shape == (case[2], case[1], k, k, k)
    _close(ref, definition(x.numpy(), g.numpy(), k, stride, dil), f"key {key}")


@pytest.mark.parametrize("case", [(2, 3, 2, (2, 3, 4)), (1, 2, 3, (1, 1, 1))])
def test_transposed_ref64_is_the_role_swapped_definition(case):
    """ConvTranspose3d(k3, s2, p1, op1): X := the output gradient on the doubled grid, G := the layer's input, the equivalent
    convolution is (k3, stride 2, pad 1) and the result is directly [Cin_d][Cout_d][27]."""
    gy_big, x_small = WC.swap_inputs(case, WC.SEED_BASE["host"] + 50 + case[1])
    assert gy_big.shape[2:] == tuple(2 * e for e in x_small.shape[2:])
    ref = WC.wgrad_ref64_transposed(gy_big, x_small)
    assert ref.shape == (case[1], case[2], 3, 3, 3)                      # [Cin_d, Cout_d, ...]
    _close(ref, definition(gy_big.numpy(), x_small.numpy(), 3, 2, 1), f"role swap {case}")
    if case[3] == (1, 1, 1):       # one input voxel at position 0 reaches output positions t - 1 >= 0 only: every tap with a 0 index is empty
        idx = np.indices((3, 3, 3)).min(axis=0)
        assert (ref[:, :, idx == 0] == 0).all() and (ref[:, :, idx > 0] != 0).all()


def test_case_tables_are_consistent():
    """The self-descriptions in the tables: the depth-part counts for a 256-CU device, the pair counts, the k1 form's conditions."""
    for name, (case, parts, last) in WC.DPART_CASES.items():
        got = WC.expected_dparts(case, 256)
        assert (got[0], got[2]) == (parts, last) and got[0] > 1, (name, got)
    units = WC.wgrad_unit_count(256)
    assert units == 80
    for name, case in WC.PAIRS_CASES.items():
        assert WC.channel_pairs(case[1], case[2]) == 99 > units, name
    for name, (case, streaming, chunks) in WC.K1_STREAM_CASES.items():
        s = int(np.prod(case[3]))
        assert (case[4] == 1 and case[2] <= 2 and s % 4 == 0) == streaming, name
        if streaming:
            assert WC.ceil_div(s // 4, 16384) == chunks, name
    for name, (kind, case, lo) in WC.STRIDED_CASES.items():
        assert case[0] == 2 and 0 < lo <= WC.STRIDED_EXTRA_CHANNELS
        big = int(np.prod(case[3])) * (8 if kind == "swap" else 1)
        small = int(np.prod(case[3])) if kind == "swap" else int(np.prod(WC.out_shape(case[3], *case[4:])))
        aligned = (lo * big) % 4 == 0 and (lo * small) % 4 == 0
        assert aligned == name.endswith(" aligned"), (name, big, small)
        if not aligned:
            assert big % 2 == 1 or small % 2 == 1, name
    for name in WC.SCALAR_STAGING_CASES:
        assert WC.K57_CASES[name][3][2] % 4 == 0
