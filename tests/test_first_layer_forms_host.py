"""The first-layer form query (include/snvc_forms.h, csrc/sheared_conv.hip) against the table of tests/first_layer_cases.py, and the
table's references against one-element-at-a-time restatements on tiny shapes.  Host code only: nothing is launched, no GPU needed."""
import os

import numpy as np
import pytest

import first_layer_cases as FC

with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "snvc_forms.h")) as _f:
    HEADER = _f.read()


def forms():
    from snvc_amd import _forms
    return _forms


def names():
    return {v: k for k, v in forms().enum_names(HEADER, "FL").items()}


def query(entry, n, c, d, h, w, q=1, m0=0, wg=1, wg2=1, flags=0):
    return forms().first_layer(entry, n, c, d, h, w, q, m0, wg, wg2, flags)


def expand_query(entry, shape, flags=0):
    n, c, h, w, d, q, m0 = shape
    off, wu, off_col, wu_col = FC.sheared_geometry(q, m0, d, w)
    return query(entry, n, c, d, h, w, q, m0, wu, wu_col, flags)


def test_binding_and_header_agree():
    from snvc_amd import ops
    F = forms()
    assert F.lib().snvc_forms_abi_version() == F._ABI == 4
    entries = F.enum_names(HEADER, "FLE")
    assert [entries[k] for k in ("SHEARED_EXPAND", "SHEARED_EXPAND_AMAX", "SHEARED_EXPAND_STATS", "SHEARED_EXPAND_SPLIT", "SHEARED_BACKWARD_REDUCE",
                                 "SHEARED_REDUCE", "WARPED_EXPAND", "WARPED_EXPAND_SPLIT", "WARPED_EXPAND_BACKWARD")] == list(range(9))
    assert (F.FLE_SHEARED_EXPAND, F.FLE_WARPED_EXPAND_BACKWARD) == (FC.SHEARED_EXPAND, FC.WARPED_EXPAND_BACKWARD) == (0, 8)
    assert sorted(names()) == list(range(1, 21))
    assert (FC.RELU, FC.STREAM_OUT, FC.R3) == (ops.EPI_RELU, ops.EPI_STREAM_OUT, ops.WARPED_EXPAND_R3)


@pytest.mark.parametrize("c", FC.EXPAND, ids=str)
def test_sheared_expand_rows(c):
    """RB, the row blocks, the threads of the case; the last block's rows and the idle threads follow from them."""
    n, ch, h, w, d, q, m0 = c.shape
    qn = {1: "Q1", 2: "Q2", 4: "Q4"}[q]
    for entry, form in ((FC.SHEARED_EXPAND, "EXPAND_" + qn), (FC.SHEARED_EXPAND_AMAX, "EXPAND_AMAX_" + qn)) + \
            (((FC.SHEARED_EXPAND_STATS, "STATS_" + qn),) if q != 4 else ()):
        rc, info, text = expand_query(entry, c.shape, FC.RELU if entry != FC.SHEARED_EXPAND_STATS else 0)
        assert rc > 0 and names()[rc] == form, (rc, text)
        assert {k: info[k] for k in c.info} == c.info, info
        assert h - (info["blocks"] - 1) * info["RB"] == c.last and info["RB"] * (w // 4) == c.active <= info["threads"] < c.active + 64
        wu = FC.sheared_geometry(q, m0, d, w)[1]
        assert info["lds"] == 4 * info["RB"] * (q * ((wu + q - 1) // q + 4) + d) and info["chunks"] == 0
    assert info["blocks"] < h, "the statistics partials: fewer row blocks than rows"
    if q == 4:
        rc, _, text = expand_query(FC.SHEARED_EXPAND_STATS, c.shape)
        assert rc == -FC.INVALID and text.startswith("snvc_sheared_expand_stats: bad sizes")


@pytest.mark.parametrize("c", FC.WARPED, ids=str)
def test_warped_expand_rows(c):
    n, ch, h, w, d = c.shape
    for flags, form in ((0, "WARPED_WIN"), (FC.R3, "WARPED_R3"), (FC.RELU, "WARPED_WIN")):
        rc, info, text = query(FC.WARPED_EXPAND, n, ch, d, h, w, flags=flags)
        assert rc > 0 and names()[rc] == form, (rc, text)
        assert {k: info[k] for k in c.info} == c.info, info
        assert h - (info["blocks"] - 1) * info["RB"] == c.last and info["RB"] * (w // 4) == c.active
        rb = info["RB"]
        assert info["lds"] == 4 * (6 * rb * (2 * w + 8) + 3 * rb * d if flags & FC.R3 else 6 * rb * (w + 16) + rb * d + 4 + 4 * (d + 2))
    # every (n, c) slice on its own runs one row per workgroup
    rc, info, _ = query(FC.WARPED_EXPAND, 1, 1, d, h, w)
    assert rc > 0 and info["RB"] == 1 and info["blocks"] == h


@pytest.mark.parametrize("row", FC.SPLIT, ids=[s[0] for s in FC.SPLIT])
def test_split_depth_chunks(row):
    name, (n, c, h, w, d), sheared, warped = row
    for q in (1, 2, 4):
        rc, info, text = query(FC.SHEARED_EXPAND_SPLIT, n, c, d, h, w, q, 3, 100, 12, FC.RELU | FC.STREAM_OUT)
        assert rc > 0 and names()[rc] == f"SPLIT_Q{q}", (rc, text)
        assert (info["chunks"], info["per_chunk"]) == sheared and info["RB"] == 1
        assert (info["grid_x"], info["grid_yz"], info["threads"]) == (h, (c + 7) // 8 * sheared[0] * n, (w + 63) // 64 * 64)
        assert info["lds"] == 4 * (8 * q * ((100 + q - 1) // q + 4) + 8 * sheared[1])
    rc, info, text = query(FC.WARPED_EXPAND_SPLIT, n, c, d, h, w, flags=FC.RELU)
    assert rc > 0 and names()[rc] == "WARPED_SPLIT", (rc, text)
    assert (info["chunks"], info["per_chunk"]) == warped
    assert (info["grid_x"], info["grid_yz"], info["threads"]) == (h, (c + 7) // 8 * warped[0] * n, (w + 63) // 64 * 64)
    assert info["lds"] == 4 * (24 * (w + 16) + 96 + 8 * warped[1] + 4 + 4 * (d + 2))


def test_the_planes_of_the_split_chunks():
    """What the rows are there for: a short last chunk, a chunk without planes, an end plane in a chunk that begins at another phase."""
    planes = {s[0]: FC.chunk_planes(s[1][4], *s[2]) for s in FC.SPLIT}
    assert planes["d35"] == [9, 9, 9, 8] and planes["d67"] == [9] * 7 + [4] and planes["d128"] == [8] * 16
    assert planes["d131"] == [9] * 14 + [5, 0] and planes["d200_wgs"] == [50] * 4
    assert FC.chunk_planes(200, *FC.SPLIT_BY_NAME["d200_wgs"][3]) == [25] * 8
    assert FC.chunk_planes(241, 16, 16) == [16] * 15 + [1]
    assert all(sum(FC.chunk_planes(s[1][4], *g)) == s[1][4] for s in FC.SPLIT for g in s[2:])
    # chunk starts at 9 k: the first plane of a chunk sits at every phase of the q = 2 and q = 4 chains
    assert {(9 * k) % 4 for k in range(15)} == {0, 1, 2, 3}
    # the existing shape of tests/test_gpu_split_format.py: two chunks, nothing more
    rc, info, _ = query(FC.SHEARED_EXPAND_SPLIT, 2, 12, 17, 2, 68, 2, 3, 100, 12)
    assert (info["chunks"], info["per_chunk"]) == (2, 9)


@pytest.mark.parametrize("c", FC.WGRAD, ids=str)
@pytest.mark.parametrize("cin", FC.WGRAD_C)
def test_sheared_wgrad_column_chunks(c, cin):
    wu, = c.shape
    rc, info, text = forms().sheared_wgrad(FC.WGRAD_N, cin, FC.WGRAD_CO, FC.WGRAD_H, wu)
    assert rc > 0 and names()[rc] == "WGRAD", (rc, text)
    assert {k: info[k] for k in c.info} == c.info, info
    assert wu - (info["chunks"] - 1) * info["per_chunk"] == c.last and info["per_chunk"] % 64 == 0
    from snvc_amd import _lib
    assert _lib.lib().snvc_sheared_wgrad_workspace_bytes(FC.WGRAD_N, FC.WGRAD_CO, FC.WGRAD_H, wu) == FC.WGRAD_N * 2 * FC.WGRAD_H * info["chunks"] * 21 * 1024 * 4


def test_sheared_wgrad_refusals_and_the_existing_width():
    F = forms()
    rc, info, _ = F.sheared_wgrad(2, 5, 40, 3, 148)
    assert rc > 0 and (info["chunks"], info["per_chunk"]) == (1, 192)
    rc, _, text = F.sheared_wgrad(2, 33, 40, 3, 148)
    assert rc == -FC.INVALID and text == "snvc_sheared_wgrad: bad sizes (1 <= C <= 32)"
    rc, _, text = F.sheared_wgrad(65536, 5, 40, 3, 148)
    assert rc == -FC.UNSUPPORTED and text == "snvc_sheared_wgrad: too many samples"


@pytest.mark.parametrize("c", FC.REDUCE, ids=str)
def test_sheared_reduce_rows(c):
    n, ch, d, h, w, q = c.shape
    off, wu, off_col, wu_col = FC.sheared_geometry(q, FC.REDUCE_M0, d, w)
    rc, info, text = query(FC.SHEARED_REDUCE, n, ch, d, h, w, q, FC.REDUCE_M0, wu, wu_col)
    assert rc > 0 and names()[rc] == f"REDUCE_Q{q}", (rc, text)
    assert {k: info[k] for k in c.info} == c.info, info
    assert ((wu + q - 1) // q, wu_col) == FC.REDUCE_SLOTS[c.name]
    assert ((wu + q - 1) // q > 256, wu_col > 256) == {"slots_308": (True, False), "wg2_260": (False, True)}[c.name] and info["threads"] == 256


@pytest.mark.parametrize("c", FC.BACKWARD, ids=str)
def test_sheared_backward_rows(c):
    n, ch, d, h, w, q = c.shape
    off, wu, off_col, wu_col = FC.sheared_geometry(q, q + 1, d, w)
    rc, info, text = query(FC.SHEARED_BACKWARD_REDUCE, n, ch, d, h, w, q, q + 1, wu, wu_col)
    assert rc > 0 and names()[rc] == f"BWD_Q{q}", (rc, text)
    assert {k: info[k] for k in c.info} == c.info, info
    assert h - (info["blocks"] - 1) * 4 == c.last
    assert info["lds"] == 4 * 4 * (q * ((wu + q - 1) // q + 4) + d + 2 * wu + 2 * wu_col)


def test_warped_expand_backward_rows():
    for (h, w), (rb, tw) in (((5, 24), (5, 64)), ((20, 100), (4, 128)), ((3, 1024), (1, 1024))):
        rc, info, text = query(FC.WARPED_EXPAND_BACKWARD, 2, 3, 9, h, w)
        assert rc > 0 and names()[rc] == "WARPED_BWD", (rc, text)
        assert (info["RB"], info["per_chunk"], info["threads"], info["blocks"]) == (rb, tw, rb * tw, -(-h // rb))


@pytest.mark.parametrize("row", FC.PINNED, ids=[p[0] for p in FC.PINNED])
def test_rows_that_only_the_lds_cap_produces(row):
    """RB 5 and 7: no halving gives them; 8 rows of more than 4800 floats pass 150 KiB and the launcher steps down one row at a time."""
    _, entry, args, want = row
    rc, info, text = query(entry, *args)
    assert rc > 0, text
    assert {k: info[k] for k in want} == want, info
    assert info["lds"] <= 150 * 1024 < info["lds"] // info["RB"] * (info["RB"] + 1)


@pytest.mark.parametrize("row", FC.REFUSALS, ids=[r[0] for r in FC.REFUSALS])
def test_refusals_carry_the_entry_points_text(row):
    _, entry, args, status, want = row
    rc, info, text = query(entry, *args)
    assert rc == -status and text == want, (rc, text)
    assert not any(info.values())


def test_empty_launches_and_bad_arguments():
    F = forms()
    for entry in (FC.SHEARED_EXPAND, FC.SHEARED_EXPAND_AMAX, FC.SHEARED_EXPAND_SPLIT, FC.SHEARED_REDUCE, FC.WARPED_EXPAND, FC.WARPED_EXPAND_SPLIT,
                  FC.WARPED_EXPAND_BACKWARD):
        rc, info, _ = query(entry, 0, 8, 8, 4, 24, 1, 0, 32, 16)
        assert rc == 0 and not any(info.values()), entry
    for entry in (FC.SHEARED_EXPAND_STATS, FC.SHEARED_BACKWARD_REDUCE):           # these entry points refuse N = 0
        assert query(entry, 0, 8, 8, 4, 24, 1, 0, 32, 16)[0] == -FC.INVALID
    rc, _, text = query(99, 1, 8, 8, 4, 24)
    assert rc == -FC.INVALID and text == "snvc_first_layer_form: unknown entry"
    assert F.lib().snvc_first_layer_form(0, 1, 8, 8, 4, 24, 1, 0, 32, 16, 0, None) == -FC.INVALID
    assert F.lib().snvc_sheared_wgrad_form(1, 8, 8, 4, 24, None) == -FC.INVALID


def test_what_the_older_tests_shapes_run():
    """The shapes of the direct tests in tests/test_gpu_parity.py run one row per workgroup (their docstrings say so)."""
    for n, c, h, w, d, q, m0 in ((2, 3, 6, 24, 10, 2, 0), (2, 32, 8, 40, 12, 2, 0), (2, 32, 12, 44, 12, 1, 0)):
        assert expand_query(FC.SHEARED_EXPAND, (n, c, h, w, d, q, m0))[1]["RB"] == 1
        assert query(FC.WARPED_EXPAND, n, c, d, h, w)[1]["RB"] == 1


# ------------------------------------------------------------------------------------------------ the references, on tiny shapes
@pytest.mark.parametrize("q,m0,planes", [(1, 0, True), (2, 3, True), (4, 1, False), (2, 0, False)])
def test_sheared_expand_ref_is_the_definition(q, m0, planes):
    shape = (2, 3, 2, 8, 5, q, m0)
    g, gcol, pl, scale, bias, (off, wu, off_col, wu_col) = FC.expand_inputs(shape, 7 + q, planes)
    out_shape = (2, 3, 5, 2, 8)
    a = FC.sheared_expand_ref(g, gcol, pl, out_shape, q, m0, off, off_col)
    b = FC.sheared_expand_loops(g, gcol, pl, out_shape, q, m0, off, off_col)
    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    # a narrower G: the index leaves the row on both sides
    a = FC.sheared_expand_ref(g[..., 3:9].copy(), gcol, pl, out_shape, q, m0, off - 3, off_col)
    b = FC.sheared_expand_loops(g[..., 3:9].copy(), gcol, pl, out_shape, q, m0, off - 3, off_col)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a[:, :, :, :, :-1] == (pl[:, :, [0, 1, 1, 1, 2]][..., :-1] if planes else 0)).any()


def test_affine_ref_rounds_twice():
    x = np.array([[[[[1.0 + 2.0 ** -23, -3.0, 0.1]]]]], np.float32)
    sc, bi = np.array([1.0 + 2.0 ** -23], np.float32), np.array([2.0 ** -24], np.float32)
    got = FC.affine_ref(x, sc, bi, False)
    want = np.array([np.float32(np.float32(float(v) * float(sc[0])) + bi[0]) for v in x.reshape(-1)], np.float32).reshape(x.shape)
    assert np.array_equal(got, want)
    fused = np.float32(float(x.reshape(-1)[0]) * float(sc[0]) + float(bi[0]))
    assert got.reshape(-1)[0] != fused, "the example tells one rounding from two"
    assert np.array_equal(FC.affine_ref(x, sc, bi, True).reshape(-1) > 0, [True, False, True])


@pytest.mark.parametrize("q,m0", [(1, 1), (2, 0), (2, 5)])
def test_line_sums_is_the_adjoint_of_the_expand(q, m0):
    """<expand(G, G'), dy> == <G, line> + <G', last> in float64, for the index rule alone (no planes)."""
    n, c, d, h, w = 2, 2, 7, 2, 10
    g, gcol, _, _, _, (off, wu, off_col, wu_col) = FC.expand_inputs((n, c, h, w, d, q, m0), 3, False)
    dy = np.random.default_rng(5).standard_normal((n, c, d, h, w))
    x = FC.sheared_expand_ref(g.astype(np.float64), gcol.astype(np.float64), None, (n, c, d, h, w), q, m0, off, off_col)
    line, last, terms = FC.line_sums(dy, q, m0, wu, off, wu_col, off_col)
    lhs = (FC.sheared_expand_loops(g, gcol, None, (n, c, d, h, w), q, m0, off, off_col).astype(np.float64) * dy).sum()
    rhs = (g.reshape(n, 3, c, h, wu) * line).sum() + (gcol.reshape(n, 3, c, h, wu_col) * last).sum()
    assert abs(lhs - rhs) < 1e-9 * max(1.0, abs(lhs)) and x.dtype == np.float32
    assert terms.sum() == d * (w - 1) - sum(1 for dd in range(d) for ww in range(w - 1) if not 0 <= q * ww - dd - m0 + off < wu)
    cs = FC.class_sums(dy)
    assert np.allclose(cs.sum(2), dy.sum(2)) and np.array_equal(cs[:, :, 0], dy[:, :, 0]) and np.array_equal(cs[:, :, 2], dy[:, :, -1])


def test_wgrad_refs_agree():
    r = np.random.default_rng(11)
    x, gy = r.standard_normal((2, 2, 3, 9)).astype(np.float32), r.standard_normal((2, 3, 3, 9)).astype(np.float32)
    ref = FC.wgrad_ref(x, gy)
    assert np.allclose(ref, FC.wgrad_loops(x, gy), rtol=1e-12, atol=1e-12)
    for chunks, cols in ((1, 64), (2, 5)):
        assert np.abs(FC.wgrad_kernel_order_f32(x, gy, chunks, cols) - ref).max() < 1e-5


def test_stats_ref_and_shifts():
    x = np.random.default_rng(2).standard_normal((2, 3, 4, 2, 4)).astype(np.float32) + 5
    gamma, beta = np.array([1.0, 2.0, 0.5], np.float32), np.array([0.0, 1.0, -1.0], np.float32)
    scale, shift, mean, var = FC.stats_ref(x, gamma, beta, 1e-5)
    for ch in range(3):
        v = x[:, ch].astype(np.float64).reshape(-1)
        m = v.sum() / v.size
        assert abs(mean[ch] - m) < 1e-12 and abs(var[ch] - ((v - m) ** 2).sum() / v.size) < 1e-12
        assert abs(scale[ch] - gamma[ch] / np.sqrt(var[ch] + 1e-5)) < 1e-12 and abs(shift[ch] - (beta[ch] - m * scale[ch])) < 1e-12
    s = FC.warped_shifts(2, 6, 24)
    assert s.dtype == np.float32 and s.shape == (2, 6) and (s >= 0).all()
    assert (s == 0).any() and (s > 24).any() and (s == np.floor(s)).any() and (s != np.floor(s)).any()
