"""Host side of the pooled first-layer prep (include/snvc_prep.h): the plan of its three grids walked block by block against the single
launchers' formulas (restated here), the header against the binding, and the argument checks that run before any launch.  No GPU."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_prep.h")

# (N, C, H, W, D, q, m0): the GPU test's three shapes in both spacings, cfg2 (the headline step), and sizes around the formulas' steps
SHAPES = [(2, 32, 8, 40, 12, 2, 0), (2, 32, 8, 40, 12, 1, 2), (2, 32, 20, 72, 12, 2, 0), (2, 32, 20, 72, 12, 1, 2), (1, 32, 7, 44, 12, 2, 0),
          (1, 32, 7, 44, 12, 1, 2), (1, 32, 96, 312, 192, 2, 0), (1, 64, 16, 32, 8, 1, 0), (3, 32, 17, 33, 40, 2, 5), (1, 32, 1, 4, 4, 1, 0)]


@pytest.fixture(scope="module")
def L():
    from snvc_amd import _lib, _prep
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _prep.lib()


def cdiv(a, b):
    return -(-a // b)


def widths(shape):
    from snvc_amd.models.submodule import sheared_geometry
    n, c, h, w, d, q, m0 = shape
    _, wu, _, wu_col = sheared_geometry(q, m0, d, w)
    return wu, wu_col


def test_header_and_binding_agree():
    """The plan struct's mirror; names, parameters and the ABI number are held by tests/test_abi_tables_host.py."""
    from snvc_amd import _prep
    text = open(HEADER).read()
    fields = re.search(r"typedef struct snvc_prep_pool_plan_t \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"int64_t (\w+)", fields) == [f[0] for f in _prep.PoolPlan._fields_]
    assert ctypes.sizeof(_prep.PoolPlan) == 8 * (2 + 3 + 3 + 1 + 3 + 1)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plan_walk(L, shape):
    """Per stage: the ranges are contiguous from 0 and cover the grid, every (sub-problem, local block) occurs exactly once, and each
    local count is the single launcher's own formula."""
    from snvc_amd import ops
    n, c, h, w, d, q, m0 = shape
    wu, wu_col = widths(shape)
    plan = ops.prep_pool_plan(n, c, h, w, wu, wu_col)
    g = c // 8
    # the single launchers, restated: snvc_f16x3_split_scale; snvc_sheared_upsample_split; snvc_f16x3_from_ncdhw; f16x3_conv2d_forward
    scale = min(max(cdiv(max(n * c * h * w, 1), 256 * 4 * 16), 1), 48)
    want = [[scale, scale],
            [cdiv(n * g * h * wu, 256), cdiv(n * g * h * wu_col, 256), cdiv(h * w, 256) * g * n],
            [cdiv(h, 16) * cdiv(x, 32) * (3 * c // 32) for x in (wu, wu_col, w)]]
    got = [list(plan.a_blocks), list(plan.b_blocks), list(plan.c_jobs)]
    assert got == want
    assert list(plan.b_items) == [n * g * h * wu, n * g * h * wu_col, n * g * h * w] and plan.b_row_blocks == cdiv(h * w, 256)
    assert plan.c_samples == n
    local = ctypes.c_int64()
    for stage in range(3):
        total = sum(want[stage])
        seen, order = set(), []
        for b in range(total):
            sub = L.snvc_prep_pool_locate(ctypes.byref(plan), stage, b, ctypes.byref(local))
            assert 0 <= sub < len(want[stage]) and 0 <= local.value < want[stage][sub]
            assert (sub, local.value) not in seen
            seen.add((sub, local.value))
            order.append(sub)
        assert len(seen) == total                                    # with the bounds above: every (sub-problem, local block) once
        assert order == sorted(order)                                # contiguous ranges in sub-problem order, from block 0
        assert L.snvc_prep_pool_locate(ctypes.byref(plan), stage, total, ctypes.byref(local)) == -1
        assert L.snvc_prep_pool_locate(ctypes.byref(plan), stage, -1, ctypes.byref(local)) == -1
    assert L.snvc_prep_pool_locate(ctypes.byref(plan), 3, 0, ctypes.byref(local)) == -1


def test_cfg2_is_the_issue_s_count(L):
    from snvc_amd import ops
    shape = SHAPES[6]
    plan = ops.prep_pool_plan(*shape[:4], *widths(shape))
    assert list(plan.c_jobs) == [360, 126, 180]                      # 666 jobs over 512 resident slots


def test_partial_blocks_shape(L):
    from snvc_amd import ops
    shape = SHAPES[4]
    plan = ops.prep_pool_plan(*shape[:4], *widths(shape))
    assert any(t % 256 for t in plan.b_items[:2]) and (shape[2] * shape[3]) % 256


def test_the_c_calls_check_their_arguments_before_any_launch(L):
    from snvc_amd import _prep
    from snvc_amd._lib import lib
    err = lambda: lib().snvc_last_error_string()  # noqa: E731
    one = 64        # a non-null, aligned stand-in: the checks below come before any pointer is read
    names = ["right", "n", "c", "h", "w", "q", "wu", "off", "wu2", "off2", "packed_g", "packed_col", "cout3", "mul_g", "mul_col", "rq", "rq2",
             "mul_right", "g", "gcol", "gi", "pitch", "lp", "left", "packed_left", "cout_left", "mul_l", "planes", "p_il", "left_split", "mul_left",
             "scratch", "left_rows", "pool", "stream"]
    good = dict(right=one, n=1, c=32, h=6, w=40, q=1, wu=48, off=4, wu2=24, off2=50, packed_g=one, packed_col=one, cout3=96, mul_g=1.0, mul_col=1.0,
                rq=one, rq2=one, mul_right=one, g=one, gcol=one, gi=one, pitch=64, lp=8, left=one, packed_left=one, cout_left=96, mul_l=1.0,
                planes=one, p_il=one, left_split=one, mul_left=one, scratch=one, left_rows=0, pool=3, stream=None)
    assert len(names) == len(_prep.SIGNATURES["snvc_prep_pooled_x3"][1])

    def call(**kw):
        a = dict(good, **kw)
        return L.snvc_prep_pooled_x3(*[a[k] for k in names])

    for ptr in ("right", "packed_g", "packed_col", "rq", "rq2", "mul_right", "g", "gcol", "left", "packed_left", "planes", "p_il", "left_split",
                "mul_left", "scratch"):
        assert call(**{ptr: None}) == 1 and b"snvc_prep_pooled_x3: null pointer" in err(), ptr
    assert call(gi=None) == 1 and b"gi is NULL" in err()
    assert call(cout3=64) == 1 and b"Cout3 != 3 * C" in err()
    assert call(c=36, cout3=108, cout_left=108) == 2 and b"C % 8" in err()
    assert call(c=40, cout3=120, cout_left=120) == 2 and b"3 * C % 32" in err()        # C % 8 == 0, 3 C = 120 is no multiple of 32
    assert call(cout_left=64) == 2 and b"cout_left" in err()
    for q in (0, 3, 4):
        assert call(q=q) == 1 and b"q in {1,2}" in err()
    assert call(n=0) == 2
    assert call(pool=4) == 1 and b"pool bits" in err()
    assert call(left_rows=2) == 1 and b"left_rows" in err()
    assert call(right=one + 4) == 1 and b"16-byte aligned" in err()
    assert call(rq=one + 8) == 1 and b"16-byte aligned" in err()
    assert call(lp=-1) == 1 and b"snvc_prep_pooled_x3: the interleaved output" in err()      # the layers' own checks, under this call's name
    assert call(pitch=40) == 1 and b"snvc_prep_pooled_x3: the interleaved output" in err()   # lp + WU > pitch
    plan = _prep.PoolPlan()
    assert L.snvc_prep_pool_plan(1, 32, 6, 40, 48, 24, None) == 1 and b"null pointer" in err()
    assert L.snvc_prep_pool_plan(1, 36, 6, 40, 48, 24, ctypes.byref(plan)) == 2
    assert L.snvc_prep_pool_plan(1, 32, 6, 40, 0, 24, ctypes.byref(plan)) == 1


@pytest.mark.parametrize("c", [32, 40, 64])
def test_class_major_rows_and_their_inverse_against_il_index(L, c):
    """Part 2's row order: row r = cls * C + co of the class-major layer holds channel oc = co * 3 + cls.  The permutation
    (ops.class_major_rows: the function the epilogue sends the plain result through) and its inverse, for every oc: the interleaved
    slot of row r under mode 0 is the slot of channel oc under mode 1, so p_il holds the same bytes."""
    from snvc_amd import ops
    perm = ops.class_major_rows(c)
    assert sorted(perm) == list(range(3 * c))
    inv = [0] * (3 * c)
    for r, oc in enumerate(perm):
        inv[oc] = r
    h_dim, w, pitch, lp = 3, 5, 7, 1
    for oc in range(3 * c):
        r = inv[oc]
        assert r == (oc % 3) * c + oc // 3 and perm[r] == oc and L.snvc_prep_plain_plane(r, c) == oc
        for h, x in ((0, 0), (1, 2), (2, 4)):
            assert ops.il_index(1, oc, c, h_dim, pitch, lp, 0, h, x) == ops.il_index(0, r, c, h_dim, pitch, lp, 0, h, x) >= 0
    assert L.snvc_prep_plain_plane(-1, c) == -1 and L.snvc_prep_plain_plane(3 * c, c) == -1 and L.snvc_prep_plain_plane(0, 0) == -1
