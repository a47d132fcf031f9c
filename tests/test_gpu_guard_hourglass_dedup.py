"""Guard bands (tests/guarded.py) around the hourglass's duplicate tiles: two cases of tests/test_gpu_hourglass_dedup.py (q 1 with two
columns of different length: every run of the live walk but two is non-empty; q 2, D 148: the shortest column) run unchanged, once as
they are and once with every operand between NaN guards and every allocation of the wrappers between guard zones -- the pair whose
duplicate rows the stride-2 layer skips and reads through its input's descriptor, the stride-1 layer's aliased reads of that pair.
Second placement: 32 bytes off 256; the C8 tensors stay 16-byte aligned there.
"""
import pytest

import guarded as GD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def hg_case(name):
    """hg_case under its module's autouse fixture: the 16x16x32 forms at every size."""
    from snvc_amd import ops
    from test_gpu_hourglass_dedup import hg_case as case
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    try:
        case(name)
    finally:
        ops.X3_Q16_MIN_JOBS[0] = old


@pytest.mark.parametrize("off", [0, 32], ids=["aligned", "off32"])
@pytest.mark.parametrize("name", ["q1_two_columns", "q2_half_pixel"])
def test_guarded(name, off):
    GD.run_existing(__name__, "hg_case", dict(name=name), DEV, off, arena_bytes=512 << 20)      # three 43 MB pairs (D 160, W 132) and the two layers' results
