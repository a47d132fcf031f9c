"""Guard bands (tests/guarded.py) around the aliased wedge duplicates: two cases of tests/test_gpu_wedge_alias.py (q 1 with two columns; q 2, D 148: the longest remap) run unchanged, once as
they are and once with every operand between NaN guards and every allocation of the wrappers between guard zones -- the pair and the
side head whose duplicate rows conv2 skips, the stride-2 layer's aliased reads of the pair, the gather's of the side head.  Second
placement: 32 bytes off 256, the least the fused first layer's operands may have; the side head's rows stay 16-byte aligned there.
"""
import pytest

import guarded as GD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def alias_case(name):
    """alias_case under its module's autouse fixture: the 16x16x32 forms at every size."""
    from snvc_amd import ops
    from test_gpu_wedge_alias import alias_case as case
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    try:
        case(name)
    finally:
        ops.X3_Q16_MIN_JOBS[0] = old


@pytest.mark.parametrize("off", [0, 32], ids=["aligned", "off32"])
@pytest.mark.parametrize("name", ["q1_two_columns", "q2_half_pixel"])
def test_guarded(name, off):
    GD.run_existing(__name__, "alias_case", dict(name=name), DEV, off, arena_bytes=512 << 20)      # two 44 MB pairs (q 2, D 148) and their readers' results
