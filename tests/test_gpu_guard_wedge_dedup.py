"""Guard bands (tests/guarded.py) around the wedge deduplication of the fused first layer: cases (a) and (b) of
tests/test_gpu_wedge_dedup.py run unchanged, once as they are and once with every operand between NaN guards and every allocation
of the wrappers -- the pair and the side head that wedge_copy_kernel reads and writes -- between guard zones.  Second placement: 32
bytes off 256, the least the fused first layer's operands may have ("gi / p_il / v_scale / v_bias must be 32-byte aligned"); the side
head's rows stay 16-byte aligned there, so the copy runs in both placements.
"""
import pytest

import guarded as GD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def wedge_case(name):
    """wedge_check under its module's autouse fixture: the 16x16x32 form at every size."""
    from snvc_amd import ops
    from test_gpu_wedge_dedup import wedge_check
    old = ops.X3_Q16_MIN_JOBS[0]
    ops.X3_Q16_MIN_JOBS[0] = 1
    try:
        wedge_check(name)
    finally:
        ops.X3_Q16_MIN_JOBS[0] = old


@pytest.mark.parametrize("off", [0, 32], ids=["aligned", "off32"])
@pytest.mark.parametrize("name", ["a_one_column", "b_two_columns_m60"])
def test_guarded(name, off):
    GD.run_existing(__name__, "wedge_case", dict(name=name), DEV, off)
