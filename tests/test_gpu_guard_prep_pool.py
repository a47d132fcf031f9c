"""Guard bands (tests/guarded.py) around the pooled first-layer prep: one case of tests/test_gpu_prep_pool.py -- two tile rows with the
second short, three tile columns with the last short, every stage-B range ending inside a block -- run once as it is and once with
the two features between NaN guards and every buffer of the three launches (the four scratch words, both scales, the three split
pairs, the five results) between guard zones.  Second placement: 32 bytes off 256; the features stay 16-byte aligned there.
"""
import pytest

import guarded as GD

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def pool_case(**kw):
    """test_gpu_prep_pool.pool_case with the module's packed layers made anew, so both runs allocate the same tensors."""
    import test_gpu_prep_pool as P
    P._LAYERS.clear()
    try:
        P.pool_case(**kw)
    finally:
        P._LAYERS.clear()


@pytest.mark.parametrize("off", [0, 32], ids=["aligned", "off32"])
def test_guarded(off):
    GD.run_existing(__name__, "pool_case", dict(n=1, h=20, w=72, q=2, m0=0), DEV, off)
