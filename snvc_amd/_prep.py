"""ctypes binding of the pooled first-layer prep's entry points of ``libsnvc_hip.so`` (``include/snvc_prep.h``); the public entries
are in ``snvc_amd.ops``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``) and from ``_fused.SIGNATURES``: this header versions
itself through ``snvc_prep_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this
module loads nothing.
"""
import ctypes

from . import _lib
from ._lib import c_f, c_i64, c_int, c_p

_ABI = 1   # snvc_prep_abi_version() this binding was written against

POOL_AB, POOL_C = 1, 2      # SNVC_PREP_POOL_AB, SNVC_PREP_POOL_C


class PoolPlan(ctypes.Structure):
    """snvc_prep_pool_plan_t"""
    _fields_ = [("a_blocks", c_i64 * 2), ("b_blocks", c_i64 * 3), ("b_items", c_i64 * 3), ("b_row_blocks", c_i64), ("c_jobs", c_i64 * 3),
                ("c_samples", c_i64)]


# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_prep_abi_version": (c_int, []),
    "snvc_prep_pool_plan": (c_int, [c_i64] * 6 + [ctypes.POINTER(PoolPlan)]),
    "snvc_prep_pool_locate": (c_int, [ctypes.POINTER(PoolPlan), c_int, c_i64, ctypes.POINTER(c_i64)]),
    "snvc_prep_pooled_x3": (c_int, [c_p, c_i64, c_i64, c_i64, c_i64, c_int, c_i64, c_int, c_i64, c_int, c_p, c_p, c_i64, c_f, c_f]
                            + [c_p] * 6 + [c_i64, c_i64, c_p, c_p, c_i64, c_f] + [c_p] * 5 + [c_int, c_int, c_p]),
    "snvc_prep_plain_plane": (c_i64, [c_i64, c_i64]),
}

lib = _lib.binder(SIGNATURES, "snvc_prep_abi_version", _ABI, "pooled prep")
