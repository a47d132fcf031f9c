"""ctypes binding of the wedge deduplication's entry points of ``libsnvc_hip.so`` (``include/snvc_dedup.h``); the public entries
are in ``snvc_amd.ops``.

Kept apart from ``_lib.SIGNATURES`` and ``_fused.SIGNATURES`` (pinned tables): this header versions itself through
``snvc_dedup_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module loads
nothing.
"""
import ctypes

from . import _fused, _lib
from ._lib import c_i64, c_int

_ABI = 1   # snvc_dedup_abi_version() this binding was written against

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_dedup_abi_version": (c_int, []),
    "snvc_dedup_fused_first_conv3d_forward": _fused.SIGNATURES["snvc_fused_first_conv3d_forward"],      # the same arguments
    "snvc_dedup_fused_first_tiles": (c_i64, [ctypes.POINTER(_lib.Conv3dDesc), c_int, c_int, c_int, ctypes.POINTER(c_i64),
                                             ctypes.POINTER(c_i64), c_int]),
}

lib = _lib.binder(SIGNATURES, "snvc_dedup_abi_version", _ABI, "wedge deduplication")
