"""ctypes binding of the fused sheared first layer's entry points of ``libsnvc_hip.so`` (``include/snvc_fused.h``); the public
entries are in ``snvc_amd.ops``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_fused_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes

from . import _lib
from ._lib import c_f, c_i64, c_int, c_p

_ABI = 1   # snvc_fused_abi_version() this binding was written against

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_fused_abi_version": (c_int, []),
    "snvc_fused_il_index": (c_i64, [c_int] + [c_i64] * 8),
    "snvc_fused_sheared_prep_x3": (c_int, [c_p, c_i64, c_i64, c_i64, c_i64, c_int, c_i64, c_int, c_i64, c_int, c_p, c_p, c_i64, c_f, c_f]
                                   + [c_p] * 7 + [c_i64, c_i64, c_p]),
    "snvc_fused_planes_from_f32": (c_int, [c_p, c_i64, c_i64, c_i64, c_i64, c_p, c_i64, c_f] + [c_p] * 6),
    "snvc_fused_first_conv3d_forward": (c_int, [ctypes.POINTER(_lib.Conv3dDesc)] + [c_p] * 7 + [c_f, c_p, c_p, c_i64, c_i64, c_p, c_p, c_p]
                                        + [c_int] * 5 + [c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_fused_abi_version", _ABI, "fused first layer")
