"""ctypes binding of the box read-out entry points of ``libsnvc_hip.so`` (``include/snvc_decode.h``); the public entry is
``snvc_amd.decode.refine_boxes``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_decode_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes

from . import _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_decode_abi_version() this binding was written against

GRID, COORDS_F32, COORDS_F64 = 0, 1, 2   # SNVC_DECODE_GRID, SNVC_DECODE_COORDS_F32, SNVC_DECODE_COORDS_F64


class DecodeConfig(ctypes.Structure):
    """Mirror of ``snvc_decode_config`` (include/snvc_decode.h)."""
    _fields_ = [("x_range", ctypes.c_double * 2), ("z_range", ctypes.c_double * 2), ("min_val", ctypes.c_float),
                ("max_val", ctypes.c_float), ("source", ctypes.c_int32), ("reserved", ctypes.c_int32)]


_cfg_p = ctypes.POINTER(DecodeConfig)

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_decode_abi_version": (c_int, []),
    "snvc_decode_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "snvc_decode_boxes": (c_int, [_cfg_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_decode_abi_version", _ABI, "decode")
