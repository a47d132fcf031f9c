"""ctypes binding of the hourglass's duplicate tiles' entry points of ``libsnvc_hip.so`` (``include/snvc_hgdedup.h``); the public
entries are in ``snvc_amd.ops``.

Kept apart from ``_lib.SIGNATURES``, ``_fused.SIGNATURES``, ``_dedup.SIGNATURES`` and ``_alias.SIGNATURES`` (pinned tables): this
header versions itself through ``snvc_hgdedup_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so
importing this module loads nothing.
"""
import ctypes

from . import _alias, _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_hgdedup_abi_version() this binding was written against

_desc_p = ctypes.POINTER(_alias.WedgeDesc)
_forward = (c_int, [ctypes.POINTER(_lib.Conv3dDesc), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, _desc_p, c_p])

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_hgdedup_abi_version": (c_int, []),
    "snvc_hgdedup_max_columns": (c_int, []),
    "snvc_hgdedup_tile_pure": (c_int, [_desc_p, c_i64, c_i64]),
    "snvc_hgdedup_tiles": (c_i64, [_desc_p, ctypes.POINTER(c_i64), ctypes.POINTER(c_i64), c_int]),
    "snvc_hgdedup_depth": (c_i64, [_desc_p, c_i64, c_i64]),
    "snvc_hgdedup_live_tile": (c_i64, [_desc_p, c_i64, c_i64] + [ctypes.POINTER(c_i64)] * 3),
    "snvc_hgdedup_f16x3_conv3d_forward": _forward,
    "snvc_hgdedup_reader_f16x3_conv3d_forward": _forward,
}

lib = _lib.binder(SIGNATURES, "snvc_hgdedup_abi_version", _ABI, "hourglass duplicate")
