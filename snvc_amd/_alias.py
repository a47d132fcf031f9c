"""ctypes binding of the aliased wedge duplicates' entry points of ``libsnvc_hip.so`` (``include/snvc_alias.h``); the public entries
are in ``snvc_amd.ops``.

Kept apart from ``_lib.SIGNATURES``, ``_fused.SIGNATURES`` and ``_dedup.SIGNATURES`` (pinned tables): this header versions itself
through ``snvc_alias_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes

from . import _fused, _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_alias_abi_version() this binding was written against


class WedgeDesc(ctypes.Structure):
    """Mirror of ``snvc_wedge_desc`` (include/snvc_alias.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("D", "W", "q", "m0", "off")]


# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_alias_abi_version": (c_int, []),
    "snvc_alias_depth": (c_i64, [ctypes.POINTER(WedgeDesc), c_i64, c_i64]),
    "snvc_alias_fused_first_conv3d_forward": _fused.SIGNATURES["snvc_fused_first_conv3d_forward"],      # the same arguments
    "snvc_alias_f16x3_conv3d_forward": (c_int, [ctypes.POINTER(_lib.Conv3dDesc), c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p,
                                                ctypes.POINTER(WedgeDesc), c_p]),
    "snvc_alias_deconv_tail_gather": (c_int, [c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i64, ctypes.POINTER(WedgeDesc), c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_alias_abi_version", _ABI, "aliased wedge")
