"""ctypes binding of the depth read-out's entry points of ``libsnvc_hip.so`` (``include/snvc_depth.h``); the public entry is
``snvc_amd.depth``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_depth_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
from . import _lib
from ._lib import c_f, c_i64, c_int, c_p

_ABI = 1   # snvc_depth_abi_version() this binding was written against

MAX_PLANES = 2048     # SNVC_DEPTH_MAX_PLANES
POINTS_BLOCK = 256    # SNVC_DEPTH_POINTS_BLOCK

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_depth_abi_version": (c_int, []),
    "snvc_depth_readout_forward": (c_int, [c_p] * 6 + [c_i64] * 7 + [c_int, c_p]),
    "snvc_depth_readout_backward": (c_int, [c_p] * 7 + [c_i64] * 7 + [c_int, c_p]),
    "snvc_depth_to_points": (c_int, [c_p, c_p, c_int, c_p] + [c_f] * 7 + [c_p, c_p, c_i64, c_i64, c_i64, c_p]),
    "snvc_depth_points_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "snvc_depth_to_points_compact": (c_int, [c_p, c_p, c_int, c_p] + [c_f] * 7 + [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_depth_abi_version", _ABI, "depth read-out")
