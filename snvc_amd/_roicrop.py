"""ctypes binding of the RoI-crop entry points of ``libsnvc_hip.so`` (``include/snvc_roicrop.h``); the public class is
``snvc_amd.geometry.RoICropper``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_roicrop_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes

from . import _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_roicrop_abi_version() this binding was written against

MAX_SIDE = 32767       # SNVC_ROICROP_MAX_SIDE
MAX_SAMPLES = 32767    # SNVC_ROICROP_MAX_SAMPLES
FIXED5, EXACT = 0, 1   # SNVC_ROICROP_FIXED5, SNVC_ROICROP_EXACT
IMAGE_BYTES = 24       # sizeof(snvc_roicrop_image)


class RoICropImage(ctypes.Structure):
    """Mirror of ``snvc_roicrop_image`` (include/snvc_roicrop.h); a table of them is uploaded as int64 triples
    (pointer, height | width << 32, row stride)."""
    _fields_ = [("data", c_p), ("height", ctypes.c_int32), ("width", ctypes.c_int32), ("row_stride", c_i64)]


class RoICropConfig(ctypes.Structure):
    """Mirror of ``snvc_roicrop_config`` (include/snvc_roicrop.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("out_w", "out_h", "interpolation", "swap_rb", "raw", "reserved")] + [
        ("aspect_ratio", ctypes.c_double), ("grid_range", ctypes.c_double * 3)]


assert ctypes.sizeof(RoICropImage) == IMAGE_BYTES
_cfg_p = ctypes.POINTER(RoICropConfig)

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_roicrop_abi_version": (c_int, []),
    "snvc_roicrop_workspace_bytes": (c_i64, [c_i64]),
    "snvc_roicrop": (c_int, [_cfg_p, c_p, c_p, c_i64, c_p, c_p, c_p, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_roicrop_abi_version", _ABI, "roicrop")
