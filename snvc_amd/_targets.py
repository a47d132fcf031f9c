"""ctypes binding of the training-target entry points of ``libsnvc_hip.so`` (``include/snvc_targets.h``); the public class
is ``snvc_amd.geometry.TargetGenerator``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_targets_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes

from . import _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_targets_abi_version() this binding was written against

MAX_PARTS = 9          # SNVC_TARGETS_MAX_PARTS
MAX_SAMPLES = 7000     # SNVC_TARGETS_MAX_SAMPLES


class TargetsGrid(ctypes.Structure):
    """Mirror of ``snvc_targets_grid`` (include/snvc_targets.h)."""
    _fields_ = [(n, ctypes.c_int32) for n in ("nh", "nw", "nl", "num_parts", "sigma", "grid_type")] + [
        ("spacing", ctypes.c_double * 3), ("grid_range", ctypes.c_double * 3), ("ranges", ctypes.c_double * 6)]


_grid_p = ctypes.POINTER(TargetsGrid)

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_targets_abi_version": (c_int, []),
    "snvc_targets_workspace_bytes": (c_i64, [c_i64]),
    "snvc_targets_fields": (c_int, [_grid_p, c_p, c_p, c_i64, c_p, c_p, c_p, c_p]),
    "snvc_targets_occupancy": (c_int, [_grid_p, c_p, c_p, c_i64, c_p, c_int, c_i64, c_p, c_i64, c_p, c_p, c_p, c_p, c_p, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_targets_abi_version", _ABI, "targets")
