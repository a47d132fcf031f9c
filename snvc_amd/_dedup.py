"""ctypes binding of the wedge deduplication's entry points of ``libsnvc_hip.so`` (``include/snvc_dedup.h``); the public entries
are in ``snvc_amd.ops``.

Kept apart from ``_lib.SIGNATURES`` and ``_fused.SIGNATURES`` (pinned tables): this header versions itself through
``snvc_dedup_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module loads
nothing.
"""
import ctypes

from . import _fused, _lib

_ABI = 1   # snvc_dedup_abi_version() this binding was written against

c_i64 = ctypes.c_int64
c_int = ctypes.c_int

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_dedup_abi_version": (c_int, []),
    "snvc_dedup_fused_first_conv3d_forward": _fused.SIGNATURES["snvc_fused_first_conv3d_forward"],      # the same arguments
    "snvc_dedup_fused_first_tiles": (c_i64, [ctypes.POINTER(_lib.Conv3dDesc), c_int, c_int, c_int, ctypes.POINTER(c_i64),
                                             ctypes.POINTER(c_i64), c_int]),
}

_bound = None


def lib() -> ctypes.CDLL:
    """``_lib.lib()``'s handle with this table's signatures set and the ABI checked."""
    global _bound
    if _bound is None:
        handle = _lib.lib()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        if handle.snvc_dedup_abi_version() != _ABI:
            raise RuntimeError("libsnvc_hip.so wedge deduplication ABI version mismatch; rebuild it")
        _bound = handle
    return _bound
