"""ctypes binding of the oriented-IoU entry points of ``libsnvc_hip.so`` (``include/snvc_oiou.h``); the public entry is
``snvc_amd.thirdparty.oriented_iou_loss``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_oiou_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes

from . import _lib
from ._lib import c_int, c_p

_ABI = 1   # snvc_oiou_abi_version() this binding was written against

BOXES, QUADS = 0, 1          # SNVC_OIOU_BOXES, SNVC_OIOU_QUADS
DIOU, GIOU = 0, 1            # SNVC_OIOU_DIOU, SNVC_OIOU_GIOU
SMALLEST, ALIGNED = 0, 1     # SNVC_OIOU_SMALLEST, SNVC_OIOU_ALIGNED
OUT = 8                      # SNVC_OIOU_OUT: inter, area1, area2, u, iou, enc_w, enc_h, loss
INTER, AREA1, AREA2, UNION, IOU, ENC_W, ENC_H, LOSS = range(8)


class OiouDesc(ctypes.Structure):
    """Mirror of ``snvc_oiou_desc`` (include/snvc_oiou.h)."""
    _fields_ = [("form", ctypes.c_int32), ("kind", ctypes.c_int32), ("enclosing", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("M", ctypes.c_int64), ("a", c_p), ("b", c_p), ("ctr_a", c_p), ("ctr_b", c_p), ("out", c_p), ("gout", c_p),
                ("ga", c_p), ("gb", c_p), ("gctr_a", c_p), ("gctr_b", c_p)]


_desc_p = ctypes.POINTER(OiouDesc)

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_oiou_abi_version": (c_int, []),
    "snvc_oiou_forward": (c_int, [_desc_p, c_p]),
    "snvc_oiou_backward": (c_int, [_desc_p, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_oiou_abi_version", _ABI, "oriented-IoU")
