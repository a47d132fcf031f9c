"""ctypes binding of the rotated-box IoU / NMS entry points of ``libsnvc_hip.so`` (``include/snvc_iou3d.h``).

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_iou3d_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this
module loads nothing.
"""
from . import _lib
from ._lib import c_f32, c_i64, c_int, c_p

_ABI = 1   # snvc_iou3d_abi_version() this binding was written against

OVERLAP, IOU_BEV, IOU_3D = 0, 1, 2          # snvc_iou3d_pairwise `what`
NMS_ROTATED, NMS_NORMAL = 0, 1              # snvc_iou3d_nms `kind`
NMS_MAX_BOXES = 65536                       # SNVC_NMS_MAX_BOXES

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_iou3d_abi_version": (c_int, []),
    "snvc_iou3d_pairwise_workspace_bytes": (c_i64, [c_i64, c_i64]),
    "snvc_iou3d_pairwise": (c_int, [c_p, c_i64, c_p, c_i64, c_int, c_int, c_p, c_p, c_p]),
    "snvc_iou3d_nms_workspace_bytes": (c_i64, [c_i64]),
    "snvc_iou3d_nms": (c_int, [c_p, c_i64, c_f32, c_int, c_p, c_p, c_p, c_p]),
    "snvc_iou3d_backward": (c_int, [c_p, c_p, c_p, c_i64, c_f32, c_p, c_p]),
    "snvc_iou3d_boxes_iou_bev_cpu": (c_int, [c_p, c_i64, c_p, c_i64, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_iou3d_abi_version", _ABI, "iou3d")
