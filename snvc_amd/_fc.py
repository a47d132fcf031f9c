"""ctypes binding of the FC box head's entry points of ``libsnvc_hip.so`` (``include/snvc_fc.h``); the public entry is
``snvc_amd.models.FCmodel``.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_fc_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
from . import _lib
from ._lib import c_f, c_i64, c_int, c_p

_ABI = 1   # snvc_fc_abi_version() this binding was written against

MAX_WIDTH = 1024   # SNVC_FC_MAX_WIDTH

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_fc_abi_version": (c_int, []),
    "snvc_fc_packed_floats": (c_i64, [c_i64, c_i64, c_i64, c_i64]),
    "snvc_fc_eval_forward": (c_int, [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_int, c_p]),
    "snvc_fc_train_layer_forward": (c_int, [c_p] * 14 + [c_i64, c_i64, c_i64, c_f, c_f, c_f, c_int, c_p]),
    "snvc_fc_train_layer_backward_params": (c_int, [c_p] * 12 + [c_i64, c_i64, c_i64, c_f, c_int, c_p]),
    "snvc_fc_train_layer_backward_input": (c_int, [c_p] * 4 + [c_i64, c_i64, c_i64, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_fc_abi_version", _ABI, "FC head")
