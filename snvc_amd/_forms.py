"""ctypes binding of the kernel-form queries of ``libsnvc_hip.so`` (``include/snvc_forms.h``): which form the cost-volume,
gather and weight-gradient launchers take for a shape.  Host code only -- nothing is launched and no device is needed.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_forms_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import ctypes
import re
from typing import Tuple

from . import _lib
from ._lib import c_f, c_i64, c_int, c_p

_ABI = 4   # snvc_forms_abi_version() this binding was written against

INFO = 8                                   # SNVC_FORMS_INFO
ALIGNED_IN, ALIGNED_OUT, ALIGNED_ALL = 1, 2, 3
GATHER_F32, GATHER_C8, GATHER_SPLIT = 0, 1, 2

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_forms_abi_version": (c_int, []),
    "snvc_cost_volume_forward_form": (c_int, [c_i64] * 6 + [c_int, c_int, c_int, c_p]),
    "snvc_cost_volume_backward_form": (c_int, [c_i64] * 6 + [c_int, c_int, c_p]),
    "snvc_voxel_gather_forward_form": (c_int, [c_int] + [c_i64] * 5 + [c_f, c_f, c_int, c_p]),
    "snvc_voxel_gather_backward_form": (c_int, [c_i64] * 5 + [c_int, c_p]),
    "snvc_conv3d_wgrad_form": (c_int, [ctypes.POINTER(_lib.Conv3dDesc), c_int, c_int, c_p]),
    "snvc_conv3d_forward_form": (c_int, [ctypes.POINTER(_lib.Conv3dDesc)] + [c_int] * 6 + [c_p]),
    "snvc_first_layer_form": (c_int, [c_int] + [c_i64] * 5 + [c_int, c_int, c_i64, c_i64, c_int, c_p]),
    "snvc_sheared_wgrad_form": (c_int, [c_i64] * 5 + [c_p]),
}

# info slot names per query (the header's comments)
CV_FWD_INFO = ("RB", "hblocks", "dsplit", "dchunk", "grid_x", "grid_y", "threads", "lds")
CV_BWD_INFO = ("", "", "", "", "grid_x", "", "threads", "")
GATHER_FWD_INFO = ("run", "nruns", "pow2", "slices", "grid_x", "grid_yz", "threads", "lds")
GATHER_BWD_INFO = ("vchunk", "nvchunks", "passes", "max_pieces", "grid_x", "grid_y", "threads", "lds")
# slots 2 and 3 by form family: split-operand forms (dparts, dchunk), 12-wave forms (P, upx), k1 (chunks, -), generic (P, tap chunks)
WGRAD_INFO = ("piece_bytes", "ws_bytes", "parts", "per_part", "grid_x", "grid_yz", "threads", "lds")
# slot 2 by family: tiles (direct, transposed), jobs (Winograd), 16-byte pieces per channel (streaming)
CONV_FWD_INFO = ("piece_bytes", "epi", "tiles", "groups", "grid_x", "grid_yz", "threads", "lds")
ENTRY_FORWARD, ENTRY_HEAD, ENTRY_SIDE_HEAD, ENTRY_STATS = 0, 1, 2, 3
# the first-layer family: slot 2 / 3 are depth chunks / planes per chunk (split producers), column chunks / columns per chunk (weight
# gradient); slot 3 of warped_expand_backward is the row width in threads
FIRST_LAYER_INFO = ("RB", "blocks", "chunks", "per_chunk", "grid_x", "grid_yz", "threads", "lds")
(FLE_SHEARED_EXPAND, FLE_SHEARED_EXPAND_AMAX, FLE_SHEARED_EXPAND_STATS, FLE_SHEARED_EXPAND_SPLIT, FLE_SHEARED_BACKWARD_REDUCE,
 FLE_SHEARED_REDUCE, FLE_WARPED_EXPAND, FLE_WARPED_EXPAND_SPLIT, FLE_WARPED_EXPAND_BACKWARD) = range(9)

lib = _lib.binder(SIGNATURES, "snvc_forms_abi_version", _ABI, "form-query")


def enum_names(header_text: str, prefix: str) -> dict:
    """{name without the prefix: value} of the ``SNVC_<prefix>_<NAME> = <int>`` enumerators of include/snvc_forms.h."""
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"\bSNVC_%s_(\w+)\s*=\s*(\d+)" % prefix, header_text)}


def _query(fn, names, *args) -> Tuple[int, dict, str]:
    info = (c_i64 * INFO)()
    rc = fn(*args, ctypes.cast(info, c_p))
    text = _lib.lib().snvc_last_error_string().decode("utf-8", "replace") if rc < 0 else ""
    return rc, {n: int(v) for n, v in zip(names, info) if n}, text


def cost_volume_forward(n, c, hi, wi, d, downsample, dtype, right_only=False, aligned=ALIGNED_ALL):
    """(form id, or 0 for no launch, or -status; info; error text) of snvc_cost_volume_forward[_right] for these sizes."""
    return _query(lib().snvc_cost_volume_forward_form, CV_FWD_INFO, n, c, hi, wi, d, downsample, dtype, int(right_only), aligned)


def cost_volume_backward(n, c, h, w, d, downsample, dtype, right_only=False):
    return _query(lib().snvc_cost_volume_backward_form, CV_BWD_INFO, n, c, h, w, d, downsample, dtype, int(right_only))


def voxel_gather_forward(kind, n, f, hf, wf, v, resolution, aligned=ALIGNED_ALL):
    """``resolution`` as the ops take it: (rows, columns) of the crop."""
    return _query(lib().snvc_voxel_gather_forward_form, GATHER_FWD_INFO, kind, n, f, hf, wf, v, float(resolution[1]), float(resolution[0]),
                  aligned)


def voxel_gather_backward(n, f, hf, wf, v, deterministic=True):
    return _query(lib().snvc_voxel_gather_backward_form, GATHER_BWD_INFO, n, f, hf, wf, v, int(deterministic))


def conv3d_wgrad(desc, x_align=16, g_align=16):
    """(form id or -status; info; error text) of snvc_conv3d_wgrad[_amax] for a ``_lib.Conv3dDesc`` and the largest of 16 / 8 / 4
    that divides the address of x / g.  ``parts`` / ``per_part``: dparts / dchunk (split-operand forms), P / upx (12-wave forms),
    chunks / 0 (k1 streaming form), partitions / tap chunks (generic forms)."""
    return _query(lambda *a: lib().snvc_conv3d_wgrad_form(ctypes.byref(desc), *a), WGRAD_INFO, x_align, g_align)


def conv3d_forward(desc, entry=ENTRY_FORWARD, x_align=16, y_align=16, res_align=0, planes_align=0, y_head_align=0):
    """(form id, or 0 for no launch, or -status; info; error text) of the fp32 forward entry point ``entry`` for a
    ``_lib.Conv3dDesc``.  Each ``*_align`` is the largest of 16 / 8 / 4 that divides the operand's address, 0 for NULL."""
    return _query(lambda *a: lib().snvc_conv3d_forward_form(ctypes.byref(desc), *a), CONV_FWD_INFO, entry, x_align, y_align, res_align,
                  planes_align, y_head_align)


def first_layer(entry, n, c, d, h, w, q=1, m0=0, wg=1, wg2=1, flags=0):
    """(form id, or 0 for no launch, or -status; info; error text) of the first-layer entry point ``entry`` (FLE_*) for these sizes;
    ``wg`` / ``wg2``: the row lengths of g and gcol.  Entries that do not take q, m0, wg, wg2 or flags ignore them."""
    return _query(lib().snvc_first_layer_form, FIRST_LAYER_INFO, entry, n, c, d, h, w, int(q), int(m0), wg, wg2, int(flags))


def sheared_wgrad(n, c, co, h, wu):
    return _query(lib().snvc_sheared_wgrad_form, FIRST_LAYER_INFO, n, c, co, h, wu)


def address_align(ptr) -> int:
    """The largest of 16 / 8 / 4 that divides ``ptr`` (a tensor's data_ptr()); 0 for None."""
    if ptr is None:
        return 0
    return 16 if ptr % 16 == 0 else 8 if ptr % 8 == 0 else 4
