"""The C ABI's header / binding pairs, one row per header of include/, and what tests/test_abi_tables_host.py holds every row
to: the declarations of a header read as (return type, name, parameters), and the rule that says which ctypes class a C
parameter or return type takes.  A new header adds one row here.
"""
import collections
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# header under include/, binding module under snvc_amd, version symbol, declared symbols, ABI number
Row = collections.namedtuple("Row", "header module version_symbol count abi")
ROWS = [
    Row("snvc_hip.h", "_lib", "snvc_abi_version", 99, 6),
    Row("snvc_alias.h", "_alias", "snvc_alias_abi_version", 5, 1),
    Row("snvc_decode.h", "_decode", "snvc_decode_abi_version", 3, 1),
    Row("snvc_dedup.h", "_dedup", "snvc_dedup_abi_version", 3, 1),
    Row("snvc_depth.h", "_depth", "snvc_depth_abi_version", 6, 1),
    Row("snvc_dsgn.h", "_dsgn", "snvc_dsgn_abi_version", 3, 1),
    Row("snvc_fc.h", "_fc", "snvc_fc_abi_version", 6, 1),
    Row("snvc_forms.h", "_forms", "snvc_forms_abi_version", 9, 4),
    Row("snvc_fused.h", "_fused", "snvc_fused_abi_version", 5, 1),
    Row("snvc_hgdedup.h", "_hgdedup", "snvc_hgdedup_abi_version", 8, 1),
    Row("snvc_hrnet.h", "_hrnet", "snvc_hrnet_abi_version", 3, 1),
    Row("snvc_iou3d.h", "_iou3d", "snvc_iou3d_abi_version", 7, 1),
    Row("snvc_loss.h", "_loss", "snvc_loss_abi_version", 11, 1),
    Row("snvc_oiou.h", "_oiou", "snvc_oiou_abi_version", 3, 1),
    Row("snvc_prep.h", "_prep", "snvc_prep_abi_version", 5, 1),
    Row("snvc_roicrop.h", "_roicrop", "snvc_roicrop_abi_version", 3, 1),
    Row("snvc_targets.h", "_targets", "snvc_targets_abi_version", 4, 1),
]

SCALARS = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "int32_t": ctypes.c_int32, "float": ctypes.c_float,
           "double": ctypes.c_double}
RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}


def module(row):
    return importlib.import_module("snvc_amd." + row.module)


def declarations(row):
    """[(return type, name, [parameter text, ...])] of the header's SNVC_API declarations, in its order, comments taken out."""
    text = open(os.path.join(ROOT, "include", row.header)).read()
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    found = []
    for ret, name, params in re.findall(r"SNVC_API\s+([\w\s\*]+?)\b(snvc_\w+)\s*\(([^)]*)\)\s*;", text):
        params = [" ".join(p.split()) for p in params.split(",")]
        found.append((" ".join(ret.split()), name, [] if params == ["void"] else params))
    return found


def pointer_like(ctype):
    return ctype in (ctypes.c_void_p, ctypes.c_char_p) or (isinstance(ctype, type) and issubclass(ctype, (ctypes._Pointer, ctypes.Array)))


def parameter_agrees(param, ctype):
    """Whether the ctypes class fits the declared parameter (``type name``).  A C type the rule does not know raises."""
    if "*" in param or "[" in param:
        return pointer_like(ctype)
    ctext = " ".join(w for w in param.split()[:-1] if w != "const")
    if ctext not in SCALARS:
        raise AssertionError(f"parameter `{param}`: the rule knows no C type `{ctext}`; add it to tests/abi_tables.py knowingly")
    return ctype is SCALARS[ctext]


def return_agrees(ret, ctype):
    if ret not in RETURNS:
        raise AssertionError(f"return type `{ret}`: the rule knows none such; add it to tests/abi_tables.py knowingly")
    return ctype is RETURNS[ret]
