"""Writes tests/golden/wgrad_workspace_table.json: what snvc_conv3d_wgrad_workspace_bytes returns, and what snvc_conv3d_wgrad_amax
answers to descriptors it refuses before it looks at a pointer, over the descriptors of tests/wgrad_cases.py.

    SNVC_HIP_LIB=<libsnvc_hip.so of the recording commit> python tests/golden/make_golden_wgrad_plan.py

Run it ONLY against a library built from the parent of the commit that put the weight gradient's dispatch behind one plan (the
commit that added this script), on a machine WITHOUT a GPU: the compute-unit count then falls back to 256 and the bytes depend on
the descriptor alone.  Nothing is launched: the launcher is called with null pointers only.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from snvc_amd import _lib  # noqa: E402

import wgrad_cases as WC  # noqa: E402


def workspace_bytes(L, fields):
    return int(L.snvc_conv3d_wgrad_workspace_bytes(ctypes.byref(WC.make_desc(fields)) if fields is not None else None))


def refusal(L, fields):
    """[status, text] of the launcher for this descriptor and null pointers."""
    rc = L.snvc_conv3d_wgrad_amax(ctypes.byref(WC.make_desc(fields)) if fields is not None else None, None, None, None, None, None, None, None)
    return [int(rc), L.snvc_last_error_string().decode("utf-8", "replace")]


def main():
    import torch
    assert not torch.cuda.is_available(), "record on a machine without a GPU: the 256-CU fallback"
    L = _lib.lib()
    cases = [[g, n, workspace_bytes(L, WC.case_desc_fields(g, n))] for g, n in WC.all_cases()]
    sweep = [[f[k] for k in WC.DESC_FIELDS] + [workspace_bytes(L, f)] for f in WC.sweep_desc_fields()]
    refusals = {what: refusal(L, f) + [workspace_bytes(L, f)] for what, f in WC.refusal_desc_fields().items()}
    assert all(r[0] != 0 for r in refusals.values())
    out = os.path.join(HERE, "wgrad_workspace_table.json")
    with open(out, "w") as f:
        json.dump({"fields": list(WC.DESC_FIELDS), "cases": cases, "sweep": sweep, "refusals": refusals}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(cases)} cases, {len(sweep)} sweep rows, {len(refusals)} refusals, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
