"""Writes tests/golden/f16_plan_table.json and, with --gpu, tests/golden/f16_plan_gpu.json: what the host side of
snvc_amd/csrc/conv3d_f16.hip decides and launches, over the descriptors and cells of tests/f16_plan_cases.py.

    SNVC_HIP_LIB=<libsnvc_hip.so of the recording commit> python tests/golden/make_golden_f16_plan.py [--gpu]

Run it ONLY against a library built from the parent of the commit that turned that file's kernel forms into records (the commit that
added this script): the files are a record of what the enum-and-switch host code returned and computed there.

Without --gpu (no device needed, nothing is launched): per descriptor the packed bytes of the fp16-storage and the split route and the
statistics workspace's bytes, with the error text behind every -1; and the status and text of the six forward entry points on a null
descriptor, null pointers and an empty batch.  With --gpu (an MI355X): per form and call kind the status and error text, and for an
accepted call the sha256 of the packed weights and of every output buffer.  The kernels are deterministic, so equal launch arguments
give equal bits.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.dont_write_bytecode = True

from snvc_amd import _fused, _lib  # noqa: E402

import f16_plan_cases as C  # noqa: E402


def host_table():
    L, F = _lib.lib(), _fused.lib()
    rows, seen = [], {}
    for tag, fields in C.plan_cases():
        got = C.probe(L, fields)
        accepted = [v >= 0 for v in got[0::2]]
        assert all(v >= -1 for v in got[0::2]) and accepted[1] == accepted[2], (fields, got)
        assert (tag == "rejected") == (not any(accepted)) or tag == "grid", (tag, fields, got)
        for split in (False, True):
            if accepted[split]:
                key = (fields["ksize"], fields["stride"], fields["dilation"]) + ((1,) if fields["transposed"] else ())
                seen.setdefault((split, key), set()).add((fields["Cout"], fields["algo"]))
        rows.append([fields[k] for k in C.FIELDS] + got)
    for name, (split, key, cout, algo) in C.FORMS.items():          # every form is reached by an accepted row
        assert (cout, algo) in seen[(split, tuple(key))], name
    out = os.path.join(HERE, "f16_plan_table.json")
    with open(out, "w") as f:
        json.dump({"fields": C.FIELDS, "probes": C.PROBES, "rows": rows, "null_calls": C.null_calls(L, F)}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(rows)} rows, {os.path.getsize(out)} bytes -> {out}")


def gpu_table():
    import torch
    dev = torch.device("cuda:0")
    cells = {name: C.run_form(name, torch, dev) for name in C.FORMS}
    cells["K3X, x batch stride + 64"] = C.run_form("K3X", torch, dev, x_pad=64)
    out = os.path.join(HERE, "f16_plan_gpu.json")
    with open(out, "w") as f:
        json.dump(cells, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    accepted = sum(1 for c in cells.values() for k, v in c.items() if k != "packed" and v[0] == 0)
    print(f"{len(cells)} forms, {accepted} accepted and {sum(len(c) - 1 for c in cells.values()) - accepted} rejected cells -> {out}")


if __name__ == "__main__":
    gpu_table() if "--gpu" in sys.argv[1:] else host_table()
