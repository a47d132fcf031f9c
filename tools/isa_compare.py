#!/usr/bin/env python3
"""Compare the device code of kernels between two `hipcc -S --cuda-device-only` listings.

    tools/isa_compare.py OLD.s NEW.s PATTERN [--map OLD_SUBSTR=NEW_SUBSTR ...]

For every kernel of NEW.s whose demangled-agnostic symbol contains PATTERN: its register counts and scratch size, and -- when a
kernel of OLD.s maps onto it (same symbol after the --map substitutions) -- whether the instruction streams are identical
(labels and symbol names normalised).  Used for profiles/fused_first_layer/device_code_identity.txt.
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if ".amdhsa_kernel " + name not in text:
            continue
        ins = []
        for line in body.splitlines():
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                continue
            ins.append(line)
        out[name] = ins
    meta = {}
    for m in re.finditer(r"\.amdhsa_kernel (\w+)(.*?)\.end_amdhsa_kernel", text, re.S):
        f = dict(re.findall(r"\.amdhsa_(\w+)\s+(\S+)", m.group(2)))
        for key in ("num_vgpr", "private_seg_size"):      # newer listings give symbols there and the numbers in .set lines
            hit = re.search(r"\.set " + re.escape(m.group(1)) + r"\." + key + r", (\d+)", text)
            if hit:
                f[key] = hit.group(1)
        meta[m.group(1)] = f
    return out, meta


def norm(ins, name):
    res = []
    for line in ins:
        line = line.replace(name, "KERNEL")
        line = re.sub(r"\.?LBB\d+_(\d+)", r"L\1", line)
        res.append(line)
    return res


def main():
    old_path, new_path, pat = sys.argv[1:4]
    maps = [a.split("=", 1) for a in sys.argv[5:]] if len(sys.argv) > 4 and sys.argv[4] == "--map" else []
    old, _ = kernels(old_path)
    new, meta = kernels(new_path)
    for name in sorted(new):
        if pat not in name:
            continue
        f = meta.get(name, {})
        line = (f"{name}: vgpr {f.get('num_vgpr', f.get('next_free_vgpr'))} "
                f"scratch {f.get('private_seg_size', f.get('private_segment_fixed_size'))} instructions {len(new[name])}")
        cands = [o for o in old if _apply(o, maps) == name]
        if cands:
            same = norm(old[cands[0]], cands[0]) == norm(new[name], name)
            line += f" | parent {cands[0]}: {'IDENTICAL' if same else 'DIFFERENT'} ({len(old[cands[0]])} instructions)"
        else:
            line += " | new"
        print(line)


def _apply(name, maps):
    for a, b in maps:
        name = name.replace(a, b)
    return name


if __name__ == "__main__":
    main()
