"""Writes tests/golden/x3_form_table.json: the kernel form the split-mode launch-size rule picks, over a grid of layers,
launch sizes and knob settings.

    python tests/golden/make_golden_x3_form.py

Run it ONLY at a commit where the rule is still the method ``Conv3dLayerX3._pick_form`` (the parent of the commit that made it
the module function ``ops.x3_form``): the table is a record of what that method returned, which tests/test_x3_form_host.py
holds ``x3_form`` to.  The method reads only attributes of ``self`` and the module knobs, so it runs without a device on
``object.__new__(ops.Conv3dLayerX3)`` with those attributes set (``algo`` as the constructor leaves it: ``int(forced or 0)``).

The file holds the grid's axes, the five forms, and one digit per row (an index into ``forms``) in the order of
``itertools.product`` over the axes as listed in ``order``.  The script asserts that every ``return`` statement of the method
is reached by at least one row and that each of the five forms occurs.
"""
import inspect
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True

from snvc_amd import _lib, ops  # noqa: E402

FORMS = [0, _lib.ALGO_X3_SERIAL, _lib.ALGO_X3_NARROW, _lib.ALGO_X3_SMALL, _lib.ALGO_X3_Q16]
AXES = {
    # knob settings: the defaults, and each of the three 16x16x32 switches off
    "knobs": [{}, {"X3_Q16": False}, {"X3_Q16_K5": False}, {"X3_Q16_S2": False}],
    "cout": [1, 8, 32, 64, 96, 128, 192],
    "ksize": [3, 5, 7],
    # (stride, transposed, dilation)
    "geometry": [[1, False, 1], [2, False, 1], [2, True, 1], [1, False, 2]],
    "n": [1, 2],
    # output extents (D, H, W).  With n = 1: 16x16x480 | 512 are 240 | 256 stride-1 tiles (X3_Q16_MIN_JOBS at cout 32), 16x32x480 | 512 are
    # 480 | 512 (the 5^3 / 7^3 rule's 512 jobs, the 512 tiles of a 32-channel layer, the 1024 32-channel jobs of a 64-channel one),
    # 32x32x480 | 512 are 960 | 1024 (the serial-plane form's 1024 64-channel jobs), 64x64x448 | 512 are 3584 | 4096 workgroups of a
    # transposed layer; the last three are the workload's quarter, half and full resolution
    "out_sp": [[2, 2, 3], [3, 5, 31], [4, 6, 36], [8, 12, 40], [16, 16, 256], [16, 16, 480], [16, 16, 512], [16, 32, 480], [16, 32, 512],
               [32, 32, 480], [32, 32, 512], [64, 64, 448], [64, 64, 512], [48, 24, 78], [96, 48, 156], [192, 96, 312]],
    "plain": [False, True],
    "split_out": [False, True],
    "forced": [None, 0, _lib.ALGO_X3_SMALL, _lib.ALGO_X3_Q16],
}
ORDER = ["knobs", "cout", "ksize", "geometry", "n", "out_sp", "plain", "split_out", "forced"]


def main():
    pick = ops.Conv3dLayerX3._pick_form
    src, first = inspect.getsourcelines(pick)
    returns = {first + i for i, line in enumerate(src) if line.strip().startswith("return ")}
    reached = {}

    def tracer(frame, event, arg):
        if frame.f_code is not pick.__code__:
            return None
        if event == "return":
            reached.setdefault(frame.f_lineno, set()).add(arg)
        return tracer

    digits = []
    defaults = {k: getattr(ops, k)[0] for k in ("X3_Q16", "X3_Q16_K5", "X3_Q16_S2")}
    sys.settrace(tracer)
    try:
        for knobs, cout, ksize, (stride, transposed, dilation), n, out_sp, plain, split_out, forced in itertools.product(*(AXES[k] for k in ORDER)):
            for k, v in defaults.items():
                getattr(ops, k)[0] = knobs.get(k, v)
            lay = object.__new__(ops.Conv3dLayerX3)
            lay.cout, lay.ksize, lay.stride, lay.dilation, lay.transposed = cout, ksize, stride, dilation, transposed
            lay.forced_algo, lay.algo = forced, int(forced or 0)
            digits.append(str(FORMS.index(pick(lay, n, tuple(out_sp), plain=plain, split_out=split_out))))
    finally:
        sys.settrace(None)
        for k, v in defaults.items():
            getattr(ops, k)[0] = v
    assert set(reached) == returns, f"return statements never reached: lines {sorted(returns - set(reached))}"
    assert set(digits) == set("01234"), "every form must occur"
    for line in sorted(reached):
        print(f"ops.py:{line}: {len(reached[line])} value(s) {sorted(reached[line])}   {src[line - first].strip()[:90]}")
    out = os.path.join(HERE, "x3_form_table.json")
    with open(out, "w") as f:
        json.dump({"order": ORDER, "axes": AXES, "forms": FORMS, "rows": "".join(digits)}, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(digits)} rows, {len(returns)} return statements, {os.path.getsize(out)} bytes -> {out}")


if __name__ == "__main__":
    main()
