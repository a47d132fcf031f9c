"""Writes tests/golden/oriented_iou_corners.npz: the corners the reference's own ``box2corners_th``
(snvc/utils/torch_utils.py:131-162) gives for the 20 boxes of ``oriented_iou_cases.corner_boxes()``; it pins the corner order
of ``snvc_amd.thirdparty.oriented_iou_loss.box2corners_th``.

    python tests/golden/make_golden_oriented_iou.py          (SNVC_REFERENCE=<checkout>, default /root/reference)

Needs the reference checkout (its torch_utils.py is imported on the CPU, by path, not copied); the tests need only the file.

    boxes      (2,10,5) float32: the inputs, as drawn from the cases' seed
    corners    (2,10,4,2) float32: the reference's output
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
REF = os.environ.get("SNVC_REFERENCE", "/root/reference")

import oriented_iou_cases as K  # noqa: E402

_spec = importlib.util.spec_from_file_location("ref_torch_utils", os.path.join(REF, "snvc", "utils", "torch_utils.py"))
ref = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ref)


def main():
    boxes = K.corner_boxes()
    corners = ref.box2corners_th(torch.from_numpy(boxes)).numpy()
    out = os.path.join(ROOT, "tests", "golden", "oriented_iou_corners.npz")
    np.savez(out, boxes=boxes, corners=corners)
    print(f"wrote {out}: boxes {boxes.shape}, corners {corners.shape}")


if __name__ == "__main__":
    main()
