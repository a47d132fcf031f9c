"""The rotated-box IoU / NMS family on the MI355X against the reference's own CPU function (tests/golden/iou3d_ref.npz,
made by tests/golden/make_golden_iou3d.py): every pairwise form, NMS keep lists of both kinds, the in-place contracts of
``iou3d_nms_cuda``, the differentiable 3D IoU and its central-difference backward, self-consistency of a large NMS, and
bitwise repeatability."""
import os

import numpy as np
import pytest
import torch

from snvc_amd.extension.iou3d_nms import iou3d_nms_utils as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "iou3d_ref.npz"))
BEV_CASES = sorted({k.split("_")[1] for k in GOLD.files if k.startswith("bev_")})
NMS_SCENES = sorted({tuple(k.split("_")[1:3]) for k in GOLD.files if k.startswith("nms_") and k.endswith("_boxes")},
                    key=lambda s: (int(s[0]), float(s[1])))
DEV = "cuda:0"
TOL = 2e-5


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _cmp(got, ref, valid, what):
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)[valid]
    assert err.size == 0 or err.max() < TOL, (what, float(err.max()))


def _derived3d(a, b, bev):
    """float64 3D IoU of pairs (a_i, b_i) from the reference's BEV IoU (iou3d_nms_utils.py:53-85)."""
    a, b, bev = a.astype(np.float64), b.astype(np.float64), bev.astype(np.float64)
    sa, sb = a[:, 3] * a[:, 4], b[:, 3] * b[:, 4]
    ov = bev * (sa + sb) / (1 + bev)
    h = np.clip(np.minimum(a[:, 2] + a[:, 5] / 2, b[:, 2] + b[:, 5] / 2) - np.maximum(a[:, 2] - a[:, 5] / 2, b[:, 2] - b[:, 5] / 2), 0, None)
    o3 = ov * h
    return o3 / np.maximum(a[:, 3] * a[:, 4] * a[:, 5] + b[:, 3] * b[:, 4] * b[:, 5] - o3, 1e-6)


@pytest.mark.parametrize("case", BEV_CASES)
def test_pairwise_matrix_forms(case):
    a, b, valid = GOLD[f"bev_{case}_a"], GOLD[f"bev_{case}_b"], GOLD[f"bev_{case}_valid"]
    A, B = _dev(a), _dev(b)
    _cmp(U.boxes_iou_bev(A, B), GOLD[f"bev_{case}_iou"], valid, "iou_bev")
    _cmp(U.boxes_iou3d_gpu(A, B), GOLD[f"bev_{case}_iou3d"], valid, "iou3d")
    ov = torch.full((len(a), len(b)), -1.0, device=DEV)
    assert U.iou3d_nms_cuda.boxes_overlap_bev_gpu(A, B, ov) == 1
    # overlap is in m^2: the reference's own fp32 error grows with the boxes' area, the bound with it
    sab = (a[:, 3] * a[:, 4])[:, None].astype(np.float64) + (b[:, 3] * b[:, 4])[None]
    err = (np.abs(ov.cpu().numpy() - GOLD[f"bev_{case}_overlap"]) / np.maximum(sab, 1.0))[valid]
    assert err.max() < TOL, float(err.max())
    iou = torch.full((len(a), len(b)), -1.0, device=DEV)
    assert U.iou3d_nms_cuda.boxes_iou_bev_gpu(A, B, iou) == 1
    assert torch.equal(iou, U.boxes_iou_bev(A, B))


@pytest.mark.parametrize("case", BEV_CASES)
def test_pairwise_onebyone_forms(case):
    a, b, valid = GOLD[f"bev_{case}_a"], GOLD[f"bev_{case}_b"], GOLD[f"bev_{case}_valid"]
    n = min(len(a), len(b))
    A, B = _dev(a[:n]), _dev(b[:n])
    diag = np.arange(n)
    out = torch.full((n,), -1.0, device=DEV)
    assert U.iou3d_nms_cuda.boxes_iou_bev_onebyone_gpu(A, B, out) == 1
    _cmp(out, GOLD[f"bev_{case}_iou"][diag, diag], valid[diag, diag], "iou_bev one-by-one")
    assert U.iou3d_nms_cuda.boxes_overlap_bev_onebyone_gpu(A, B, out) == 1
    ov = torch.full((n, n), 0.0, device=DEV)
    U.iou3d_nms_cuda.boxes_overlap_bev_gpu(A, B, ov)
    assert torch.allclose(out, ov.diagonal(), rtol=1e-6, atol=1e-6)   # same geometry code (fused differently per kernel)
    _cmp(U.boxes_iou3d_gpu_differentiable(A, B), GOLD[f"bev_{case}_iou3d"][diag, diag], valid[diag, diag], "iou3d one-by-one")


def test_empty_and_odd_sizes():
    a = _dev(GOLD["bev_kitti0_a"])
    z = torch.zeros((0, 7), device=DEV)
    assert U.boxes_iou_bev(z, a).shape == (0, len(a)) and U.boxes_iou3d_gpu(a, z).shape == (len(a), 0)
    for n, m in ((1, 1), (63, 65), (65, 129), (130, 1)):
        got = U.boxes_iou_bev(a[:n], a[:m]).cpu().numpy()
        _cmp(torch.from_numpy(got), GOLD["bev_kitti0_iou"][:n, :m], GOLD["bev_kitti0_valid"][:n, :m], f"{n}x{m}")
    keep, _ = U.nms_gpu(z, torch.zeros(0, device=DEV), 0.5)
    assert keep.numel() == 0
    keep, _ = U.nms_normal_gpu(a[:1], torch.ones(1, device=DEV), 0.5)
    assert keep.tolist() == [0]


@pytest.mark.parametrize("n,t", NMS_SCENES)
def test_nms_keep_lists_equal_the_reference(n, t):
    boxes, scores = _dev(GOLD[f"nms_{n}_{t}_boxes"]), _dev(GOLD[f"nms_{n}_{t}_scores"])
    thresh = float(t)
    order = np.argsort(-GOLD[f"nms_{n}_{t}_scores"], kind="stable")
    rank = np.empty_like(order)
    rank[order] = np.arange(len(order))
    for kind, fn in (("rotated", U.nms_gpu), ("normal", U.nms_normal_gpu)):
        ref = GOLD[f"nms_{n}_{t}_{kind}_keep"]
        keep, none = fn(boxes, scores, thresh)
        assert none is None and keep.dtype == torch.int64 and keep.device == boxes.device
        assert np.array_equal(keep.cpu().numpy(), ref), (kind, n, t)
    ref = GOLD[f"nms_{n}_{t}_rotated_keep"]
    for pre in (int(n), int(n) + 5, max(int(n) // 3, 1)):
        keep, _ = U.nms_gpu(boxes, scores, thresh, pre_maxsize=pre)
        # greedy decisions for a box depend only on higher-ranked boxes: the top-`pre` result is a prefix filter
        assert np.array_equal(keep.cpu().numpy(), ref[rank[ref] < pre]), (n, t, pre)


def test_pybind_nms_contracts():
    n, t = NMS_SCENES[-1]
    boxes, scores = GOLD[f"nms_{n}_{t}_boxes"], GOLD[f"nms_{n}_{t}_scores"]
    order = np.argsort(-scores, kind="stable")
    sb = _dev(boxes[order])
    for kind, fn in (("rotated", U.iou3d_nms_cuda.nms_gpu), ("normal", U.iou3d_nms_cuda.nms_normal_gpu)):
        keep = torch.full((len(order),), -7, dtype=torch.long)            # CPU LongTensor, filled in place
        num = fn(sb, keep, float(t))
        assert isinstance(num, int)
        assert np.array_equal(order[keep[:num].numpy()], GOLD[f"nms_{n}_{t}_{kind}_keep"])
        assert (keep[num:] == -7).all()
    with pytest.raises(RuntimeError):
        U.iou3d_nms_cuda.nms_gpu(sb, torch.zeros(len(order), dtype=torch.long, device=DEV), 0.5)   # keep must be on the CPU
    with pytest.raises(ValueError, match="65536"):
        U.nms_gpu(torch.zeros((65537, 7), device=DEV), torch.rand(65537, device=DEV), 0.5)


def test_differentiable_iou_forward_and_backward():
    a, b, g = GOLD["jac_a"], GOLD["jac_b"], GOLD["jac_grad"]
    bev, valid = GOLD["jac_bev"], GOLD["jac_valid"]
    A = _dev(a).requires_grad_(True)
    out = U.boxes_iou3d_gpu_differentiable(A, _dev(b))
    _cmp(out.detach(), _derived3d(a, b, bev[:, 0]), valid, "forward")
    out.backward(_dev(g))
    eps = np.float32(1e-3)
    ref = np.zeros_like(a, dtype=np.float64)
    for k in range(7):
        lo, hi = a.copy(), a.copy()
        lo[:, k] = a[:, k] - eps
        hi[:, k] = a[:, k] + eps
        ref[:, k] = (_derived3d(hi, b, bev[:, 2 + 2 * k]) - _derived3d(lo, b, bev[:, 1 + 2 * k])) / (2 * 1e-3) * g
    err = np.abs(A.grad.cpu().numpy() - ref)[valid]
    assert err.max() < 2e-3, float(err.max())
    assert (np.abs(ref[valid]) > 1e-2).sum() > 20                         # the pairs do overlap and move


def test_large_nms_is_self_consistent():
    r = np.random.default_rng(5)
    n = 16384
    boxes = np.concatenate([r.uniform(0, 70, (n, 1)), r.uniform(-40, 40, (n, 1)), r.uniform(-2, 0, (n, 1)),
                            r.uniform(0.5, 4.5, (n, 2)), r.uniform(1.4, 1.8, (n, 1)), r.uniform(-np.pi, np.pi, (n, 1))], 1)
    B, S = _dev(boxes.astype(np.float32)), torch.rand(n, device=DEV)
    thresh = 0.1
    order = S.sort(0, descending=True)[1]
    sb = B[order].contiguous()
    iou = U.boxes_iou_bev(sb, sb)                                         # rows: higher-ranked box first
    for run in range(2):
        keep, _ = U.nms_gpu(B, S, thresh)
        if run:
            assert torch.equal(keep, first)                              # bitwise identical on a repeat
        first = keep
    rank = torch.empty_like(order)
    rank[order] = torch.arange(n, device=DEV)
    kr = rank[keep].sort()[0]
    assert torch.equal(rank[keep], kr)                                    # returned in score order
    kept = torch.zeros(n, dtype=torch.bool, device=DEV)
    kept[kr] = True
    sub = iou[kr][:, kr]
    assert (torch.triu(sub, 1) <= thresh).all()                           # no kept pair above the threshold
    over = torch.triu(iou > thresh, 1) & kept[:, None]                    # kept i suppresses later j
    assert torch.equal(over.any(0), ~kept)                                # every suppressed box has its reason
    assert 100 < kr.numel() < n


def test_repeat_runs_are_bitwise_identical():
    a = _dev(GOLD["bev_kitti0_a"])
    for fn in (U.boxes_iou_bev, U.boxes_iou3d_gpu):
        assert torch.equal(fn(a, a), fn(a, a))
    n, t = NMS_SCENES[-1]
    boxes, scores = _dev(GOLD[f"nms_{n}_{t}_boxes"]), _dev(GOLD[f"nms_{n}_{t}_scores"])
    assert torch.equal(U.nms_normal_gpu(boxes, scores, float(t))[0], U.nms_normal_gpu(boxes, scores, float(t))[0])
    A = _dev(GOLD["jac_a"]).requires_grad_(True)
    grads = []
    for _ in range(2):
        A.grad = None
        U.boxes_iou3d_gpu_differentiable(A, _dev(GOLD["jac_b"])).sum().backward()
        grads.append(A.grad.clone())
    assert torch.equal(grads[0], grads[1])
