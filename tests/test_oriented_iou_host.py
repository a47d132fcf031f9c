"""CPU checks of the oriented-IoU losses (snvc_amd.thirdparty.oriented_iou_loss, snvc_amd.models.iou_loss,
include/snvc_oiou.h): the float64 reference of tests/oriented_iou_cases.py against closed forms, against two other
algorithms and against central differences; the case table's margins; the module's torch route against the reference; the
corner order against the reference's own box2corners_th (tests/golden/oriented_iou_corners.npz); the four loss functions and
classes against a float64 composition written out here; the header against the binding and the library's exports."""
import ctypes
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oriented_iou_cases as K
from snvc_amd import _lib, _oiou
from snvc_amd.models import iou_loss, loss3d
from snvc_amd.thirdparty import oriented_iou_loss as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "snvc_oiou.h")
ROWS = {r.name: r for r in K.table()}
CFG = K.CFG


# ---------------------------------------------------------------------------------------------------- the reference itself
def _square(side, alpha=0.0, cx=0.0, cy=0.0):
    return K.ref_corners([cx, cy, side, side, alpha], cx, cy)


def test_reference_closed_forms():
    assert abs(K.ref_inter(_square(2.0), _square(2.0, math.pi / 4)) - 8 * (math.sqrt(2) - 1)) < 1e-14
    assert abs(K.ref_inter(_square(2.0, 0.3), _square(2.0, 0.3)) - 4.0) < 1e-14
    assert K.ref_inter(_square(2.0), _square(2.0, 0.4, 5.0, 0.0)) == 0.0
    assert abs(K.ref_inter(_square(1.0, 0.2, 0.1, -0.1), _square(4.0, 1.0)) - 1.0) < 1e-14
    assert abs(K.ref_inter(_square(4.0, 1.0), _square(1.0, 0.2, 0.1, -0.1)) - 1.0) < 1e-14
    # a clip polygon given clockwise is walked the other way round
    assert abs(K.ref_inter(_square(2.0), _square(2.0, math.pi / 4)[::-1]) - 8 * (math.sqrt(2) - 1)) < 1e-14
    # the enclosing rectangle of two unit squares side by side is 2 x 1, whichever edge it is found from
    w, h = K.ref_enclosing(_square(1.0) + _square(1.0, 0.0, 1.0, 0.0), K.SMALLEST)
    assert sorted([round(w, 12), round(h, 12)]) == [1.0, 2.0]
    assert K.ref_enclosing(_square(1.0) + _square(1.0, 0.0, 1.0, 2.0), K.ALIGNED) == (2.0, 3.0)


def _candidate_points_area(S, C):
    """Convex x convex: the vertices of either inside the other and the edge crossings, ordered by angle, shoelace."""
    def inside(p, Q):
        sgn = 1.0 if K.signed_area(Q) >= 0 else -1.0
        return all(sgn * K.cross(Q[(k + 1) % 4][0] - Q[k][0], Q[(k + 1) % 4][1] - Q[k][1], p[0] - Q[k][0], p[1] - Q[k][1]) >= 0 for k in range(4))
    pts = [p for p in S if inside(p, C)] + [p for p in C if inside(p, S)]
    for i in range(4):
        p, q = S[i], S[(i + 1) % 4]
        for k in range(4):
            a, b = C[k], C[(k + 1) % 4]
            den = K.cross(q[0] - p[0], q[1] - p[1], b[0] - a[0], b[1] - a[1])
            if den == 0:
                continue
            t = K.cross(a[0] - p[0], a[1] - p[1], b[0] - a[0], b[1] - a[1]) / den
            s = K.cross(a[0] - p[0], a[1] - p[1], q[0] - p[0], q[1] - p[1]) / den
            if 0 <= t <= 1 and 0 <= s <= 1:
                pts.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    if len(pts) < 3:
        return 0.0
    mx, my = sum(p[0] for p in pts) / len(pts), sum(p[1] for p in pts) / len(pts)
    pts.sort(key=lambda p: math.atan2(p[1] - my, p[0] - mx))
    return abs(K.signed_area(pts))


def _triangle_split_area(S, C):
    """The subject cut along the diagonal from its reflex vertex, two convex clips."""
    orient = 1.0 if K.signed_area(S) >= 0 else -1.0
    turns = K._turns(S)
    k = next((i for i in range(4) if orient * turns[i] < 0), 0)
    tri1, tri2 = [S[k], S[(k + 1) % 4], S[(k + 2) % 4]], [S[k], S[(k + 2) % 4], S[(k + 3) % 4]]
    return K.ref_inter(tri1, C) + K.ref_inter(tri2, C)


def _shapes(row):
    return [K.shapes_of(row.form, row.a[m], row.b[m]) for m in range(row.M)]


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.cls != "quads_reflex"])
def test_clip_equals_candidate_points_and_is_symmetric_on_convex_rows(name):
    """Every row whose subject is convex, the identical / parallel / contained rows (coincident vertices, shared edge directions)
    included."""
    for S, C in _shapes(ROWS[name]):
        area = K.ref_inter(S, C)
        assert abs(area - _candidate_points_area(S, C)) <= 1e-12
        assert abs(area - K.ref_inter(C, S)) <= 1e-12
        assert abs(area - _triangle_split_area(S, C)) <= 1e-12


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.cls == "quads_reflex"])
def test_clip_equals_triangle_split_on_reflex_rows(name):
    for S, C in _shapes(ROWS[name]):
        assert abs(K.ref_inter(S, C) - _triangle_split_area(S, C)) <= 1e-12


@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.check_grads and r.M <= 5])
def test_reference_gradients_equal_central_differences(name):
    row = ROWS[name]
    _, grads = K.reference(name)
    flat = np.concatenate([g.reshape(row.M, -1) for g in grads], axis=1)
    ops = [t.copy() for t in row.operands()]
    eps = 1e-5

    def total(m):
        out = K.ref_pair(row.form, row.kind, row.enc, *K._pair_args(row, m, ops))
        return sum(row.gout[m, k] * out[k] for k in range(8))
    for m in range(row.M):
        col = 0
        for t in ops:
            view = t[m].reshape(-1)          # a view: writes reach `ops`
            for i in range(view.size):
                keep = view[i]
                view[i] = keep + eps
                up = total(m)
                view[i] = keep - eps
                down = total(m)
                view[i] = keep
                assert abs((up - down) / (2 * eps) - flat[m, col]) <= 1e-6 * np.abs(flat[m]).max(), (name, m, col)
                col += 1


def test_every_row_is_clear_of_the_margins():
    assert len(ROWS) == len(K.SIZES) * 9 and {r.M for r in ROWS.values()} == set(K.SIZES)
    for row in ROWS.values():
        assert row.a.shape[0] == row.M
        for S, C in _shapes(row):
            assert K.margin_a(S, C) >= K.MARGIN_AREA, row.name
            if row.check_grads:
                assert K.margin_b(S, C) >= K.MARGIN_DIST and K.margin_c(S, C) >= K.MARGIN_ANGLE, row.name
        for t in row.operands():
            assert np.array_equal(t, t.astype(np.float32).astype(np.float64))


# ---------------------------------------------------------------------------------------------------- the torch route
@pytest.mark.parametrize("name", sorted(ROWS))
def test_torch_route_equals_the_reference(name):
    row = ROWS[name]
    ref, gref = K.reference(name)
    out, grads = K.route_outputs(row, torch.float64)
    # per element: 1e-12 of the element, absolute below 1
    assert (np.abs(out - ref) <= 1e-12 * np.maximum(1.0, np.abs(ref))).all(), np.abs(out - ref).max()
    if gref is not None:
        for g, r in zip(grads, gref):
            assert (np.abs(g - r) <= 1e-12 * np.maximum(1.0, np.abs(r))).all(), np.abs(g - r).max()
    out32, grads32 = K.route_outputs(row, torch.float32)
    err = np.abs(out32 - ref)
    assert err[:, [_oiou.IOU, _oiou.LOSS]].max() <= 1e-5, err[:, [_oiou.IOU, _oiou.LOSS]].max()
    assert all(np.isfinite(g).all() for g in grads32)
    if row.cls == "identical":
        assert np.abs(out32[:, _oiou.IOU] - 1.0).max() <= 1e-6


def test_public_functions_select_the_outputs():
    row = ROWS["generic-5"]
    ref = np.array([[[K._f(v) for v in K.ref_pair(K.BOXES, kind, K.SMALLEST, list(row.a[m]), list(row.b[m]))] for m in range(5)]
                    for kind in (K.DIOU, K.GIOU)])
    b1, b2 = torch.tensor(row.a)[None], torch.tensor(row.b)[None]
    loss, iou, overlap = O.cal_diou(b1, b2, return_overlap=True)
    assert loss.shape == iou.shape == overlap.shape == (1, 5)
    assert np.abs(loss[0].numpy() - ref[0][:, 7]).max() < 1e-12 and np.abs(overlap[0].numpy() - ref[0][:, 0]).max() < 1e-12
    assert len(O.cal_diou(b1, b2)) == 2
    gloss, giou = O.cal_giou(b1, b2)
    assert np.abs(gloss[0].numpy() - ref[1][:, 7]).max() < 1e-12 and torch.equal(giou, iou)
    iou2, c1, c2, u = O.cal_iou(b1, b2)
    assert torch.equal(iou2, iou) and np.abs(u[0].numpy() - ref[0][:, 3]).max() < 1e-12
    assert torch.equal(c1, O.box2corners_th(b1)) and c2.shape == (1, 5, 4, 2)
    area, none = O.oriented_box_intersection_2d(c1, c2)
    assert none is None and np.abs(area[0].numpy() - ref[0][:, 0]).max() < 1e-12
    w, h = O.enclosing_box(c1, c2)
    assert np.abs(w[0].numpy() - ref[0][:, 5]).max() < 1e-12 and np.abs(h[0].numpy() - ref[0][:, 6]).max() < 1e-12
    wa, ha = O.enclosing_box(c1, c2, "aligned")
    both = torch.cat([c1, c2], dim=2)[0]
    assert torch.equal(wa[0], both[..., 0].amax(1) - both[..., 0].amin(1)) and torch.equal(ha[0], both[..., 1].amax(1) - both[..., 1].amin(1))
    with pytest.raises(NotImplementedError):
        O.enclosing_box(c1, c2, "pca")
    # the closed form, through the public name
    sq = torch.tensor([[[0.0, 0.0, 2.0, 2.0, 0.0]]], dtype=torch.float64)
    turned = torch.tensor([[[0.0, 0.0, 2.0, 2.0, math.pi / 4]]], dtype=torch.float64)
    assert abs(float(O.cal_diou(sq, turned, return_overlap=True)[2]) - 8 * (math.sqrt(2) - 1)) < 1e-14
    # the two operands pair up row by row: another count is refused before anything runs
    with pytest.raises(ValueError, match="one shape"):
        O.cal_diou(b1, b2[:, :4])
    with pytest.raises(ValueError, match="centres"):
        O.pair_outputs(_oiou.QUADS, _oiou.DIOU, _oiou.SMALLEST, c1[0], c2[0], torch.zeros(4, 2), torch.zeros(4, 2))
    # no pairs: empty results of the right shape
    empty = O.cal_diou(b1[:, :0], b2[:, :0])
    assert empty[0].shape == (1, 0)


def test_results_do_not_depend_on_where_the_pair_lies():
    row = ROWS["generic-64"]
    a, b = torch.tensor(row.a, dtype=torch.float32), torch.tensor(row.b, dtype=torch.float32)
    a[:, :2], b[:, :2] = torch.round(a[:, :2] * 1024) / 1024, torch.round(b[:, :2] * 1024) / 1024
    shift = torch.tensor([64.0, -64.0, 0.0, 0.0, 0.0])          # exact in float32 for centres on a 2^-10 grid
    here = O.cal_diou(a[None], b[None])
    there = O.cal_diou((a + shift)[None], (b + shift)[None])
    assert torch.equal(here[0], there[0]) and torch.equal(here[1], there[1])


def test_corner_order_equals_the_references():
    gold = np.load(os.path.join(ROOT, "tests", "golden", "oriented_iou_corners.npz"))
    assert np.array_equal(gold["boxes"], K.corner_boxes())
    ours = O.box2corners_th(torch.from_numpy(gold["boxes"]))
    assert ours.shape == (2, 10, 4, 2)
    # float32 on both sides, coordinates up to 36: a few units in the last place of 36
    assert np.abs(ours.numpy() - gold["corners"]).max() <= 8 * 36 * 2.0 ** -24
    exact = O.box2corners_th(torch.from_numpy(gold["boxes"]).double()).numpy()
    for bi in range(2):
        for n in range(10):
            box = [float(v) for v in gold["boxes"][bi, n]]
            assert np.abs(exact[bi, n] - np.array(K.ref_corners(box, box[0], box[1]))).max() <= 1e-13


# ---------------------------------------------------------------------------------------------------- models/iou_loss.py
def _corner_loss_ref(pred, gt):
    """compute_IoU_loss_corner per pair on the float64 reference."""
    loss, iou = [], []
    for p, g in zip(pred, gt):
        pc = [tuple(0.5 * (p[i] + p[j])) for i, j in zip(K.SELECT_IND1, K.SELECT_IND2)]
        gc = [tuple(g[i]) for i in K.SELECT_IND1]
        out = K.ref_pair(K.QUADS, K.DIOU, K.SMALLEST, pc, gc, list(p[0]), list(g[0]))
        loss.append(out[7])
        iou.append(out[4])
    return np.array(loss), np.array(iou)


def test_compute_iou_loss_corner_equals_its_composition():
    gt = K.parts(7, 1)
    pred = gt + np.random.default_rng(2).normal(0, 0.15, gt.shape)
    keep = pred.copy()
    tp = torch.tensor(pred)[None].requires_grad_()
    loss, iou = iou_loss.compute_IoU_loss_corner(tp, torch.tensor(gt)[None])
    ref_loss, ref_iou = _corner_loss_ref(pred, gt)
    assert loss.shape == iou.shape == (1, 7)
    assert np.abs(loss[0].detach().numpy() - ref_loss).max() <= 1e-12 and np.abs(iou[0].detach().numpy() - ref_iou).max() <= 1e-12
    loss.sum().backward()
    assert torch.isfinite(tp.grad).all() and float(tp.grad.abs().max()) > 0 and np.array_equal(pred, keep)


def _iou3d_ref(pred, gt, idx):
    out = []
    for p, g in zip(pred, gt):
        bev = K.ref_pair(K.BOXES, K.DIOU, K.SMALLEST, list(p[idx]), list(g[idx]))[0]
        hov = max(min(p[1] + p[3] / 2, g[1] + g[3] / 2) - max(p[1] - p[3] / 2, g[1] - g[3] / 2), 0.0)
        o3 = bev * hov
        out.append(o3 / max(p[3] * p[4] * p[5] + g[3] * g[4] * g[5] - o3, 1e-6))
    return np.array(out)


def test_approximated_3d_iou_and_bbox3d_loss_equal_their_composition():
    pred, gt = K.boxes7(7, 3)
    idx = [0, 2, 5, 4, 6]
    got = iou_loss.approximated_3d_iou_pt(torch.tensor(pred), torch.tensor(gt), idx)
    assert np.abs(got.numpy() - _iou3d_ref(pred, gt, idx)).max() <= 1e-12
    # Bbox3DLoss: sizes are relative to the proposals
    samples = np.random.default_rng(4).uniform(0.1, 0.3, (7, 7))
    raw = np.concatenate([pred, np.zeros((7, 2))], axis=1)
    outputs, data = {"bbox": torch.tensor(raw, requires_grad=True)}, {"gt_box_local": torch.tensor(gt), "samples": samples}
    res = iou_loss.Bbox3DLoss(types.SimpleNamespace(head_reg_type="vector3d"))(outputs, data)
    size = np.zeros((7, 7))
    size[:, 3:6] = samples[:, :3]
    p2, g2 = pred + size, gt + size
    assert set(res) == {"sl1", "IoU3D"}
    assert abs(float(res["IoU3D"].detach()) - (1 - _iou3d_ref(p2, g2, idx)).mean()) <= 1e-12
    assert abs(float(res["sl1"].detach()) - 0.5 * float(F.smooth_l1_loss(torch.tensor(p2), torch.tensor(g2), beta=0.2))) <= 1e-15
    (res["sl1"] + res["IoU3D"]).backward()
    assert torch.isfinite(outputs["bbox"].grad).all() and float(outputs["bbox"].grad[:, 7:].abs().max()) == 0
    assert np.array_equal(outputs["bbox"].detach().numpy(), raw) and np.array_equal(data["gt_box_local"].numpy(), gt)      # nothing written
    as_list = iou_loss.Bbox3DLoss()(outputs, dict(data, samples=[s[None] for s in samples]))
    assert float(as_list["IoU3D"].detach()) == float(res["IoU3D"].detach())
    masked = iou_loss.Bbox3DLoss()
    masked.use_reg_mask = True
    with pytest.raises(NotImplementedError, match="synchronisation"):
        masked(outputs, data)


@pytest.mark.parametrize("normalize_gt", [False, True])
def test_coordinate_iou_loss_equals_its_composition(normalize_gt):
    gt = K.parts(7, 5)
    pred = gt + np.random.default_rng(6).normal(0, 0.1, gt.shape)
    corners3 = np.zeros((7, 9, 3))
    corners3[:, :, 0], corners3[:, :, 2] = gt[:, :, 0], gt[:, :, 1]
    gt_used = gt.copy()
    if normalize_gt:
        gt_used[:, :, 0] = (gt[:, :, 0] - CFG.x_range[0]) / 3.2
        gt_used[:, :, 1] = (gt[:, :, 1] - CFG.z_range[0]) / 4.8
    meta = {"gt_corners_local": torch.tensor(corners3)}
    keep = corners3.copy()
    got = iou_loss.CoordinateIoULoss(CFG, IoU_type="corner", normalize_gt=normalize_gt)({"coordinates": torch.tensor(pred)}, meta)
    ref = 0.1 * np.abs(pred - gt_used).mean() + _corner_loss_ref(pred, gt_used)[0].mean()
    assert abs(float(got) - ref) <= 1e-12 and np.array_equal(meta["gt_corners_local"].numpy(), keep)
    # 'bbox': the box is decoded from five logits
    r = np.random.default_rng(8)
    raw = r.normal(0, 0.5, (7, 5))
    s = 1 / (1 + np.exp(-raw))
    dec = np.stack([(2 * s[:, 0] - 1) * 3.2, (2 * s[:, 1] - 1) * 4.8, s[:, 2] * 3.2, s[:, 3] * 4.8, s[:, 4] * 2 * math.pi], axis=1)
    gt_box = dec + r.normal(0, 0.2, dec.shape)
    meta["gt_box_local"] = torch.tensor(gt_box)
    outputs = {"coordinates": torch.tensor(pred), "bbox": torch.tensor(raw)}
    got = iou_loss.CoordinateIoULoss(CFG, IoU_type="bbox", normalize_gt=normalize_gt)(outputs, meta)
    diou = np.mean([K.ref_pair(K.BOXES, K.DIOU, K.SMALLEST, list(d), list(g))[7] for d, g in zip(dec, gt_box)])
    assert abs(float(got) - (0.1 * np.abs(pred - gt_used).mean() + diou)) <= 1e-12
    assert np.array_equal(outputs["bbox"].numpy(), raw)
    with pytest.raises(ValueError):
        iou_loss.CoordinateIoULoss(CFG, IoU_type="other")


def test_loss3d_names_still_raise_and_point_here():
    t = torch.zeros(2, 7)
    for fn in (lambda: loss3d.compute_IoU_loss_corner(t, t), lambda: loss3d.approximated_3d_iou_pt(t, t, [0, 2, 5, 4, 6]),
               lambda: loss3d.BboxLoss(types.SimpleNamespace(head_reg_type="vector3d")),
               lambda: loss3d.CoordinateLoss(CFG, enable_IoU=True)):
        with pytest.raises(NotImplementedError):
            fn()
    for obj in (loss3d.compute_IoU_loss_corner, loss3d.approximated_3d_iou_pt, loss3d.BboxLoss, loss3d.CoordinateLoss):
        assert "snvc_amd.models.iou_loss" in obj.__doc__


# ---------------------------------------------------------------------------------------------------- binding, alias
def test_header_and_binding_agree():
    """The struct's mirror, the constants and the tie rule; names, parameters and the ABI number are held by
    tests/test_abi_tables_host.py."""
    text = open(HEADER).read()
    fields = re.findall(r"^\s+(?:const\s+)?(?:int32_t|int64_t|float)\s*\*?\s*(\w+);", re.search(r"typedef struct snvc_oiou_desc \{(.*?)\}", text, re.S).group(1), re.M)
    assert fields == [n for n, _ in _oiou.OiouDesc._fields_]
    assert int(re.search(r"#define SNVC_OIOU_OUT (\d+)", text).group(1)) == _oiou.OUT
    source = open(os.path.join(ROOT, "snvc_amd", "csrc", "oriented_iou.hip")).read()
    # one tie rule in all three: 32 epsilons of the arithmetic at hand
    assert "kTie = 32.f * 1.1920929e-7f;" in source and np.float32(1.1920929e-7) == np.finfo(np.float32).eps
    assert O.TIE_EPSILONS == 32 and K.TIE == 32 * np.finfo(np.float64).eps
    assert K.SELECT_IND1 == loss3d.SELECT_IND1 and K.SELECT_IND2 == loss3d.SELECT_IND2


def test_the_c_calls_check_their_arguments_before_any_launch():
    L = _oiou.lib()
    err = _lib.lib().snvc_last_error_string
    d = _oiou.OiouDesc()
    assert L.snvc_oiou_forward(ctypes.byref(d), None) == 0 and L.snvc_oiou_backward(ctypes.byref(d), None) == 0      # M = 0: nothing to do
    assert L.snvc_oiou_forward(None, None) == 1 and b"null descriptor" in err()
    d.M = 4
    assert L.snvc_oiou_forward(ctypes.byref(d), None) == 1 and b"null pointer" in err()
    d.a = d.b = d.out = 16
    d.form = _oiou.QUADS
    assert L.snvc_oiou_forward(ctypes.byref(d), None) == 1 and b"null pointer" in err()            # the centres
    d.form = _oiou.BOXES
    assert L.snvc_oiou_backward(ctypes.byref(d), None) == 1 and b"null pointer" in err()           # gout, ga, gb
    d.out = 20
    assert L.snvc_oiou_forward(ctypes.byref(d), None) == 1 and b"aligned" in err()
    d.out, d.M = 16, -1
    assert L.snvc_oiou_forward(ctypes.byref(d), None) == 1 and b"negative" in err()
    d.M = 1 << 31
    assert L.snvc_oiou_forward(ctypes.byref(d), None) == 2
    d.M = 4
    for field, text in (("form", b"form"), ("kind", b"kind"), ("enclosing", b"enclosing"), ("reserved", b"reserved")):
        setattr(d, field, 7)
        assert L.snvc_oiou_forward(ctypes.byref(d), None) == 1 and text in err(), field
        setattr(d, field, 0)


def test_install_as_snvc_aliases_the_module():
    import snvc_amd
    saved = {k: sys.modules.get(k) for k in list(snvc_amd._ALIASES) + ["snvc", "snvc.models", "snvc.extension", "snvc.thirdparty"]}
    try:
        snvc_amd.install_as_snvc(backbone=False)
        from snvc.thirdparty.oriented_iou_loss import cal_diou, enclosing_box, oriented_box_intersection_2d
        assert cal_diou is O.cal_diou and enclosing_box is O.enclosing_box and oriented_box_intersection_2d is O.oriented_box_intersection_2d
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
