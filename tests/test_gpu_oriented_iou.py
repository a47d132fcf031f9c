"""The oriented-IoU kernels (csrc/oriented_iou.hip) against the float64 reference of tests/oriented_iou_cases.py, on every row
of its table.

Values: 1e-5 absolute on ``iou`` and ``loss`` (the project's bound for losses, tests/test_gpu_loss.py), 1e-5 of
``area1 + area2`` on ``inter`` and ``u``, 1e-5 relative on ``enc_w`` and ``enc_h``.

Gradients (rows outside ``VALUES_ONLY``): those of ``sum(gout * out)`` for the row's seeded ``gout``, compared with the float64
gradient in units of the table-wide largest gradient magnitude of the same input column.  The yardstick is the worst such
error of the module's float32 torch route on the CPU over the same rows -- a number of the table, not of the kernel -- and the
HIP route is held to four times it: the four covers the device's float32 sin / cos and another order of summation.
Measured (profiles/oriented_iou/accuracy.txt): torch route 1.19e-06, HIP route 8.90e-07 at worst (bound 4.74e-06).
"""
import numpy as np
import pytest
import torch

import guarded as GD
import oriented_iou_cases as K
from snvc_amd import _oiou
from snvc_amd.models import iou_loss, loss3d
from snvc_amd.thirdparty import oriented_iou_loss as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = {r.name: r for r in K.table()}
FACTOR = 4.0
_cache = {}


def hip_outputs(name):
    if ("hip", name) not in _cache:
        _cache["hip", name] = K.route_outputs(ROWS[name], torch.float32, DEV)
    return _cache["hip", name]


def yardstick():
    """(scales, the float32 CPU torch route's worst gradient error over the table)."""
    if "yard" not in _cache:
        scales = K.grad_scales()
        worst = max(K.grad_error(r, K.route_outputs(r, torch.float32)[1], scales) for r in ROWS.values() if r.check_grads)
        print(f"float32 CPU torch route, worst gradient error over the table: {worst:.3e}")
        assert 0 < worst < 1e-4, worst           # float32 of well-conditioned rows; anything else means the table is broken
        _cache["yard"] = scales, worst
    return _cache["yard"]


@pytest.mark.parametrize("name", sorted(ROWS))
def test_values_against_float64(name):
    row = ROWS[name]
    ref = K.reference(name)[0]
    out = hip_outputs(name)[0]
    assert out.shape == ref.shape == (row.M, 8)
    err = np.abs(out - ref)
    areas = ref[:, _oiou.AREA1] + ref[:, _oiou.AREA2]
    figures = {"iou": err[:, _oiou.IOU].max(), "loss": err[:, _oiou.LOSS].max(),
               "inter/areas": (err[:, _oiou.INTER] / areas).max(), "u/areas": (err[:, _oiou.UNION] / areas).max(),
               "area1/areas": (err[:, _oiou.AREA1] / areas).max(), "area2/areas": (err[:, _oiou.AREA2] / areas).max(),
               "w rel": (err[:, _oiou.ENC_W] / ref[:, _oiou.ENC_W]).max(), "h rel": (err[:, _oiou.ENC_H] / ref[:, _oiou.ENC_H]).max()}
    print(name, {k: f"{v:.2e}" for k, v in figures.items()})
    for what, v in figures.items():
        assert v <= 1e-5, f"{name}: {what} off by {v:.3e}"
    if row.cls == "identical":
        assert np.abs(out[:, _oiou.IOU] - 1.0).max() <= 1e-6


@pytest.mark.parametrize("name", sorted(ROWS))
def test_gradients_against_float64(name):
    row = ROWS[name]
    grads = hip_outputs(name)[1]
    assert [g.shape for g in grads] == [t.shape for t in row.operands()]
    assert all(np.isfinite(g).all() for g in grads), f"{name}: a gradient is not finite"
    if not row.check_grads:
        return
    scales, torch_worst = yardstick()
    err = K.grad_error(row, grads, scales)
    print(f"{name}: HIP gradient error {err:.3e}, float32 torch route at worst {torch_worst:.3e}, bound {FACTOR * torch_worst:.3e}")
    assert err <= FACTOR * torch_worst, f"{name}: gradient error {err:.3e} above {FACTOR} x {torch_worst:.3e}"


def _run(row, device=DEV):
    a, b, ca, cb = row.tensors(torch.float32, device, requires_grad=True)
    out = O.pair_outputs(row.form, row.kind, row.enc, a, b, ca, cb)
    total = (out * torch.tensor(row.gout, dtype=torch.float32, device=device)).sum()
    torch.autograd.backward([total])          # not Tensor.backward: inside guarded() that call would hide the backward's allocations
    return [out.detach()] + [t.grad for t in (a, b, ca, cb) if t is not None]


@pytest.mark.parametrize("name", ["generic-257", "quads_reflex-257"])
def test_two_runs_give_the_same_bits(name):
    first, second = _run(ROWS[name]), _run(ROWS[name])
    assert all(torch.equal(x, y) for x, y in zip(first, second))


def test_no_pairs():
    box = torch.zeros(1, 0, 5, device=DEV, requires_grad=True)
    loss, iou = O.cal_diou(box, box.detach())
    assert loss.shape == iou.shape == (1, 0) and loss.is_cuda
    loss.sum().backward()
    assert box.grad.shape == (1, 0, 5)
    quads = torch.zeros(1, 0, 4, 2, device=DEV)
    assert O.oriented_box_intersection_2d(quads, quads)[0].shape == (1, 0)


def test_routing_of_other_inputs():
    """Non-contiguous operands are copied and served by the kernels; a CPU or float64 operand takes the torch route; a second
    operand on the CPU or in float64 follows the first."""
    row = ROWS["generic-64"]
    a, b = torch.tensor(row.a, dtype=torch.float32, device=DEV), torch.tensor(row.b, dtype=torch.float32, device=DEV)
    dense = O.cal_diou(a[None], b[None])
    wide = torch.zeros(64, 9, device=DEV)
    wide[:, 2:7] = a
    strided = O.cal_diou(wide[None, :, 2:7], b[None])
    assert not wide[:, 2:7].is_contiguous() and torch.equal(strided[0], dense[0]) and torch.equal(strided[1], dense[1])
    mixed = O.cal_diou(a[None], torch.tensor(row.b)[None])                        # float64 on the CPU
    assert mixed[0].is_cuda and torch.equal(mixed[0], dense[0])
    on_cpu = O.cal_diou(a.cpu()[None], b.cpu()[None])
    assert not on_cpu[0].is_cuda and float((on_cpu[0] - dense[0].cpu()).abs().max()) <= 1e-5
    in_double = O.cal_diou(a.double()[None], b.double()[None])
    assert in_double[0].dtype == torch.float64 and in_double[0].is_cuda
    with loss3d._torch_route():
        switched = O.cal_diou(a[None], b[None])
    assert float((switched[0] - dense[0]).abs().max()) <= 1e-5 and float((in_double[0] - dense[0]).abs().max()) <= 1e-5


@pytest.mark.parametrize("misalign", [0, 16])
@pytest.mark.parametrize("name", [n for n, r in ROWS.items() if r.M == 64])
def test_inside_guard_bands(name, misalign):
    """The M = 64 rows between guard zones (tests/guarded.py): nothing outside the tensors is written, and the outputs and
    gradients have the bits of the unguarded run."""
    GD.run_case(lambda: _run(ROWS[name]), DEV, misalign, what=f"oriented_iou {name}")


# ---------------------------------------------------------------------------------------------------- the losses over it
def _both_routes(make):
    """(loss, gradient) of ``make(leaf)`` on the HIP route and on the torch route, for the same float32 GPU leaf."""
    results = []
    for torch_route in (False, True):
        leaf, fn = make()
        if torch_route:
            with loss3d._torch_route():
                loss = fn(leaf)
        else:
            loss = fn(leaf)
        loss.backward()
        results.append((float(loss.detach()), leaf.grad.clone()))
    return results


def _agree(results, what):
    (l0, g0), (l1, g1) = results
    gerr = float((g0 - g1).abs().max()) / max(float(g1.abs().max()), 1e-30)
    print(f"{what}: loss {l0:.7f} (HIP) {l1:.7f} (torch), gradient difference {gerr:.2e} of the largest")
    assert abs(l0 - l1) <= 1e-5 and gerr <= 1e-5 and bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0, what


def _clear(form, a, b):
    """The pair is clear of the table's margins (a)-(c), measured on its float32 values: where it is not, two float32
    evaluations may differ by far more than rounding, and a comparison at 1e-5 says nothing."""
    f32 = lambda t: np.asarray(t, dtype=np.float32).astype(np.float64)          # noqa: E731
    return K.clear_of_margins("generic", *K.shapes_of(form, f32(a), f32(b)))


def _drawn(n, draw, seed):
    """n instances from ``draw(rng)`` -> (arrays..., clear), redrawn until clear; stacked per array."""
    kept = []
    while len(kept) < n:
        *arrays, ok = draw(np.random.default_rng(seed))
        seed += 1
        if ok:
            kept.append(arrays)
    return [np.stack(col) for col in zip(*kept)]


def test_bbox3d_loss_equals_the_torch_route():
    idx = iou_loss.Bbox3DLoss().indices

    def draw(r):
        pred, gt = K.boxes7(1, int(r.integers(1 << 30)))
        sample = r.uniform(0.1, 0.3, 7)
        size = np.zeros(7)
        size[3:6] = sample[:3]
        return pred[0], gt[0], sample, _clear(K.BOXES, (pred[0] + size)[idx], (gt[0] + size)[idx])
    pred, gt, samples = _drawn(7, draw, 300)
    data = {"gt_box_local": torch.tensor(gt, dtype=torch.float32), "samples": samples}

    def make():
        leaf = torch.tensor(np.concatenate([pred, np.zeros((7, 2))], axis=1), dtype=torch.float32, device=DEV, requires_grad=True)
        return leaf, lambda x: sum(iou_loss.Bbox3DLoss()({"bbox": x}, data).values())
    _agree(_both_routes(make), "Bbox3DLoss")


@pytest.mark.parametrize("iou_type", ["corner", "bbox"])
def test_coordinate_iou_loss_equals_the_torch_route(iou_type):
    crit = iou_loss.CoordinateIoULoss(K.CFG, IoU_type=iou_type)
    first, second = loss3d.SELECT_IND1, loss3d.SELECT_IND2

    def draw(r):
        gt = K.parts(1, int(r.integers(1 << 30)))[0]
        pred = gt + r.normal(0, 0.15, gt.shape)
        raw = r.normal(0, 0.5, 5)
        gt_box = crit.decode_bbox(torch.tensor(raw, dtype=torch.float32)[None])[0].double().numpy() + r.normal(0, 0.2, 5)
        if iou_type == "corner":
            ok = _clear(K.QUADS, 0.5 * (np.float32(pred)[first] + np.float32(pred)[second]), gt[first])
        else:
            ok = _clear(K.BOXES, crit.decode_bbox(torch.tensor(raw, dtype=torch.float32)[None])[0].double().numpy(), gt_box)
        return gt, pred, raw, gt_box, ok
    gt, pred, raw, gt_box = _drawn(7, draw, 500)
    corners3 = np.zeros((7, 9, 3))
    corners3[:, :, 0], corners3[:, :, 2] = gt[:, :, 0], gt[:, :, 1]
    meta = {"gt_corners_local": torch.tensor(corners3, dtype=torch.float32), "gt_box_local": torch.tensor(gt_box, dtype=torch.float32)}

    def make():
        if iou_type == "corner":
            leaf = torch.tensor(pred, dtype=torch.float32, device=DEV, requires_grad=True)
            return leaf, lambda x: crit({"coordinates": x}, meta)
        leaf = torch.tensor(raw, dtype=torch.float32, device=DEV, requires_grad=True)
        coords = torch.tensor(pred, dtype=torch.float32, device=DEV)
        return leaf, lambda x: crit({"coordinates": coords, "bbox": x}, meta)
    _agree(_both_routes(make), f"CoordinateIoULoss({iou_type})")


def test_a_diou_loss_trains_the_fc_box_head():
    """The FC box head (snvc_amd.models.FCmodel, HIP training route) under the DIoU loss of its decoded box: the gradient
    reaches every weight matrix and norm parameter, and equals the one the torch route of the loss sends back."""
    from snvc_amd.models.FCmodel import get_fc_model
    crit = iou_loss.CoordinateIoULoss(K.CFG, IoU_type="bbox")
    r = np.random.default_rng(11)
    x = torch.tensor(r.normal(0, 1, (8, 18)), dtype=torch.float32, device=DEV)
    gt_box = torch.tensor(np.stack([r.uniform(-1, 1, 8), r.uniform(-1, 1, 8), r.uniform(1.4, 1.8, 8), r.uniform(2, 3, 8), r.uniform(0, 6, 8)], axis=1),
                          dtype=torch.float32)
    grads = []
    for torch_route in (False, True):
        torch.manual_seed(3)
        head = get_fc_model().to(DEV).train()
        torch.manual_seed(4)                                     # the dropout masks
        box = head(x)
        assert box.shape == (8, 5)
        if torch_route:
            with loss3d._torch_route():
                loss = O.cal_diou(crit.decode_bbox(box)[None], gt_box[None])[0].mean()
        else:
            loss = O.cal_diou(crit.decode_bbox(box)[None], gt_box[None])[0].mean()
        loss.backward()
        grads.append([p.grad.clone() for p in head.parameters()])
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads[0])
    # every weight matrix and every norm parameter is reached; a Linear bias in front of a BatchNorm has a zero gradient by construction
    named = dict(zip([n for n, _ in head.named_parameters()], grads[0]))
    assert all(float(g.abs().max()) > 0 for n, g in named.items() if g.dim() == 2 or "batch_norm" in n), [n for n, g in named.items() if float(g.abs().max()) == 0]
    scale = max(float(g.abs().max()) for g in grads[1])
    worst = max(float((g0 - g1).abs().max()) for g0, g1 in zip(*grads)) / scale
    print(f"FC head under DIoU: parameter gradients differ between the loss's routes by {worst:.2e} of the largest")
    assert worst <= 1e-5
