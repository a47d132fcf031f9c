"""Host-side face of ``snvc.extension.iou3d_nms`` on the HIP kernels (``include/snvc_iou3d.h``).

Written against the reference module's INTERFACE (snvc/extension/iou3d_nms/iou3d_nms_utils.py: the public names,
their argument order and what each returns), not its bodies.  The reference file cannot be imported as shipped
(``common_utils`` does not exist, :10; ``numerical_jaccobian`` imports the removed ``torch._six``).

    boxes_bev_iou_cpu(boxes_a, boxes_b)            -> (N, M) BEV IoU on the host; numpy in, numpy out      (:16-32)
    boxes_iou_bev(boxes_a, boxes_b)                -> (N, M) BEV IoU                                         (:35-49)
    boxes_iou3d_gpu(boxes_a, boxes_b)              -> (N, M) 3D IoU, one fused launch                        (:52-85)
    nms_gpu(boxes, scores, thresh, pre_maxsize)    -> (kept indices into boxes, None), rotated BEV IoU       (:88-103)
    nms_normal_gpu(boxes, scores, thresh)          -> (kept indices into boxes, None), axis-aligned          (:106-120)
    boxes_iou3d_gpu_differentiable(boxes_a, boxes_b) -> (N,) one-by-one 3D IoU; d/d boxes_a by central
                                                      differences (eps 1e-3) as the reference's backward    (:123-177)

Boxes are [x, y, z, dx, dy, dz, heading].  The BEV overlap is the reference's definition, not exact geometry: the
crossings of the two outlines plus each box's corners that lie inside the OTHER box grown by 1e-2 on each
half-extent.  Two boxes a few millimetres apart therefore overlap a little (2x2 boxes 5 mm apart: IoU 0.0013), and
a corner within 1e-2 of the other box counts.  An exact clip would move IoUs by up to ~3e-3 for such pairs and
change NMS decisions next to the threshold, so the margin is kept on purpose.

NMS sorts by score with torch as the reference does, then runs two HIP launches (the upper-triangle suppression
mask, then the greedy pass in one workgroup); only the kept count (4 bytes) is read back to size the result.  At most
65536 boxes (after ``pre_maxsize``) go into one NMS call: the mask alone is then 512 MB.

``iou3d_nms_cuda`` carries the seven names of the pybind module (iou3d_nms_api.cpp:11-19) with their contracts:
outputs are filled in place and each returns an int (``nms_gpu`` / ``nms_normal_gpu`` fill a CPU LongTensor ``keep``
and return how many entries are valid).  Importing this module loads no library and does not touch the GPU.
"""
import ctypes
import types

import numpy as np
import torch

from ... import _iou3d
from ..._lib import check
from ...ops import _gpu, _ptr, _stream
from . import numerical_jaccobian  # noqa: F401  (the reference module's sibling, kept importable)


def _boxes(t, name):
    if t.dim() != 2 or t.shape[1] != 7:
        raise AssertionError(f"{name} must be (N, 7) [x, y, z, dx, dy, dz, heading]")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")


def _contiguous_gpu(t, name):
    _gpu(t, name)
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _pairwise(boxes_a, boxes_b, out, what, onebyone):
    for t, nm in ((boxes_a, "boxes_a"), (boxes_b, "boxes_b"), (out, "ans")):
        _contiguous_gpu(t, nm)
    _boxes(boxes_a, "boxes_a")
    _boxes(boxes_b, "boxes_b")
    na, nb = boxes_a.shape[0], boxes_b.shape[0]
    if onebyone and nb != na:
        raise AssertionError("one-by-one forms need as many boxes_b as boxes_a")
    if out.dtype != torch.float32 or out.numel() != (na if onebyone else na * nb):
        raise RuntimeError("ans must be float32 with one element per result")
    L = _iou3d.lib()
    ws = None
    if not onebyone and na * nb:
        ws = torch.empty((L.snvc_iou3d_pairwise_workspace_bytes(na, nb),), dtype=torch.uint8, device=boxes_a.device)
    with torch.cuda.device(boxes_a.device):
        check(L.snvc_iou3d_pairwise(_ptr(boxes_a), na, _ptr(boxes_b), nb, what, int(onebyone), _ptr(ws), _ptr(out),
                                    _stream(boxes_a)), "snvc_iou3d_pairwise")
    return 1


def _nms_device(boxes, thresh, kind):
    """boxes sorted by rank, on the GPU -> (keep int64 [n] on the device, number of valid entries)."""
    _contiguous_gpu(boxes, "boxes")
    _boxes(boxes, "boxes")
    n = boxes.shape[0]
    if n > _iou3d.NMS_MAX_BOXES:
        raise ValueError(f"NMS takes at most {_iou3d.NMS_MAX_BOXES} boxes per call, got {n} (use pre_maxsize)")
    L = _iou3d.lib()
    ws = torch.empty((max(L.snvc_iou3d_nms_workspace_bytes(n), 1),), dtype=torch.uint8, device=boxes.device)
    keep = torch.empty((n,), dtype=torch.int64, device=boxes.device)
    num = torch.empty((1,), dtype=torch.int32, device=boxes.device)
    with torch.cuda.device(boxes.device):
        check(L.snvc_iou3d_nms(_ptr(boxes), n, float(thresh), kind, _ptr(ws), _ptr(keep), _ptr(num), _stream(boxes)),
              "snvc_iou3d_nms")
    return keep, int(num.item())


def _nms_into(boxes, keep, thresh, kind):
    if keep.is_cuda or keep.dtype != torch.int64 or not keep.is_contiguous() or keep.numel() < boxes.shape[0]:
        raise RuntimeError("keep must be a contiguous CPU LongTensor with one entry per box")
    kept, n = _nms_device(boxes, thresh, kind)
    keep[:n].copy_(kept[:n])
    return n


def _iou_bev_cpu(boxes_a, boxes_b, ans_iou):
    for t, nm in ((boxes_a, "boxes_a"), (boxes_b, "boxes_b"), (ans_iou, "ans_iou")):
        if t.is_cuda:
            raise RuntimeError(f"{nm} must be a CPU tensor")
        if not t.is_contiguous():
            raise RuntimeError(f"{nm} must be contiguous")
    _boxes(boxes_a, "boxes_a")
    _boxes(boxes_b, "boxes_b")
    na, nb = boxes_a.shape[0], boxes_b.shape[0]
    if ans_iou.dtype != torch.float32 or ans_iou.numel() != na * nb:
        raise RuntimeError("ans_iou must be float32 (N, M)")
    check(_iou3d.lib().snvc_iou3d_boxes_iou_bev_cpu(ctypes.c_void_p(boxes_a.data_ptr()), na,
                                                    ctypes.c_void_p(boxes_b.data_ptr()), nb,
                                                    ctypes.c_void_p(ans_iou.data_ptr())), "boxes_iou_bev_cpu")
    return 1


iou3d_nms_cuda = types.SimpleNamespace(
    boxes_overlap_bev_gpu=lambda a, b, ans: _pairwise(a, b, ans, _iou3d.OVERLAP, False),
    boxes_overlap_bev_onebyone_gpu=lambda a, b, ans: _pairwise(a, b, ans, _iou3d.OVERLAP, True),
    boxes_iou_bev_gpu=lambda a, b, ans: _pairwise(a, b, ans, _iou3d.IOU_BEV, False),
    boxes_iou_bev_onebyone_gpu=lambda a, b, ans: _pairwise(a, b, ans, _iou3d.IOU_BEV, True),
    nms_gpu=lambda boxes, keep, thresh: _nms_into(boxes, keep, thresh, _iou3d.NMS_ROTATED),
    nms_normal_gpu=lambda boxes, keep, thresh: _nms_into(boxes, keep, thresh, _iou3d.NMS_NORMAL),
    boxes_iou_bev_cpu=_iou_bev_cpu,
)


def boxes_bev_iou_cpu(boxes_a, boxes_b):
    """(N, 7), (M, 7) host boxes -> (N, M) BEV IoU; numpy arrays in give a numpy array out."""
    is_numpy = isinstance(boxes_a, np.ndarray) or isinstance(boxes_b, np.ndarray)
    a = torch.from_numpy(np.ascontiguousarray(boxes_a, np.float32)) if isinstance(boxes_a, np.ndarray) else boxes_a
    b = torch.from_numpy(np.ascontiguousarray(boxes_b, np.float32)) if isinstance(boxes_b, np.ndarray) else boxes_b
    if a.is_cuda or b.is_cuda:
        raise AssertionError("Only support CPU tensors")
    if a.shape[1] != 7 or b.shape[1] != 7:
        raise AssertionError("boxes must be (N, 7)")
    ans_iou = a.new_zeros((a.shape[0], b.shape[0]))
    iou3d_nms_cuda.boxes_iou_bev_cpu(a.contiguous(), b.contiguous(), ans_iou)
    return ans_iou.numpy() if is_numpy else ans_iou


def _matrix(boxes_a, boxes_b, what):
    if boxes_a.shape[1] != 7 or boxes_b.shape[1] != 7:
        raise AssertionError("boxes must be (N, 7)")
    _gpu(boxes_a, "boxes_a")
    ans = torch.empty((boxes_a.shape[0], boxes_b.shape[0]), dtype=torch.float32, device=boxes_a.device)
    _pairwise(boxes_a.contiguous(), boxes_b.contiguous(), ans, what, False)
    return ans


def boxes_iou_bev(boxes_a, boxes_b):
    """(N, 7), (M, 7) GPU boxes -> (N, M) BEV IoU."""
    return _matrix(boxes_a, boxes_b, _iou3d.IOU_BEV)


def boxes_iou3d_gpu(boxes_a, boxes_b):
    """(N, 7), (M, 7) GPU boxes -> (N, M) 3D IoU: BEV overlap x height overlap over the union volume (floor 1e-6)."""
    return _matrix(boxes_a, boxes_b, _iou3d.IOU_3D)


def _nms(boxes, scores, thresh, pre_maxsize, kind):
    if boxes.shape[1] != 7:
        raise AssertionError("boxes must be (N, 7)")
    _gpu(boxes, "boxes")
    order = scores.sort(0, descending=True)[1]
    if pre_maxsize is not None:
        order = order[:pre_maxsize]
    keep, n = _nms_device(boxes[order].contiguous(), thresh, kind)
    return order[keep[:n]].contiguous(), None


def nms_gpu(boxes, scores, thresh, pre_maxsize=None, **kwargs):
    """Rotated NMS: boxes (N, 7), scores (N,) on the GPU -> (indices into boxes of the kept ones by descending score,
    None)."""
    return _nms(boxes, scores, thresh, pre_maxsize, _iou3d.NMS_ROTATED)


def nms_normal_gpu(boxes, scores, thresh, **kwargs):
    """Axis-aligned NMS (heading ignored), same contract as ``nms_gpu`` without ``pre_maxsize``."""
    return _nms(boxes, scores, thresh, None, _iou3d.NMS_NORMAL)


def _iou3d_onebyone(boxes_a, boxes_b):
    if boxes_a.shape[1] != 7 or boxes_b.shape[1] != 7:
        raise AssertionError("boxes must be (N, 7)")
    _gpu(boxes_a, "boxes_a")
    ans = torch.empty((boxes_a.shape[0],), dtype=torch.float32, device=boxes_a.device)
    _pairwise(boxes_a.detach().contiguous(), boxes_b.detach().contiguous(), ans, _iou3d.IOU_3D, True)
    return ans


class BoxesIou3dDifferentiableFunction(torch.autograd.Function):
    """boxes_a (N, 7), boxes_b (N, 7) -> (N,) 3D IoU of pair i.  The gradient reaches ``boxes_a`` only; it is the
    reference's numerical Jacobian (central differences, eps 1e-3, in fp32) times the incoming gradient, evaluated by
    one HIP kernel (``snvc_iou3d_backward``)."""

    EPS = 1e-3

    @staticmethod
    def call_func(input):
        boxes_a, boxes_b = input
        return _iou3d_onebyone(boxes_a, boxes_b)

    @staticmethod
    def forward(ctx, boxes_a, boxes_b):
        ctx.save_for_backward(boxes_a, boxes_b)
        return BoxesIou3dDifferentiableFunction.call_func((boxes_a, boxes_b))

    @staticmethod
    def backward(ctx, grad):
        boxes_a, boxes_b = ctx.saved_tensors
        a = boxes_a.detach().contiguous()
        b = boxes_b.detach().contiguous()
        g = grad.detach().float().contiguous()
        for t, nm in ((a, "boxes_a"), (b, "boxes_b"), (g, "grad")):
            _contiguous_gpu(t, nm)
        _boxes(a, "boxes_a")
        _boxes(b, "boxes_b")
        grad_a = torch.empty_like(a)
        with torch.cuda.device(a.device):
            check(_iou3d.lib().snvc_iou3d_backward(_ptr(a), _ptr(b), _ptr(g), a.shape[0],
                                                   BoxesIou3dDifferentiableFunction.EPS, _ptr(grad_a), _stream(a)),
                  "snvc_iou3d_backward")
        return grad_a, None


boxes_iou3d_gpu_differentiable = BoxesIou3dDifferentiableFunction.apply
