"""Differentiable IoU, DIoU and GIoU of oriented boxes and of quadrilaterals: the ``snvc.thirdparty.oriented_iou_loss`` that
the reference's ``loss3d.py`` calls (``cal_diou``, ``oriented_box_intersection_2d``, ``enclosing_box``) and never shipped.
No source exists for it; DESIGN.md "Oriented IoU" holds the definitions this module and its kernels are written from.

A pair is (subject, clip).  Per pair, eight numbers are computed together:

    inter, area1, area2, u = area1 + area2 - inter, iou = inter / u, enc_w, enc_h, loss

``inter`` is the exact area of the subject clipped (Sutherland-Hodgman, a point on a clip line is inside) against the four
half-planes of the clip shape; the clip shape must be convex, the subject simple (convex, or one reflex vertex).
``enc_w, enc_h`` are the sides of the least-area rectangle flush with a line through two of the eight corners
(``"smallest"``), or of the axis-aligned box (``"aligned"``).  ``loss`` is ``1 - iou + d^2 / (enc_w^2 + enc_h^2)`` (DIoU, ``d``
the distance of the centres) or ``1 - iou + (enc_w enc_h - u) / (enc_w enc_h)`` (GIoU).  Before any product of coordinates both
shapes are moved so that the clip shape's centre is the origin, so a result does not depend on where the pair lies.
Non-finite or degenerate input gives IEEE results; nothing is checked.

Routes.  Float32 GPU operands take the HIP route: one ``torch.autograd.Function`` over one forward and one backward launch
(``csrc/oriented_iou.hip``, ``include/snvc_oiou.h``); non-contiguous operands are copied first, and a second operand on
another device or of another dtype is brought to the first one's.  Everything else -- CPU tensors, float64, and any call
inside ``loss3d._torch_route()`` -- takes a torch route written from the same definitions, vectorised over the pairs.
"""
import ctypes
import itertools

import torch
from torch.autograd.function import once_differentiable

from .. import _lib, _oiou

__all__ = ["box2corners_th", "oriented_box_intersection_2d", "enclosing_box", "cal_iou", "cal_diou", "cal_giou"]

TIE_EPSILONS = 32                # enclosing candidates within this many machine epsilons, relatively, are a tie: the first one stays
_LOCAL_X = (0.5, -0.5, -0.5, 0.5)
_LOCAL_Y = (0.5, 0.5, -0.5, -0.5)
_SLOTS = 16                      # vertices kept per polygon on the torch route
_PAIRS = tuple(itertools.combinations(range(8), 2))


def _enclosing_code(enclosing_type):
    if enclosing_type == "smallest":
        return _oiou.SMALLEST
    if enclosing_type == "aligned":
        return _oiou.ALIGNED
    if enclosing_type == "pca":
        raise NotImplementedError("enclosing_type 'pca' is not built")
    raise ValueError(f"unknown enclosing_type {enclosing_type!r}")


# ------------------------------------------------------------------------------ corners
def _corners(box, cx, cy):
    """Corners [..., 4, 2] of ``box`` [..., 5] about the centre (cx, cy) [...]."""
    lx = box.new_tensor(_LOCAL_X) * box[..., 2:3]
    ly = box.new_tensor(_LOCAL_Y) * box[..., 3:4]
    sin, cos = torch.sin(box[..., 4:5]), torch.cos(box[..., 4:5])
    return torch.stack([lx * cos - ly * sin + cx[..., None], lx * sin + ly * cos + cy[..., None]], dim=-1)


def box2corners_th(box):
    """(B,N,5) ``[x, y, w, h, alpha]`` -> (B,N,4,2): the local corners (+,+), (-,+), (-,-), (+,-) times (w/2, h/2), turned
    counter-clockwise by ``alpha`` and moved to (x, y)."""
    return _corners(box, box[..., 0], box[..., 1])


# ------------------------------------------------------------------------------ the torch route
def _cross(ax, ay, bx, by):
    return ax * by - ay * bx


def _clip_area(S, C):
    """Area [M] of the polygons S [M,4,2] clipped against the half-planes of the convex quadrilaterals C [M,4,2]."""
    M, K = S.shape[0], _SLOTS
    twice_c = sum(_cross(C[:, k, 0], C[:, k, 1], C[:, (k + 1) % 4, 0], C[:, (k + 1) % 4, 1]) for k in range(4))
    sgn = torch.where(twice_c >= 0, 1.0, -1.0).to(S.dtype)[:, None]
    poly = torch.cat([S, S.new_zeros(M, K - 4, 2)], dim=1)
    cnt = torch.full((M,), 4, dtype=torch.long, device=S.device)
    slot = torch.arange(K, device=S.device)[None, :]
    for e in range(4):
        a, edge = C[:, e], C[:, (e + 1) % 4] - C[:, e]
        valid = slot < cnt[:, None]
        prev_slot = (slot - 1) % cnt.clamp(min=1)[:, None]
        dist = sgn * _cross(edge[:, None, 0], edge[:, None, 1], poly[..., 0] - a[:, None, 0], poly[..., 1] - a[:, None, 1])
        dist_prev = torch.gather(dist, 1, prev_slot)
        prev = torch.gather(poly, 1, prev_slot[..., None].expand(M, K, 2))
        inside, inside_prev = dist >= 0, dist_prev >= 0
        crossing = valid & (inside != inside_prev)
        t = dist_prev / torch.where(crossing, dist_prev - dist, torch.ones_like(dist))
        cut = prev + t[..., None] * (poly - prev)
        # per edge: the crossing point, then the end point if it is inside
        both = torch.stack([cut, poly], dim=2).reshape(M, 2 * K, 2)
        keep = torch.stack([crossing, valid & inside], dim=2).reshape(M, 2 * K)
        order = torch.argsort((~keep).to(torch.int8), dim=1, stable=True)[:, :K]
        cnt = keep.sum(dim=1).clamp(max=K)
        kept = slot < cnt[:, None]
        poly = torch.where(kept[..., None], torch.gather(both, 1, order[..., None].expand(M, K, 2)), torch.zeros_like(poly))
    valid = slot < cnt[:, None]
    nxt = torch.gather(poly, 1, ((slot + 1) % cnt.clamp(min=1)[:, None])[..., None].expand(M, K, 2))
    twice = torch.where(valid, _cross(poly[..., 0], poly[..., 1], nxt[..., 0], nxt[..., 1]), torch.zeros_like(poly[..., 0])).sum(dim=1)
    return 0.5 * twice.abs()


def _enclosing(P, code):
    """(w, h) [M] of the enclosing rectangles of the points P [M,8,2]."""
    if code == _oiou.ALIGNED:
        return P[..., 0].amax(dim=1) - P[..., 0].amin(dim=1), P[..., 1].amax(dim=1) - P[..., 1].amin(dim=1)
    w, h = P.new_zeros(P.shape[0]), P.new_zeros(P.shape[0])
    best = torch.full_like(w, float("inf"))
    tie = TIE_EPSILONS * torch.finfo(P.dtype).eps
    for i, j in _PAIRS:
        others = [k for k in range(8) if k not in (i, j)]
        ex, ey = (P[:, j, 0] - P[:, i, 0])[:, None], (P[:, j, 1] - P[:, i, 1])[:, None]
        len2 = (ex * ex + ey * ey)[:, 0]
        rx, ry = P[:, others, 0] - P[:, i, 0:1], P[:, others, 1] - P[:, i, 1:2]
        zero = torch.zeros_like(ex)
        c = torch.cat([zero, _cross(ex, ey, rx, ry)], dim=1)                   # the line's own two points: 0
        d = torch.cat([zero, len2[:, None], ex * rx + ey * ry], dim=1)       # and 0, |e|^2 along it
        cmin, cmax = c.amin(dim=1), c.amax(dim=1)
        above, below = cmin >= 0, cmax <= 0
        length = torch.sqrt(torch.where(len2 > 0, len2, torch.ones_like(len2)))
        cw = (d.amax(dim=1) - d.amin(dim=1)) / length
        ch = torch.where(above, cmax, -cmin) / length
        take = (len2 > 0) & (above | below) & ((cw * ch).detach() < best * (1.0 - tie))
        best = torch.where(take, (cw * ch).detach(), best)
        w, h = torch.where(take, cw, w), torch.where(take, ch, h)
    return w, h


def _quad_area(Q):
    """``compute_area_4pts(..., 'cross-product')``: the triangles at vertices 0 and 2."""
    def at(k):
        u, v = Q[:, 1] - Q[:, k], Q[:, 3] - Q[:, k]
        return _cross(u[:, 0], u[:, 1], v[:, 0], v[:, 1]).abs()
    return 0.5 * (at(0) + at(2))


def _torch_outputs(form, kind, enc, a, b, ctr_a, ctr_b):
    if form == _oiou.BOXES:
        ox, oy = a[:, 0] - b[:, 0], a[:, 1] - b[:, 1]
        S, C = _corners(a, ox, oy), _corners(b, torch.zeros_like(ox), torch.zeros_like(oy))
        area1, area2 = a[:, 2] * a[:, 3], b[:, 2] * b[:, 3]
        d2 = ox * ox + oy * oy
    else:
        origin = 0.25 * ((b[:, 0] + b[:, 1]) + (b[:, 2] + b[:, 3]))
        S, C = a - origin[:, None], b - origin[:, None]
        area1, area2 = _quad_area(S), _quad_area(C)
        d2 = ((ctr_a - ctr_b) ** 2).sum(dim=-1)
    inter = _clip_area(S, C)
    u = area1 + area2 - inter
    iou = inter / u
    w, h = _enclosing(torch.cat([S, C], dim=1), enc)
    loss = 1.0 - iou + (d2 / (w * w + h * h) if kind == _oiou.DIOU else (w * h - u) / (w * h))
    return torch.stack([inter, area1, area2, u, iou, w, h, loss], dim=1)


# ------------------------------------------------------------------------------ the HIP route
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _describe(form, kind, enc, a, b, ctr_a, ctr_b):
    d = _oiou.OiouDesc()
    d.form, d.kind, d.enclosing, d.reserved, d.M = form, kind, enc, 0, a.shape[0]
    d.a, d.b, d.ctr_a, d.ctr_b = _ptr(a), _ptr(b), _ptr(ctr_a), _ptr(ctr_b)
    return d


class _Pairs(torch.autograd.Function):
    """One ``snvc_oiou_forward`` / ``snvc_oiou_backward`` pair: [M,8] from the operands of M pairs."""

    @staticmethod
    def forward(ctx, form, kind, enc, a, b, ctr_a, ctr_b):
        out = torch.empty((a.shape[0], _oiou.OUT), dtype=torch.float32, device=a.device)
        d = _describe(form, kind, enc, a, b, ctr_a, ctr_b)
        d.out = _ptr(out)
        with torch.cuda.device(a.device):
            _lib.check(_oiou.lib().snvc_oiou_forward(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)),
                       "snvc_oiou_forward")
        ctx.save_for_backward(a, b, ctr_a, ctr_b)
        ctx.args = (form, kind, enc)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        a, b, ctr_a, ctr_b = ctx.saved_tensors
        form, kind, enc = ctx.args
        gout = gout.to(torch.float32).contiguous()
        if gout.data_ptr() % 16:                 # a view into a larger buffer: the kernel reads gout in 16-byte pieces
            gout = gout.clone()
        ga, gb = torch.empty_like(a), torch.empty_like(b)
        gca = torch.empty_like(ctr_a) if ctr_a is not None else None
        gcb = torch.empty_like(ctr_b) if ctr_b is not None else None
        d = _describe(form, kind, enc, a, b, ctr_a, ctr_b)
        d.gout, d.ga, d.gb, d.gctr_a, d.gctr_b = _ptr(gout), _ptr(ga), _ptr(gb), _ptr(gca), _ptr(gcb)
        with torch.cuda.device(a.device):
            _lib.check(_oiou.lib().snvc_oiou_backward(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream(a.device).cuda_stream)),
                       "snvc_oiou_backward")
        return None, None, None, ga, gb, gca, gcb


def _torch_only():
    from ..models import loss3d
    return getattr(loss3d._route, "torch_only", False)


def pair_outputs(form, kind, enc, a, b, ctr_a=None, ctr_b=None):
    """[M,8] ``inter, area1, area2, u, iou, enc_w, enc_h, loss`` of M pairs.  ``form`` BOXES: ``a``, ``b`` [M,5]; QUADS: ``a``,
    ``b`` [M,4,2] and the centres ``ctr_a``, ``ctr_b`` [M,2] (None: the origin for both).  The other operands follow ``a``'s
    device and dtype."""
    tail = (5,) if form == _oiou.BOXES else (4, 2)
    if a.dim() != 1 + len(tail) or tuple(a.shape[1:]) != tail or b.shape != a.shape:
        raise ValueError(f"expected two tensors of one shape (M, {', '.join(map(str, tail))}), got {tuple(a.shape)} and {tuple(b.shape)}")
    b = b.to(device=a.device, dtype=a.dtype)
    if form == _oiou.QUADS:
        ctr_a = a.new_zeros(a.shape[0], 2) if ctr_a is None else ctr_a.to(device=a.device, dtype=a.dtype)
        ctr_b = a.new_zeros(a.shape[0], 2) if ctr_b is None else ctr_b.to(device=a.device, dtype=a.dtype)
        if tuple(ctr_a.shape) != (a.shape[0], 2) or ctr_b.shape != ctr_a.shape:
            raise ValueError(f"expected centres of shape ({a.shape[0]}, 2), got {tuple(ctr_a.shape)} and {tuple(ctr_b.shape)}")
    else:
        ctr_a = ctr_b = None
    if a.is_cuda and a.dtype == torch.float32 and not _torch_only():
        dense = [t if t is None else t.contiguous() for t in (a, b, ctr_a, ctr_b)]
        return _Pairs.apply(form, kind, enc, *dense)
    return _torch_outputs(form, kind, enc, a, b, ctr_a, ctr_b)


# ------------------------------------------------------------------------------ public names
def _flat(t, tail):
    if t.dim() < len(tail) or tuple(t.shape[t.dim() - len(tail):]) != tail:
        raise ValueError(f"expected a tensor of shape (..., {', '.join(map(str, tail))}), got {tuple(t.shape)}")
    return t.reshape((-1,) + tail), tuple(t.shape[:t.dim() - len(tail)])


def oriented_box_intersection_2d(corners1, corners2):
    """Intersection area of the quadrilaterals ``corners1`` (subject) and ``corners2`` (clip), both (B,N,4,2): ``(area (B,N),
    None)``.  (The second value of the module this stands in for, the clipped vertices, has no user.)"""
    a, lead = _flat(corners1, (4, 2))
    b, _ = _flat(corners2, (4, 2))
    # the whole QUADS evaluation with both centres at the origin: the other seven outputs, and in a backward the centres' (zero)
    # gradients, are computed and dropped -- a call is bound by its launch, not by the pair's arithmetic
    out = pair_outputs(_oiou.QUADS, _oiou.DIOU, _oiou.ALIGNED, a, b)
    return out[:, _oiou.INTER].reshape(lead), None


def enclosing_box(corners1, corners2, enclosing_type="smallest"):
    """``(w, h)``, each (B,N), of the rectangle enclosing the eight corners (the whole QUADS evaluation, as above)."""
    code = _enclosing_code(enclosing_type)
    a, lead = _flat(corners1, (4, 2))
    b, _ = _flat(corners2, (4, 2))
    out = pair_outputs(_oiou.QUADS, _oiou.DIOU, code, a, b)
    return out[:, _oiou.ENC_W].reshape(lead), out[:, _oiou.ENC_H].reshape(lead)


def _boxes(box1, box2, kind, enclosing_type):
    a, lead = _flat(box1, (5,))
    b, _ = _flat(box2, (5,))
    return pair_outputs(_oiou.BOXES, kind, _enclosing_code(enclosing_type), a, b), lead


def cal_iou(box1, box2):
    """``(iou (B,N), corners1 (B,N,4,2), corners2 (B,N,4,2), u (B,N))`` of the boxes (B,N,5); box 1 is the subject."""
    out, lead = _boxes(box1, box2, _oiou.DIOU, "aligned")
    return out[:, _oiou.IOU].reshape(lead), box2corners_th(box1), box2corners_th(box2.to(device=box1.device, dtype=box1.dtype)), \
        out[:, _oiou.UNION].reshape(lead)


def cal_diou(box1, box2, enclosing_type="smallest", return_overlap=False):
    """``(diou_loss (B,N), iou (B,N))`` of the boxes (B,N,5), plus the intersection area with ``return_overlap``."""
    out, lead = _boxes(box1, box2, _oiou.DIOU, enclosing_type)
    result = out[:, _oiou.LOSS].reshape(lead), out[:, _oiou.IOU].reshape(lead)
    return result + (out[:, _oiou.INTER].reshape(lead),) if return_overlap else result


def cal_giou(box1, box2, enclosing_type="smallest"):
    """``(giou_loss (B,N), iou (B,N))`` of the boxes (B,N,5)."""
    out, lead = _boxes(box1, box2, _oiou.GIOU, enclosing_type)
    return out[:, _oiou.LOSS].reshape(lead), out[:, _oiou.IOU].reshape(lead)
