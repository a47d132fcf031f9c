"""ctypes binding of the loss entry points of ``libsnvc_hip.so`` (``include/snvc_loss.h``), and the autograd functions built
on them (the public classes are in ``snvc_amd.models.loss3d``).

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_loss_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.

Nothing here waits for the device: mask counts and normalisers stay in a small float64 workspace that the backward kernel
reads, the upstream gradient scalar is read on the device, and the two input checks that need a count (a heat map without a
positive target, a focal target outside {0, 1}) are bits of a device flag whose pinned host copy is looked at by the next
call, or by ``check_flags()``.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_loss_abi_version() this binding was written against

# enum snvc_loss_kind
MSE_ROWS, MSE_POSNEG, OCCUPANCY, OFFSET, SMOOTH_L1_MASKED, SIGMOID_FOCAL, SMOOTH_L1_ROWS = range(7)
EMPTY_IS_NAN, TARGET_INT32, TARGET_INT64, TARGET_UINT8 = 1, 2, 4, 8       # enum snvc_loss_flags
TARGET_FLAGS = {torch.int32: TARGET_INT32, torch.int64: TARGET_INT64, torch.uint8: TARGET_UINT8}
FLAG_NO_POSITIVE, FLAG_BAD_TARGET = 1, 2          # SNVC_LOSS_FLAG_*
MAX_ROWS = 65535                                  # SNVC_LOSS_MAX_ROWS

FLAG_TEXT = {
    FLAG_NO_POSITIVE: "VoxelMSELossWeighted: a part's target heat map has no positive element",
    FLAG_BAD_TARGET: "labels should be 0 or 1 in multitargetloss.",
}


class LossDesc(ctypes.Structure):
    """Mirror of ``snvc_loss_desc`` (include/snvc_loss.h)."""
    _fields_ = [("kind", ctypes.c_int32), ("flags", ctypes.c_int32), ("rows", c_i64), ("cols", c_i64), ("group", c_i64),
                ("p0", ctypes.c_float), ("p1", ctypes.c_float)] + [
        (n, c_p) for n in ("a", "b", "c", "roww", "partials", "fin", "loss", "flag", "gout", "ga")]


_desc_p = ctypes.POINTER(LossDesc)

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_loss_abi_version": (c_int, []),
    "snvc_loss_partials_count": (c_i64, [_desc_p]),
    "snvc_loss_forward": (c_int, [_desc_p, c_p]),
    "snvc_loss_backward": (c_int, [_desc_p, c_p]),
    "snvc_loss_wdist_partials_count": (c_i64, [c_i64, c_i64, c_i64, c_int]),
    "snvc_loss_wdist_forward": (c_int, [c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p]),
    "snvc_loss_wdist_backward": (c_int, [c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, c_p]),
    "snvc_loss_depth_regression_partials_count": (c_i64, [c_i64, c_i64]),
    "snvc_loss_depth_regression_forward": (c_int, [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_p]),
    "snvc_loss_depth_regression_backward": (c_int, [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p, c_p, c_p, c_p]),
    "snvc_loss_disparity_regression_backward": (c_int, [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_loss_abi_version", _ABI, "loss")


# ------------------------------------------------------------------------------ the deferred input checks
class LossInputError(RuntimeError):
    """An input check of a loss failed: raised at once on the torch route, by the next call or ``check_flags()`` on the HIP
    route (the reference asserts at this point, with a host synchronisation)."""


class _Flag:
    """The int32 the loss kernels OR their SNVC_LOSS_FLAG_* bits into, its pinned host copy and the event behind the copy
    (the scheme of ``submodule.OverflowGuard`` with ``overflow_check = "deferred"``)."""

    def __init__(self, device):
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None

    def post(self):
        self.host.copy_(self.flag, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def look(self, wait: bool):
        """Raise what an earlier call posted.  ``wait=False`` looks only if the copy has already landed (no waiting)."""
        ev = self.event
        if ev is None:
            return
        if wait:
            ev.synchronize()
        elif not ev.query():
            return
        self.event = None
        bits = int(self.host[0])
        if bits:
            self.host.zero_()
            self.flag.zero_()
            raise LossInputError("; ".join(text for bit, text in FLAG_TEXT.items() if bits & bit))


_flags = {}


def flag_of(device) -> _Flag:
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    f = _flags.get(device)
    if f is None:
        with torch.cuda.device(device):
            f = _flags[device] = _Flag(device)
    return f


def check_flags():
    """Wait for every posted flag and raise ``LossInputError`` if a check failed since the last look."""
    for f in list(_flags.values()):
        f.look(wait=True)


# ------------------------------------------------------------------------------ helpers
def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() > 0 else ctypes.c_void_p(0)


def _stream(t):
    return c_p(torch.cuda.current_stream(t.device).cuda_stream)


def _f32_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor: Not implemented on the CPU")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _same_device(ref, *others):
    for o in others:
        if o is not None and o.device != ref.device:
            raise RuntimeError(f"loss operands on different devices: {ref.device} and {o.device}")


# ------------------------------------------------------------------------------ elementwise kinds
class _Elementwise(torch.autograd.Function):
    """One ``snvc_loss_forward`` / ``snvc_loss_backward`` pair.  ``a`` is the only differentiable operand."""

    @staticmethod
    def forward(ctx, a, kind, b, c, roww, rows, cols, group, p0, p1, flags, post_flag):
        dev = a.device
        d = LossDesc()
        d.kind, d.flags, d.rows, d.cols, d.group, d.p0, d.p1 = kind, flags, rows, cols, group, p0, p1
        d.a, d.b, d.c, d.roww = _ptr(a), _ptr(b), _ptr(c), _ptr(roww)
        with torch.cuda.device(dev):
            L = lib()
            count = L.snvc_loss_partials_count(ctypes.byref(d))
            if count < 0:
                _lib.check(1, "snvc_loss_partials_count")
            partials = torch.empty(count, dtype=torch.float32, device=dev)
            fin = torch.empty(2 * group if kind == MSE_POSNEG else 2, dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            fl = flag_of(dev)
            d.partials, d.fin, d.loss, d.flag = _ptr(partials), _ptr(fin), _ptr(loss), _ptr(fl.flag)
            _lib.check(L.snvc_loss_forward(ctypes.byref(d), _stream(a)), "snvc_loss_forward")
            if post_flag:
                fl.post()
        ctx.save_for_backward(a, b, c, roww, fin)
        ctx.args = (kind, rows, cols, group, p0, p1, flags)
        return loss

    @staticmethod
    def backward(ctx, gout):
        a, b, c, roww, fin = ctx.saved_tensors
        kind, rows, cols, group, p0, p1, flags = ctx.args
        gout = gout.to(torch.float32).contiguous()
        ga = torch.empty_like(a)
        d = LossDesc()
        d.kind, d.flags, d.rows, d.cols, d.group, d.p0, d.p1 = kind, flags, rows, cols, group, p0, p1
        d.a, d.b, d.c, d.roww = _ptr(a), _ptr(b), _ptr(c), _ptr(roww)
        d.fin, d.gout, d.ga = _ptr(fin), _ptr(gout), _ptr(ga)
        with torch.cuda.device(a.device):
            _lib.check(lib().snvc_loss_backward(ctypes.byref(d), _stream(a)), "snvc_loss_backward")
        return (ga,) + (None,) * 11


def elementwise(kind, a, b, c=None, roww=None, *, rows=1, group=1, p0=0.0, p1=0.0, flags=0, post_flag=False):
    """The loss of ``kind`` (include/snvc_loss.h) over ``a`` viewed as [rows][a.numel() / rows]: a 0-d float32 tensor,
    differentiable with respect to ``a``.  Every operand is a contiguous GPU tensor; ``b`` and ``c`` are float32 of the kind's
    shape (``b`` int32 / int64 / uint8 with the TARGET_* flag of its dtype, ``c`` uint8 for SMOOTH_L1_MASKED)."""
    _f32_gpu(a, "prediction")
    rows, group = int(rows), int(group)
    if rows < 1 or group < 1 or a.numel() % rows:
        raise RuntimeError(f"loss: {a.numel()} elements do not split into {rows} rows")
    if rows > MAX_ROWS:
        raise RuntimeError(f"loss: {rows} rows is above the kernel's limit of {MAX_ROWS}")
    want_b = next((dt for dt, bit in TARGET_FLAGS.items() if flags & bit), torch.float32)
    if b.dtype != want_b or b.numel() != a.numel() or not b.is_contiguous():
        raise RuntimeError(f"loss: the target must be a contiguous {want_b} tensor with the prediction's {a.numel()} elements")
    if c is not None:
        want_c = torch.uint8 if kind == SMOOTH_L1_MASKED else torch.float32
        want_n = a.numel() // group if kind == OFFSET else a.numel()
        if c.dtype != want_c or c.numel() != want_n or not c.is_contiguous():
            raise RuntimeError(f"loss: the third operand must be a contiguous {want_c} tensor of {want_n} elements")
    if roww is not None:
        want_n = rows if kind == MSE_ROWS else a.numel() // group
        if roww.dtype != torch.float32 or roww.numel() != want_n or not roww.is_contiguous():
            raise RuntimeError(f"loss: the row weights must be a contiguous float32 tensor of {want_n} elements")
    _same_device(a, b, c, roww)
    return _Elementwise.apply(a, kind, b, c, roww, rows, a.numel() // rows, group, float(p0), float(p1), int(flags), post_flag)


# ------------------------------------------------------------------------------ W_loss
class _WDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, prob, off, target, mask, levels, per_pixel):
        b, d, h, w = prob.shape
        dev = prob.device
        with torch.cuda.device(dev):
            L = lib()
            count = L.snvc_loss_wdist_partials_count(b, d, h * w, int(per_pixel))
            partials = torch.empty(count, dtype=torch.float32, device=dev)
            fin = torch.empty(2, dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            pix = torch.empty((b, h, w), dtype=torch.float32, device=dev) if per_pixel else None
            _lib.check(L.snvc_loss_wdist_forward(_ptr(prob), _ptr(off), _ptr(target), _ptr(mask), _ptr(levels), b, d, h * w, _ptr(pix),
                                                 _ptr(partials), _ptr(fin), _ptr(loss), _stream(prob)), "snvc_loss_wdist_forward")
        ctx.save_for_backward(prob, off, target, mask, levels, fin)
        ctx.per_pixel = per_pixel
        return pix if per_pixel else loss

    @staticmethod
    def backward(ctx, gout):
        prob, off, target, mask, levels, fin = ctx.saved_tensors
        b, d, h, w = prob.shape
        gout = gout.to(torch.float32).contiguous()
        gprob = torch.empty_like(prob) if ctx.needs_input_grad[0] else None
        goff = torch.empty_like(off) if ctx.needs_input_grad[1] else None
        scalar, gpix = (None, gout) if ctx.per_pixel else (gout, None)
        with torch.cuda.device(prob.device):
            _lib.check(lib().snvc_loss_wdist_backward(_ptr(prob), _ptr(off), _ptr(target), _ptr(mask), _ptr(levels), b, d, h * w, _ptr(fin),
                                                      _ptr(scalar), _ptr(gpix), _ptr(gprob),
                                                      _ptr(goff), _stream(prob)), "snvc_loss_wdist_backward")
        return gprob, goff, None, None, None, None


def wdist(prob, off, target, mask, levels, per_pixel=False):
    """sum_d prob |levels[d] + off - target| per masked pixel of [B,D,H,W] ``prob`` / ``off``: their mean (0-d), or with
    ``per_pixel`` the [B,H,W] map of the sums (0 outside the mask).  ``mask`` is a uint8 [B,H,W] tensor."""
    _f32_gpu(prob, "prob"); _f32_gpu(off, "off"); _f32_gpu(target, "target"); _f32_gpu(levels, "depth_levels")
    if prob.dim() != 4 or off.shape != prob.shape:
        raise RuntimeError(f"W_loss: prob and off must share one [B,D,H,W] shape, got {tuple(prob.shape)} and {tuple(off.shape)}")
    b, d, h, w = prob.shape
    if tuple(target.shape) != (b, h, w) or tuple(mask.shape) != (b, h, w) or levels.numel() != d:
        raise RuntimeError("W_loss: target and mask must be [B,H,W] and depth_levels [D]")
    if mask.dtype != torch.uint8 or not mask.is_cuda or not mask.is_contiguous():
        raise RuntimeError("W_loss: mask must be a contiguous uint8 GPU tensor")
    _same_device(prob, off, target, mask, levels)
    return _WDist.apply(prob, off, target, mask, levels, bool(per_pixel))


# ------------------------------------------------------------------------------ depth head
class _DepthRegressionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, levels, gt):
        b, d, h, w = cost.shape
        dev = cost.device
        with torch.cuda.device(dev):
            L = lib()
            partials = torch.empty(L.snvc_loss_depth_regression_partials_count(b, h * w), dtype=torch.float32, device=dev)
            fin = torch.empty(2, dtype=torch.float64, device=dev)
            loss = torch.empty((), dtype=torch.float32, device=dev)
            _lib.check(L.snvc_loss_depth_regression_forward(_ptr(cost), _ptr(levels), _ptr(gt), b, d, h * w, _ptr(partials), _ptr(fin),
                                                            _ptr(loss), _stream(cost)), "snvc_loss_depth_regression_forward")
        ctx.save_for_backward(cost, levels, gt, fin)
        return loss

    @staticmethod
    def backward(ctx, gout):
        cost, levels, gt, fin = ctx.saved_tensors
        b, d, h, w = cost.shape
        gout = gout.to(torch.float32).contiguous()
        gcost = torch.empty_like(cost)
        with torch.cuda.device(cost.device):
            _lib.check(lib().snvc_loss_depth_regression_backward(_ptr(cost), _ptr(levels), _ptr(gt), b, d, h * w, _ptr(fin),
                                                                 _ptr(gout), _ptr(gcost), _stream(cost)),
                       "snvc_loss_depth_regression_backward")
        return gcost, None, None


def depth_regression_loss(cost, levels, gt):
    _f32_gpu(cost, "cost"); _f32_gpu(levels, "depth_levels"); _f32_gpu(gt, "gt_depth")
    if cost.dim() != 4 or cost.size(1) < 1:
        raise RuntimeError(f"depth_regression_loss: cost must be [B,D,H,W] with D >= 1, got {tuple(cost.shape)}")
    b, d, h, w = cost.shape
    if levels.numel() != d or tuple(gt.shape) != (b, h, w):
        raise RuntimeError("depth_regression_loss: depth_levels must be [D] and gt_depth [B,H,W]")
    _same_device(cost, levels, gt)
    return _DepthRegressionLoss.apply(cost, levels, gt)


def disparity_regression_backward(gy, depth, d):
    """Gradient of ``ops.disparity_regression`` with respect to ``x``: [N,H,W] x [D] -> [N,D,H,W]."""
    _f32_gpu(gy, "gy"); _f32_gpu(depth, "depth")
    n, h, w = gy.shape
    gx = torch.empty((n, d, h, w), dtype=torch.float32, device=gy.device)
    with torch.cuda.device(gy.device):
        _lib.check(lib().snvc_loss_disparity_regression_backward(_ptr(gy), _ptr(depth), _ptr(gx), n, d, h * w, _stream(gy)),
                   "snvc_loss_disparity_regression_backward")
    return gx
