"""ctypes binding of the HRNet fusion entry points of ``libsnvc_hip.so`` (``include/snvc_hrnet.h``), and the two tensor-level
calls built on them.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_hrnet_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this
module loads nothing.
"""
import ctypes

import torch

from . import _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_hrnet_abi_version() this binding was written against

MAX_TERMS = 4                  # SNVC_HRNET_MAX_TERMS
FACTORS = (1, 2, 4, 8)

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_hrnet_abi_version": (c_int, []),
    "snvc_hrnet_fuse_forward": (c_int, [c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i64, c_int, c_p]),
    "snvc_hrnet_fuse_backward": (c_int, [c_p, c_p, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i64, c_int, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_hrnet_abi_version", _ABI, "hrnet")


def host_arrays(ptrs, factors, extents):
    """The three host arrays of snvc_hrnet_fuse_forward: term pointers (0 = NULL), factors, (h, w) per term."""
    n = MAX_TERMS
    t = (c_p * n)(*(list(ptrs) + [None] * (n - len(ptrs))))
    f = (ctypes.c_int32 * n)(*(list(factors) + [1] * (n - len(factors))))
    e = (c_i64 * (2 * n))(*(list(extents) + [0] * (2 * n - len(extents))))
    return t, f, e


def _check_gpu(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor: Not implemented on the CPU")
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 4:
        raise RuntimeError(f"{name} must be a contiguous float32 NCHW tensor")


def fuse_forward(terms, factors, relu=True, out=None):
    """act(terms[0] + up(terms[1], factors[1]) + ...), left to right, None terms skipped; ``out`` may be terms[0] (in place,
    factor 1).  The output extent is terms[0]'s times factors[0]."""
    from .ops import _ptr, _stream
    t0, f0 = terms[0], factors[0]
    if t0 is None:
        raise RuntimeError("hrnet fusion: term 0 must not be None")
    for k, t in enumerate(terms):
        if t is not None:
            _check_gpu(t, f"term {k}")
    n, c, h, w = t0.shape[0], t0.shape[1], t0.shape[2] * f0, t0.shape[3] * f0
    for k, t in enumerate(terms):
        if t is not None and (t.shape[0], t.shape[1]) != (n, c):
            raise RuntimeError(f"hrnet fusion: term {k} has shape {tuple(t.shape)}, term 0 {tuple(t0.shape)}")
    if out is None:
        out = torch.empty((n, c, h, w), dtype=torch.float32, device=t0.device)
    else:
        _check_gpu(out, "out")
        if tuple(out.shape) != (n, c, h, w):
            raise RuntimeError(f"hrnet fusion: out has shape {tuple(out.shape)}, expected {(n, c, h, w)}")
    ptrs = [_ptr(t).value for t in terms]            # None: a skipped term
    ext = [v for t in terms for v in ((t.shape[2], t.shape[3]) if t is not None else (0, 0))]
    ta, fa, ea = host_arrays(ptrs, factors, ext)
    with torch.cuda.device(t0.device):
        _lib.check(lib().snvc_hrnet_fuse_forward(ta, fa, ea, _ptr(out), n, c, h, w, int(bool(relu)), _stream(t0)),
                   "snvc_hrnet_fuse_forward")
    return out


def fuse_backward(gy, out, factors, relu=True):
    """Gradients of ``fuse_forward`` w.r.t. its terms: {factor: tensor} for every factor in ``factors`` (factor 1: the masked
    gradient at full resolution, shared by every factor-1 term; f > 1: its f x f block sums)."""
    from .ops import _ptr, _stream
    _check_gpu(gy, "gy")
    if relu:
        _check_gpu(out, "out")
        if out.shape != gy.shape:
            raise RuntimeError("hrnet fusion backward: gy and out differ in shape")
    n, c, h, w = gy.shape
    grads = {}
    for f in sorted(set(factors)):
        if f not in FACTORS:
            raise RuntimeError(f"hrnet fusion backward: factor {f} is not 1, 2, 4 or 8")
        grads[f] = torch.empty((n, c, h // f, w // f), dtype=torch.float32, device=gy.device)
    p = [_ptr(grads[f]) if f in grads else None for f in FACTORS]
    with torch.cuda.device(gy.device):
        _lib.check(lib().snvc_hrnet_fuse_backward(_ptr(gy), _ptr(out) if relu else None, p[0], p[1], p[2], p[3], n, c, h, w,
                                                  int(bool(relu)), _stream(gy)), "snvc_hrnet_fuse_backward")
    return grads
