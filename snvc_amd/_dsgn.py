"""ctypes binding of the DSGN SPP entry points of ``libsnvc_hip.so`` (``include/snvc_dsgn.h``), and the two tensor-level calls
built on them.

Kept apart from ``_lib.SIGNATURES`` (the table of ``include/snvc_hip.h``): this header versions itself through
``snvc_dsgn_abi_version()``.  The symbols are resolved on ``_lib.lib()``'s handle at first use, so importing this module
loads nothing.
"""
import torch

from . import _lib
from ._lib import c_i64, c_int, c_p

_ABI = 1   # snvc_dsgn_abi_version() this binding was written against

WINDOWS = (8, 16, 32, 64)       # out8, out16, out32, out64 of snvc_dsgn_spp_pool
MAX_CELLS = 8192                # SNVC_DSGN_MAX_CELLS

# name -> (restype, argtypes); kept next to the header so the symbol test can walk it
SIGNATURES = {
    "snvc_dsgn_abi_version": (c_int, []),
    "snvc_dsgn_spp_pool": (c_int, [c_p, c_i64, c_p, c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i64, c_p]),
    "snvc_dsgn_spp_upsample": (c_int, [c_p, c_p, c_p, c_i64, c_i64, c_i64, c_i64, c_i64, c_int, c_p]),
}

lib = _lib.binder(SIGNATURES, "snvc_dsgn_abi_version", _ABI, "dsgn")


def _check_gpu(t, name, dense=True):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor: Not implemented on the CPU")
    if t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{name} must be a float32 NCHW tensor")
    c, h, w = t.shape[1:]
    if dense and not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    if not dense and t.size(0) > 0 and tuple(t.stride()[1:]) != (h * w, w, 1):
        raise RuntimeError(f"{name} must have dense (C, H, W) planes (a channel slice of an NCHW buffer at most)")


def _batch_stride(t):
    return t.stride(0) if t.size(0) > 1 else 0


def spp_pool(x):
    """The four SPP average pools of ``x`` [N,C,H,W] (a channel slice allowed) in one launch: [pool8, pool16, pool32, pool64],
    each ``F.avg_pool2d(x, k, k)``."""
    from .ops import _ptr, _stream
    _check_gpu(x, "x", dense=False)
    n, c, h, w = x.shape
    if h < 64 or w < 64:
        raise RuntimeError(f"SPP pooling needs H, W >= 64 (the 64 x 64 window), got {h} x {w}")
    outs = [torch.empty((n, c, h // k, w // k), dtype=torch.float32, device=x.device) for k in WINDOWS]
    with torch.cuda.device(x.device):
        _lib.check(lib().snvc_dsgn_spp_pool(_ptr(x), _batch_stride(x), *[_ptr(o) for o in outs], n, c, h, w, _stream(x)),
                   "snvc_dsgn_spp_pool")
    return outs


def spp_upsample(maps, out, align_corners):
    """``out[:, k*C:(k+1)*C] = F.interpolate(maps[k], out's (H, W), mode='bilinear', align_corners=align_corners)`` for the four
    [N,C,h_k,w_k] ``maps``, in one launch; ``out`` [N,4C,H,W] may be a channel slice of a wider buffer."""
    from .ops import _ptr, _stream
    if len(maps) != 4:
        raise RuntimeError("spp_upsample takes four maps")
    _check_gpu(out, "out", dense=False)
    n, c4, h, w = out.shape
    for k, m in enumerate(maps):
        _check_gpu(m, f"map {k}")
        if (m.size(0), 4 * m.size(1)) != (n, c4):
            raise RuntimeError(f"spp_upsample: map {k} has shape {tuple(m.shape)}, out {tuple(out.shape)}")
    ptrs = (c_p * 4)(*[_ptr(m).value for m in maps])
    ext = (c_i64 * 8)(*[v for m in maps for v in m.shape[2:]])
    with torch.cuda.device(out.device):
        _lib.check(lib().snvc_dsgn_spp_upsample(ptrs, ext, _ptr(out), _batch_stride(out), n, c4 // 4, h, w, int(bool(align_corners)),
                                                _stream(out)), "snvc_dsgn_spp_upsample")
    return out
