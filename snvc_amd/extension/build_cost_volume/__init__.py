"""Drop-in for ``snvc.extension.build_cost_volume`` (reference __init__.py:1-26).

``build_cost_volume(left, right, shift, downsample)`` -> ``[N, 2C, D, H/ds, W/ds]``; the left
half of the channel axis repeats the left feature for every plane, the right half holds the
right feature shifted by ``shift[n, d]`` pixels with linear interpolation (a CONCAT volume, no
correlation: BuildCostVolume_cuda.cu:81-96).  Backward returns ``(gL, gR, None, None)``.
"""
import types

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import ops
from ..._derived import stamp

# Stands where the reference's pybind module sits (BuildCostVolume.cpp:44-48): same two names.
build_cost_volume_cuda = types.SimpleNamespace(
    build_cost_volume_forward=ops.cost_volume_forward,
    build_cost_volume_backward=ops.cost_volume_backward,
)


class _BuildCostVolume(Function):
    @staticmethod
    def forward(ctx, left, right, shift, downsample):
        ctx.save_for_backward(shift)
        ctx.downsample = downsample
        # reference __init__.py:12 (forces a device->host sync there too)
        assert torch.all(shift >= 0.)
        return build_cost_volume_cuda.build_cost_volume_forward(left, right, shift, downsample)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        shift, = ctx.saved_tensors
        grad_left, grad_right = build_cost_volume_cuda.build_cost_volume_backward(
            grad_output, shift, ctx.downsample)
        return grad_left, grad_right, None, None


def build_cost_volume(left, right, shift, downsample):
    """Reference signature (__init__.py:26).  With autograd on, or for anything but the fp32 / downsample 1, 2 or 4 case of the
    global model, this is the eager autograd function.  Under ``torch.no_grad()`` the result is a ``LazyCostVolume``
    (snvc_amd/lazy.py): a tensor of the volume's shape that ``GlobalStack.forward`` consumes without building it and that
    turns into the real volume -- the same values -- on any other use."""
    lazy_ok = (not torch.is_grad_enabled() and downsample in (1, 2, 4) and left.is_cuda and left.dtype == torch.float32 and
               left.dim() == 4 and left.shape == right.shape and shift.dim() == 2 and shift.shape[0] == left.shape[0] and
               not (left.requires_grad or right.requires_grad) and
               (left.shape[2] % downsample == 0 and left.shape[3] % downsample == 0))      # r6: downsample 2 and 4 have fused routes too
    if not lazy_ok:
        return _BuildCostVolume.apply(left, right, shift, downsample)
    from ...lazy import CONSUMER, LazyCostVolume
    from ... import ops
    spacing = "unknown"
    ref = CONSUMER.ref
    model = ref() if (ref is not None and downsample == 1) else None
    if model is not None:
        # r5: the model that consumed the previous lazy volume runs this call's step up to its one host sync -- the same check of
        # `shift` as below (an AssertionError comes out of here, reference __init__.py:12) -- with its first-layer prep queued in
        # front of the wait; model(volume) resumes it.  Without this the GPU idles through the wait and the host's way from here to
        # the model's first launch (reference_api 0.076 ms/step behind forward_pair at cfg2).
        # r6: this function is a pure function in the reference (__init__.py:7-26), so (a) nothing but the reference's own
        # AssertionError may come out of the speculative step -- any other failure drops it and the plain path below runs; (b) the
        # paused step is stamped with the model's prep epoch and starts over if any other call used the model's prep buffers before
        # model(volume) resumes it (two pending volumes, a forward_pair in between: tests/test_gpu_lazy_alias.py).
        gen = None
        try:
            gen = model.lazy_prefetch(left, right, shift)
        except AssertionError:
            raise
        except Exception:        # Unsupported shape, misaligned view, workspace OOM, ...: not this function's errors
            gen = None
        if gen is not None:
            seen = model.conv1[0][0].__dict__["_snvc_factored"].get("spacing_seen")      # (q, m0, D, W) of THIS shift array, or ("general", D, W)
            stream = torch.cuda.current_stream(left.device).cuda_stream
            return LazyCostVolume(left, right, shift, downsample, build_cost_volume_cuda.build_cost_volume_forward,
                                  tuple(seen[:2]) if (seen is not None and seen[0] != "general") else None,
                                  prefetch=(ref, gen, stamp((model.conv1[0][0].weight,), (stream,))))
    if shift.dtype == torch.float32 and shift.numel() > 0:
        # reference __init__.py:12, at the same point of the call sequence and with the same single sync; the launch also
        # classifies the array's spacing, which GlobalStack.forward_pair would otherwise sync for a second time
        nonneg, spacing = ops.shift_spacing_result(ops.shift_structure_begin(shift.detach()), shift.size(1))
        assert nonneg
    else:
        assert torch.all(shift >= 0.)
    return LazyCostVolume(left, right, shift, downsample, build_cost_volume_cuda.build_cost_volume_forward, spacing)
