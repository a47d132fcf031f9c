"""Central-difference Jacobian of the reference's ``numerical_jaccobian`` module (numerical_jaccobian.py:17-57), on
host torch and without the removed ``torch._six``.  ``BoxesIou3dDifferentiableFunction.backward`` does not call it:
the HIP kernel ``snvc_iou3d_backward`` evaluates the same differences, one lane per pair.  It stays for callers of the
reference's module and as the definition the kernel reproduces."""
from collections import abc

import torch


def iter_tensors(x, only_requiring_grad=False):
    if isinstance(x, torch.Tensor):
        if x.requires_grad or not only_requiring_grad:
            yield x
    elif isinstance(x, abc.Iterable) and not isinstance(x, str):
        for elem in x:
            yield from iter_tensors(elem, only_requiring_grad)


def get_numerical_jacobian(fn, input, target=None, eps=1e-3):
    """Column k of the result is ``(fn(input) at target[:, k] + eps  -  fn(input) at target[:, k] - eps) / (2 eps)``,
    with ``target`` (default: ``input``) a 2-D tensor that ``fn`` reads through ``input`` and is modified in place
    (through ``.data``) for each evaluation, then restored.  Row i of ``fn``'s output must depend on row i of
    ``target`` only, as for the one-by-one IoU."""
    if target is None:
        target = input
    if not isinstance(target, torch.Tensor) or target.dim() != 2:
        raise TypeError("target must be a 2-D tensor")
    if target.dtype.is_complex or target.is_sparse:
        raise TypeError("target must be a dense real tensor")
    jacobian = torch.zeros_like(target)
    x = target.data
    for k in range(x.size(1)):
        orig = x[:, k].clone()
        x[:, k] = orig - eps
        outa = fn(input).clone()
        x[:, k] = orig + eps
        outb = fn(input).clone()
        x[:, k] = orig
        jacobian[:, k] = ((outb - outa) / (2 * eps)).detach()
    return jacobian
