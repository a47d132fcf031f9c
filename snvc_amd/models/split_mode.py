"""Split mode ("f16x3", r4): inference with frozen statistics on the snvc_f16x3_* kernels -- the fp32 layers at fp32 accuracy on
the half-precision matrix pipe (csrc/conv3d_f16.hip, F16Cfg::PL).  A tensor travels as SplitT: the (hi, lo) pair,
the power of two its values are stored times (an int exponent, or a one-element device tensor when the range is only known
from the data), and the bound |value| is promised to stay below (None for data-scaled tensors: they cannot overflow).

This module holds what every split-mode model shares: the tensor tag, the exponent rule, the overflow flag and the POLICY for a
flag that came back set (``SplitModePolicy``).  ``submodule`` re-exports all of it; the layers themselves
(``fused_conv3d_x3``) live there."""
import math
import warnings

import torch
import torch.nn as nn

from .. import ops
from .._derived import derived

X3_SIGMAS = 64.0     # a BatchNorm output is promised to stay below |beta| + X3_SIGMAS * |gamma|
X3_GROUP_NORM = [True]      # False: GroupNorm models stay on the fp32-MFMA kernels (r4's behaviour; kept for measuring)


class SplitT:
    __slots__ = ("t", "exp", "mul_dev", "bound")

    def __init__(self, t, exp=0, bound=None, mul_dev=None):
        self.t, self.exp, self.bound, self.mul_dev = t, exp, bound, mul_dev

    def slice_groups(self, lo: int, hi: int):
        """Channel groups [lo, hi) of the pair (a view: split tensors are [N, 2, C/8, D, H, W, 8])."""
        return SplitT(self.t[:, :, lo:hi], self.exp, self.bound, self.mul_dev)


class SplitOverflow(RuntimeError):
    """Raised INSIDE a split-mode call whose overflow flag came back set: the call's result (an activation clamped to half's
    range) is dropped and the model's public entry point redoes the call on the fp32-MFMA kernels.  Never reaches the caller
    unless split mode was demanded (arithmetic / precision = "x3")."""


class OverflowGuard:
    """The overflow flag of a model's split-mode calls: an int32 on the device that every clamping epilogue ORs into, its pinned
    host copy and the event behind the copy.

    ``post()`` is queued right after the LAST layer that can clamp (the layers behind it write float32); ``wait()`` is called
    once the rest of the call has been queued: the host then waits for the flag while the GPU still has those last layers to
    run, so the check costs no GPU idle time and the result never leaves the call unchecked (r4 looked at the flag one call
    late).  ``check="deferred"`` models post without waiting; ``pending()`` is the synchronous look a caller can take then."""

    def __init__(self, device):
        self.flag = torch.zeros(1, dtype=torch.int32, device=device)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None

    def post(self):
        self.host.copy_(self.flag, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def wait(self) -> bool:
        """True if a value was clamped since the last look (the device flag is cleared again then)."""
        ev, self.event = self.event, None
        if ev is None:
            return False
        ops.spin_wait(ev)
        if int(self.host.item()) == 0:
            return False
        self.flag.zero_()
        return True

    pending = wait


def overflow_guard(module, device) -> OverflowGuard:
    """The module's guard for ``device`` (kept across rebuilds of the packed split-mode state: a pending flag is never dropped)."""
    guards = module.__dict__.setdefault("_snvc_x3_guard", {})
    g = guards.get(device)
    if g is None:
        g = guards[device] = OverflowGuard(device)
    return g


def x3_exponent(bound: float) -> int:
    """e with bound * 2^e <= 2^15 (half overflows at 65504; a value beyond the bound is clamped and FLAGGED)."""
    if not (bound > 0.0) or not math.isfinite(bound):
        return 0
    return max(-14, min(14, 15 - math.frexp(bound)[1]))


def x3_norm_bound(norm, plan) -> float:
    """|beta| + X3_SIGMAS * |gamma| of a frozen BatchNorm3d, maximised over channels (cached with the folded affine); of a
    GroupNorm likewise (its result is gamma * xhat + beta with xhat normalised per sample and group)."""
    w, b = norm.weight, norm.bias

    def build():
        g = w.detach().abs() if w is not None else torch.ones(1)
        bb = b.detach().abs().to(g.device) if b is not None else torch.zeros(1, device=g.device)
        return float((bb + X3_SIGMAS * g).max().item())
    return derived(plan, "x3_bound", (w, b), build)


def x3_ok(*modules, group_norm: bool = True) -> bool:
    """Every norm a frozen BatchNorm3d (eval mode, running statistics) or -- r5, ``group_norm`` -- a GroupNorm (its statistics are
    taken from the layer's fp32 result, see fused_conv3d_x3); nothing to differentiate."""
    if torch.is_grad_enabled():
        return False
    for m in modules:
        for n in m.modules():
            if isinstance(n, nn.GroupNorm) and not (group_norm and X3_GROUP_NORM[0]):
                return False
            if isinstance(n, nn.modules.batchnorm._BatchNorm) and (n.training or n.running_mean is None):
                return False
    return True


class SplitModePolicy:
    """What a model (``GlobalStack``, ``VernierScale``) does when split mode overflows.  A split tensor's exponent is chosen from its
    norm's parameters; a value beyond that range is clamped by the epilogue and FLAGGED.  ``overflow_check`` = "call" (default,
    r5): the flag is read before the result leaves the call -- the copy is queued behind the last layer that can clamp, the host
    waits for it after queueing the rest, so the GPU never idles -- and a flagged call is REDONE on the fp32-MFMA kernels (with a
    warning, and split mode stays off for this model; mode "x3": RuntimeError).  No clamped result is ever returned.  "deferred"
    (r4's behaviour, for measuring what the check costs): the flag is only posted; ``check_overflow()`` or the next call looks at it.

    The two models spell their mode switch differently; the three attributes below carry the difference."""
    overflow_check = "call"
    _split_attr = "arithmetic"      # the public attribute that selects the mode ("x3": split mode or an error)
    _split_where = ""               # where the overflow happened, for the warning
    _check_raises = False           # check_overflow() in mode "x3": a RuntimeError like a flagged call (else the warning)

    @property
    def split_off(self) -> bool:
        """An overflow switched split mode off for this model (``reset_split_mode()`` turns it back on)."""
        return bool(self.__dict__.get("_snvc_x3_off"))

    def split_guard(self, device, mode):
        """This model's guard for ``device`` -- None if a flag that an earlier call only posted (``overflow_check = "deferred"``)
        turns out to be set: the model has left split mode then."""
        guard = overflow_guard(self, device)
        if guard.event is not None and self.overflowed(guard, mode, "an earlier call's result clamped it"):
            return None
        return guard

    def overflowed(self, guard, mode, what):
        """Look at a posted flag (synchronous).  True: a value was clamped -- split mode is switched off for this model."""
        return guard.wait() and self.leave(mode, what)

    def leave(self, mode, what):
        self.__dict__["_snvc_x3_off"] = True
        msg = ("snvc_amd: split-mode (f16x3) overflow%s -- an activation exceeded |beta| + %g |gamma| of its BatchNorm; %s.  "
               "This model now runs on the fp32-MFMA kernels (reset_split_mode() turns split mode back on)."
               % (self._split_where, X3_SIGMAS, what))
        if mode == "x3":
            raise RuntimeError("%s='x3': %s" % (self._split_attr, msg))
        warnings.warn(msg)
        return True

    def check_overflow(self) -> bool:
        """With ``overflow_check = "deferred"``: wait for the last split-mode call's flag.  True if that call's result was
        clamped (the model leaves split mode, as in the checked mode); always False in the default checked mode."""
        mode = getattr(self, self._split_attr) if self._check_raises else "auto"
        hit = False
        for guard in self.__dict__.get("_snvc_x3_guard", {}).values():
            hit |= self.overflowed(guard, mode, "the last result clamped it")
        return hit

    def reset_split_mode(self):
        """Turn split mode back on after an overflow switched it off (e.g. after loading matching statistics)."""
        self.__dict__.pop("_snvc_x3_off", None)

    def checked(self, mode, run_split, run_fp32):
        """Run a split-mode call; one whose overflow flag came back set is redone on the fp32-MFMA kernels (its clamped result
        never leaves).  One extra step, once per model: split mode stays off afterwards."""
        try:
            return run_split()
        except SplitOverflow:
            self.leave(mode, "this call was redone in fp32")
            from .submodule import _ROUTES
            _ROUTES["x3_overflow_redo"] += 1
            return run_fp32()
